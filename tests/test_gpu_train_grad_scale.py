"""The three HIP training steps held to the gradient rule (tests/util.py:assert_grad_path): every gradient within 1e-4 of
its float64 oracle at the tensor's OWN scale, the word-indexed ones (dVgen's rows, dT's [S, S] blocks) also at each present
word's own scale, and exactly zero for the words that occur at no valid position (the output buffers are pre-filled).

What runs here that ran nowhere before (the draws are tests/train_grad_cases.py's, whose references
tests/test_train_grad_faults.py checks on the CPU):
  * the production vocabulary (V = 11 000, S = 104, R = 250, B = 256, L = 64, Zipf tokens): the sum step with farnn 0 / CE1
    and farnn 2 / CRF, dVgen included -- the one gradient scattered by token id with float atomics; the max step at the same
    V, S, R on B = 32, L = 16 (the restatement needs every maximum of the batch decided by more than 2e-5, which bounds the
    batch: train_grad_cases.PROD_MAX);
  * word counts planted on the bucketing boundaries (1, 31, 32, 33, 63, 64, 65, 257 valid occurrences; a word only at the
    last valid position of the last non-empty sequence; a word only behind sequence ends; valid positions on both sides of
    flat position 256), one batch per step; 63, 64, 65 and 129 distinct words for the max step's 64 word chunks;
  * the onehot step on dense states (T and W small positive floats): more than half of the present words' dT entries
    are non-zero, where the 0/1 automata of the other tests leave 99.8 % of them zero.
Every step goes through the C-ABI; one context per test, closed.  With TRAIN_GRAD_REPORT set, each comparison appends its
figures to that file (profiles/train_grad_error.txt)."""
import numpy as np
import pytest
import torch

import train_grad_cases as tg
from test_gpu_onehot_train import run_step_c_abi
from test_gpu_train_envelope import SumRun
from test_gpu_train_max import run_library
from util import assert_float_path, check_grad

pytestmark = pytest.mark.gpu


def run_case(case):
    """(loss, {name: gradient}) of the library on the case, through the C-ABI"""
    from re2nn_seq_amd import _lib
    if case['step'] == 'onehot':
        loss, dT = run_step_c_abi(case['c'], case['nl'])
        return loss, {'T': dT}
    if case['step'] == 'max':
        res, tc = run_library(case['w'], case['x'], case['lengths'], case['labels'], case['nl'], case['farnn'], case['crf'])
        tc.close()
    else:
        p = case['p']
        V, R = p['V_embed'].shape
        tc = _lib.TrainContext(V, p['S1'].shape[0], R, p['C_output_mat'].shape[0], nl=case['nl'], threshold=0.5, o_idx=1,
                               use_crf=case['crf'], farnn=case['farnn'], sigmoid_exponent=case['sig_k'])
        try:
            res = SumRun(p, case['x'], case['lengths'], case['labels'], case['farnn'], case['crf']).step(tc)
        finally:
            tc.close()
    return res['loss'], {n[1:]: v for n, v in res.items() if n.startswith('d')}


def check_case(name, case):
    ref32, ref64 = tg.refs(case)
    loss, got = run_case(case)
    assert_float_path([loss], [ref32[0]], [ref64[0]], err_msg=name + ' loss')
    assert set(got) == set(ref64[1]), (sorted(got), sorted(ref64[1]))
    for n in ref64[1]:
        assert_float_path(np.asarray(got[n]).reshape(ref64[1][n].shape), ref32[1][n], ref64[1][n], err_msg=name + ' d' + n)
    tg.check_all(name, got, ref32, ref64, tg.present_of(case), check_grad)
    return ref64


@pytest.mark.parametrize('name', ['prod-sum-farnn0-ce1', 'prod-sum-farnn2-crf', 'prod-max-farnn2-crf'])
def test_production_vocabulary(name):
    case = tg.GPU_CASES[name]()
    d = tg.PROD_MAX if case['step'] == 'max' else tg.PROD
    x, lengths = tg.batch_of(case)
    assert case['V'] == 11000 and x.shape == (d['B'], d['L'])
    present = tg.present_of(case)
    assert present.sum() > 100 and not present.all()          # many words, and most of the table absent
    check_case(name, case)


@pytest.mark.parametrize('step', ['sum', 'max', 'onehot'])
def test_planted_word_counts(step):
    name = 'planted-' + step
    case = tg.GPU_CASES[name]()
    x, lengths = tg.batch_of(case)
    tg.assert_planted(x, lengths, case['info'])               # the counts, before the library is called
    check_case(name, case)


@pytest.mark.parametrize('n_words', [63, 64, 65, 129])
def test_max_step_distinct_word_counts(n_words):
    name = 'max-{}-words'.format(n_words)
    case = tg.GPU_CASES[name]()
    assert int(tg.present_of(case).sum()) == n_words
    check_case(name, case)


@pytest.mark.parametrize('nl', ['none', 'tanh'])
@pytest.mark.parametrize('S', [32, 72, 96, 128])
def test_onehot_step_dense_states(S, nl):
    name = 'dense-onehot-S{}-{}'.format(S, nl)
    case = tg.GPU_CASES[name]()
    ref64 = check_case(name, case)
    assert tg.dense_share(case, ref64) > 0.5
