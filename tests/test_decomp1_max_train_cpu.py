"""CPU checks of the decomposed independent=1 training step in the MAX semiring (--train_mode max): the
torch restatement (tests/decomp1_max_train_ref.py) against the configurations captured from the reference, the planted faults
that every fixture must see (the dropped row-0 carry of dh0 / dhT among them), and the opt-in switch RE2NN_BUCKETED_MAX_TRAIN."""
import json
import os

import numpy as np
import pytest
import torch

import decomp1_max_train_ref as dmr
from test_decomp1_train_cpu import FLAGS, N_CASES, PARAMS, WORD_ROWS, _no_device, check_all_grads
from util import GOLDEN, assert_float_path, check_grad, ns


def _golden():
    with open(os.path.join(GOLDEN, 'decomp1_train_max_small.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, 'decomp1_train_max_small.npz'))


def case(k):
    """(configuration, inputs dict, captured dict) of captured configuration k (the layout of test_decomp1_train_cpu.case)"""
    meta, g = _golden()
    cfg = meta['configs'][k]
    pre = 'c{}.'.format(k)
    p = {n: g[pre + 'p.' + n].astype(np.float32) for n in PARAMS}
    inp = dict(p=p, P=g[pre + 'priority'].astype(np.float32) if cfg['use_priority'] else None, x=g[cfg['base'] + '.x'],
               lengths=g[cfg['base'] + '.lengths'], labels=g[cfg['base'] + '.labels'], nl=cfg['update_nonlinear'],
               add_nl=cfg.get('additional_nonlinear', 'none'), threshold=float(meta['threshold']), o_idx=int(meta['o_idx']))
    grads = {}
    for n in PARAMS:
        gr = g[pre + 'g.' + n]
        if n in WORD_ROWS:
            full = np.zeros(p[n].shape, np.float32)
            full[g[pre + 'words']] = gr
            gr = full
        grads[n] = gr
    ref = dict(loss=float(g[pre + 'loss']), grads=grads, words=g[pre + 'words'], flat_pred=g[pre + 'flat_pred'])
    return cfg, inp, ref


def model(k=0, **kw):
    """the mirror built from captured configuration k's parameters, --train_mode max (every train_* flag on unless kw says
    otherwise)"""
    from re2nn_seq_amd.farnn.model_decompose_independent import FARNN_S_D_W_I
    cfg, inp, _ = case(k)
    p = inp['p']
    a = ns(independent=1, threshold=inp['threshold'],
           **dict(FLAGS, **dict({q: v for q, v in cfg.items() if q != 'base'}, **dict(dict(train_mode='max'), **kw))))
    a.additional_states, a.rand_constant = 0, 0.0            # the captured tensors are already padded
    S = p['S1'].shape[0]
    m = FARNN_S_D_W_I(V=p['V_embed'], S1=p['S1'], S2=p['S2'], C_output=p['C_output'], S1_output=p['S1_output'],
                      S2_output=p['S2_output'], wildcard_mat=p['wildcard_mat'], wildcard_output=np.zeros((S, S), np.float32),
                      final_vector=p['hT'], start_vector=p['h0'], pretrained_word_embed=p['embedding.weight'],
                      priority_mat=None, args=a, o_idx=inp['o_idx'])
    m.load_state_dict({n: torch.from_numpy(p[n]) for n in PARAMS})
    if inp['P'] is not None:
        m.priority_full = inp['P']
    return m


def _present(inp, ref):
    present = np.zeros(inp['p']['V_embed'].shape[0], bool)
    present[ref['words']] = True
    return present


def test_the_captures_cover_the_configurations():
    meta, _ = _golden()
    cfgs = meta['configs']
    assert len(cfgs) == N_CASES and meta['train_mode'] == 'max'
    assert {(c['base'], c['update_nonlinear'], c['use_priority']) for c in cfgs[:16]} == \
        {(b, nl, u) for b in ('decomp_ind1_small', 'signed') for nl in ('none', 'relu', 'tanh', 'relutanh') for u in (0, 1)}


@pytest.mark.parametrize('k', range(N_CASES))
def test_restatement_matches_the_reference_capture(k):
    """the float32 and float64 restatement against the float32 reference, at the bars of tests/util.py; the gap rule holds on
    every stored configuration"""
    cfg, inp, ref = case(k)
    dmr.check_gap(inp['p'], inp['P'], inp['x'], inp['lengths'], nl=inp['nl'], add_nl=inp['add_nl'], min_gap=2e-5,
                  relu_gap=2e-5 if cfg['base'] == 'signed' else 0.0)
    loss64, g64, pred = dmr.step(dtype=torch.float64, **inp)
    loss32, g32, pred32 = dmr.step(dtype=torch.float32, **inp)
    assert_float_path(ref['loss'], loss32, loss64, err_msg='loss')
    for n in PARAMS:
        assert np.abs(ref['grads'][n]).max() > 0, n
    check_all_grads('decomp1-max-ref-c{}'.format(k), ref['grads'], g32, g64, _present(inp, ref))
    assert np.array_equal(pred, ref['flat_pred']) and np.array_equal(pred32, ref['flat_pred'])


@pytest.mark.parametrize('fault', ['sum', 'last', 'fwd_idx', 'no_carry0'])
@pytest.mark.parametrize('k', range(N_CASES))
def test_every_fixture_sees_the_planted_fault(k, fault):
    """from the restatement alone: with the fault planted, a captured gradient no longer passes the bar (the dropped row-0
    carry is looked for where it acts: in dh0 and dhT).  The last-index fault shows on the relu configurations too because
    the capture script plants exact non-zero ties (a twin state: make_golden_train_decomp1_max.py)"""
    cfg, inp, ref = case(k)
    g64 = dmr.step(dtype=torch.float64, fault=fault, **inp)[1]
    g32 = dmr.step(dtype=torch.float32, fault=fault, **inp)[1]
    with pytest.raises(AssertionError):
        if fault == 'no_carry0':
            for n in ('h0', 'hT'):
                check_grad('decomp1-max-fault-c{}'.format(k), n, ref['grads'][n], g32[n], g64[n])
        else:
            check_all_grads('decomp1-max-fault-c{}'.format(k), ref['grads'], g32, g64, _present(inp, ref))


def test_with_both_switches_and_no_device_enable_training_reports_the_missing_gpu(monkeypatch):
    from re2nn_seq_amd import _lib
    monkeypatch.setenv('RE2NN_DECOMP_IND1_TRAIN', '1')
    monkeypatch.setenv('RE2NN_BUCKETED_MAX_TRAIN', '1')
    m = model()
    _no_device(monkeypatch)
    with pytest.raises(_lib.FarnnError, match='no MI355X visible'):
        m.enable_training()


def test_with_the_model_switch_alone_the_refusal_is_todays(monkeypatch):
    from re2nn_seq_amd.train_onehot import check_trainable
    monkeypatch.setenv('RE2NN_DECOMP_IND1_TRAIN', '1')
    monkeypatch.delenv('RE2NN_BUCKETED_MAX_TRAIN', raising=False)
    m = model()
    _no_device(monkeypatch)
    x = torch.zeros((2, 3), dtype=torch.int64)
    want = ('training the decomposed independent=1 model covers farnn 0, the sum semiring and the CE1 loss on one GPU; the max '
            'semiring (--train_mode max) is not built (DESIGN.md, row f9)')
    for call in (m.enable_training, lambda: check_trainable(m), lambda: m.forward_local(x, x, torch.tensor([3, 2]), train=True)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == want


@pytest.mark.parametrize('kw,match', [(dict(farnn=1), 'farnn 1'), (dict(use_crf=1), 'use_crf 1'), (dict(marryup_type='kd'), 'marryup_type kd'),
                                      (dict(local_loss_func='CE'), 'CE1')])
def test_the_other_refusals_stay_with_both_switches(monkeypatch, kw, match):
    monkeypatch.setenv('RE2NN_DECOMP_IND1_TRAIN', '1')
    monkeypatch.setenv('RE2NN_BUCKETED_MAX_TRAIN', '1')
    m = model(**kw)
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError) as e:
        m.enable_training()
    assert match in str(e.value) and 'row f9' in str(e.value), str(e.value)
