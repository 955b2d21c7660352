"""CPU checks of the onehot FST training step in the MAX semiring (--train_mode max): the torch restatement
(tests/fst4_max_train_ref.py) against the configurations captured from the reference, the planted faults that every fixture
must see, and the opt-in switch RE2NN_BUCKETED_MAX_TRAIN."""
import json
import os

import numpy as np
import pytest
import torch

import fst4_max_train_ref as fmr
from test_fst4_train_cpu import _fst, _no_device
from util import GOLDEN, check_grad

N_CASES = 8
KEYS = ('T4', 'W4', 'h0', 'hT', 'x', 'lengths')


def _golden():
    with open(os.path.join(GOLDEN, 'fst4_train_max_small.json')) as f:
        meta = json.load(f)
    return meta['configs'], np.load(os.path.join(GOLDEN, 'fst4_train_max_small.npz'))


def case(k):
    """(configuration, inputs dict, captured dict) of captured configuration k (the layout of test_fst4_train_cpu.case)"""
    cfgs, g = _golden()
    cfg = cfgs[k]
    small = np.load(os.path.join(GOLDEN, 'fst4_small.npz'))
    b = {n: (small[n] if cfg['base'] == 'fst4_small' else g['signed.' + n]) for n in KEYS}
    C = b['W4'].shape[0]
    pri = np.eye(C, dtype=np.float32)
    if cfg['use_priority']:
        sp = small['priority']
        pri[:sp.shape[0], :sp.shape[0]] = sp
    inp = dict(T4=b['T4'].astype(np.float32), W4=b['W4'].astype(np.float32), h0=b['h0'].astype(np.float32),
               hT=b['hT'].astype(np.float32), P=pri if cfg['use_priority'] else None, x=b['x'], lengths=b['lengths'],
               labels=g[cfg['base'] + '.labels'], threshold=float(small['threshold']), o_idx=int(small['o_idx']))
    pre = 'c{}.'.format(k)
    dT4 = np.zeros(inp['T4'].shape, np.float32)
    dT4[g[pre + 'words']] = g[pre + 'g.language_tensor']
    ref = dict(loss=float(g[pre + 'loss']), dT4=dT4, words=g[pre + 'words'], flat_pred=g[pre + 'flat_pred'],
               dW4=g[pre + 'g.wildcard_tensor'] if cfg['train_wildcard'] else None)
    return cfg, inp, ref


def test_the_captures_cover_the_eight_configurations():
    cfgs, _ = _golden()
    assert len(cfgs) == N_CASES and all(c['train_mode'] == 'max' for c in cfgs)
    assert {(c['base'], c['use_priority'], c['train_wildcard']) for c in cfgs} == \
        {(b, u, w) for b in ('fst4_small', 'signed') for u in (0, 1) for w in (0, 1)}


def _present(inp, ref):
    present = np.zeros(inp['T4'].shape[0], bool)
    present[ref['words']] = True
    return present


@pytest.mark.parametrize('k', range(N_CASES))
def test_restatement_matches_the_reference_capture(k):
    """the float32 and float64 restatement against the float32 reference, at the gradient bar of tests/util.py; the gap rule
    holds on every stored configuration"""
    cfg, inp, ref = case(k)
    fmr.check_gap(*(inp[n] for n in KEYS))
    loss64, dT64, dW64, pred = fmr.step(dtype=torch.float64, **inp)
    loss32, dT32, dW32, pred32 = fmr.step(dtype=torch.float32, **inp)
    np.testing.assert_allclose(loss64, ref['loss'], rtol=2e-6, atol=1e-7)
    assert np.abs(ref['dT4']).max() > 0
    check_grad('fst4-max-ref-c{}'.format(k), 'dT4', ref['dT4'], dT32, dT64, slices=0, present=_present(inp, ref))
    if cfg['train_wildcard']:
        check_grad('fst4-max-ref-c{}'.format(k), 'dW4', ref['dW4'], dW32, dW64)
    assert np.array_equal(pred, ref['flat_pred']) and np.array_equal(pred32, ref['flat_pred'])


@pytest.mark.parametrize('fault', ['sum', 'last', 'fwd_idx'])
@pytest.mark.parametrize('k', range(N_CASES))
def test_every_fixture_sees_the_planted_fault(k, fault):
    """from the restatement alone: with the fault planted, the capture's gradient no longer passes the bar"""
    cfg, inp, ref = case(k)
    _, dT64, _, _ = fmr.step(dtype=torch.float64, fault=fault, **inp)
    _, dT32, _, _ = fmr.step(dtype=torch.float32, fault=fault, **inp)
    with pytest.raises(AssertionError):
        check_grad('fst4-max-fault-c{}'.format(k), 'dT4', ref['dT4'], dT32, dT64, slices=0, present=_present(inp, ref))


def test_with_both_switches_and_no_device_enable_training_reports_the_missing_gpu(monkeypatch):
    from re2nn_seq_amd import _lib
    monkeypatch.setenv('RE2NN_ONEHOT_FST_TRAIN', '1')
    monkeypatch.setenv('RE2NN_BUCKETED_MAX_TRAIN', '1')
    m = _fst(train_mode='max')
    _no_device(monkeypatch)
    with pytest.raises(_lib.FarnnError, match='no MI355X visible'):
        m.enable_training()


def test_with_the_model_switch_alone_the_refusal_is_todays(monkeypatch):
    from re2nn_seq_amd.train_onehot import check_trainable
    monkeypatch.setenv('RE2NN_ONEHOT_FST_TRAIN', '1')
    monkeypatch.delenv('RE2NN_BUCKETED_MAX_TRAIN', raising=False)
    m = _fst(train_mode='max')
    _no_device(monkeypatch)
    x = torch.zeros((2, 3), dtype=torch.int64)
    want = 'training the onehot FST covers the sum semiring only, --train_mode max was asked for (DESIGN.md, row f7)'
    for call in (m.enable_training, lambda: check_trainable(m), lambda: m.forward_local(x, x, torch.tensor([3, 2]), train=True)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == want


def test_the_other_refusals_stay_with_both_switches(monkeypatch):
    from re2nn_seq_amd import dist
    monkeypatch.setenv('RE2NN_ONEHOT_FST_TRAIN', '1')
    monkeypatch.setenv('RE2NN_BUCKETED_MAX_TRAIN', '1')
    _no_device(monkeypatch)
    for kw, match in ((dict(local_loss_func='CE'), 'CE1'), (dict(train_wildcard_wildcard=1), 'train_wildcard_wildcard')):
        with pytest.raises(NotImplementedError, match=match):
            _fst(train_mode='max', **kw).enable_training()
    m = _fst(train_mode='max')
    monkeypatch.setattr(dist, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='multi-GPU'):
        m.enable_training()
