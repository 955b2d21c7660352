"""CPU checks of the onehot i-FST training step in the max semiring (--train_mode max): the torch
restatement against the loss / gradient / predictions captured from the reference, the binding of the new C-ABI entry, and
the opt-in switch RE2NN_ONEHOT_MAX_TRAIN of the model mirror."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import onehot_train_max_ref as omr
from util import GOLDEN, ns

N_CASES = 16
MIN_GAP = 2e-5


def case(k):
    """(config, inputs dict, captured dict) of captured configuration k of ifst_train_max_small"""
    with open(os.path.join(GOLDEN, 'ifst_train_max_small.json')) as f:
        cfg = json.load(f)['configs'][k]
    g = np.load(os.path.join(GOLDEN, 'ifst_train_max_small.npz'))
    base = np.load(os.path.join(GOLDEN, cfg['base'] + '.npz'))
    C = base['O'].shape[0]
    pri = np.eye(C, dtype=np.float32)
    if cfg['use_priority']:
        sp = np.load(os.path.join(GOLDEN, 'ifst_small.npz'))['priority']
        pri[:sp.shape[0], :sp.shape[0]] = sp
    inp = dict(T=base['T'].astype(np.float32), W=base['W'].astype(np.float32), O=base['O'].astype(np.float32),
               h0=base['h0'].astype(np.float32), hT=base['hT'].astype(np.float32),
               P=pri if cfg['use_priority'] else None, x=base['x'], lengths=base['lengths'],
               labels=g[cfg['base'] + '.labels'], nl=cfg['update_nonlinear'], threshold=float(base['threshold']),
               o_idx=int(base['o_idx']))
    pre = 'c{}.'.format(k)
    ref = dict(loss=float(g[pre + 'loss']), dT=g[pre + 'g.language_tensor'], flat_pred=g[pre + 'flat_pred'])
    return cfg, inp, ref


@pytest.mark.parametrize('k', range(N_CASES))
def test_restatement_matches_the_reference_capture(k):
    cfg, inp, ref = case(k)
    assert cfg['train_mode'] == 'max'
    loss, dT, pred = omr.step(dtype=torch.float32, min_gap=MIN_GAP, **inp)
    np.testing.assert_allclose(loss, ref['loss'], rtol=2e-6, atol=1e-7)
    scale = float(np.abs(ref['dT']).max())
    np.testing.assert_allclose(dT, ref['dT'], rtol=1e-5, atol=1e-6 * scale)
    assert np.array_equal(pred, ref['flat_pred'])


def test_the_gap_rule_refuses_a_near_tie_and_accepts_an_exact_one():
    """two source states with equal inputs and equal matrix entries tie exactly in both evaluations (accepted, the first
    index wins); an entry moved by one part in 1e6 is decided by rounding-sized margins (refused); an exact-zero maximum is
    exempt"""
    S, V = 3, 2
    T = np.zeros((V, S, S), np.float32)
    W = np.zeros((S, S), np.float32)
    T[:, 0, :] = 0.7
    T[:, 1, :] = 0.7
    O = np.array([[1.0, 0.25, 0.5], [0.25, 1.0, 0.75]], np.float32)      # equal column sums: o keeps the ties
    h0 = np.array([0.3, 0.3, 0.0], np.float32)
    hT = np.array([0.3, 0.3, 0.0], np.float32)
    x, lengths = np.array([[0, 1, 0]]), np.array([3])
    omr.check_gap(T, W, O, h0, hT, x, lengths, 'none', MIN_GAP)
    Tn = T.copy()
    Tn[:, 1, :] *= np.float32(1 + 1e-6)
    with pytest.raises(omr.GapError):
        omr.check_gap(Tn, W, O, h0, hT, x, lengths, 'none', MIN_GAP)
    omr.check_gap(np.zeros_like(T), W, O, h0, hT, x, lengths, 'none', MIN_GAP)
    # the first maximal index takes the whole adjoint: entries (0, s) from the forward chain, (s, 0) from the backward chain
    _, dT, _ = omr.step(T, W, O, h0, hT, None, x, lengths, np.array([[0, 1, 0]]), dtype=torch.float64)
    assert dT[:, 0, :].any() and not dT[:, 1:, 1:].any()


def test_ctypes_signature_of_the_semiring_entry():
    from re2nn_seq_amd import _lib
    res, args = _lib.SIGNATURES['farnn_onehot_train_set_semiring']
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_int32]
    assert _lib.SIGNATURES['farnn_onehot_train_set_semiring'] == _lib.SIGNATURES['farnn_train_set_semiring']
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, 'farnn_onehot_train_set_semiring')
    with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, 'include', 'farnn.h')) as f:
        assert 'int  farnn_onehot_train_set_semiring(farnn_onehot_train_ctx *ctx, int32_t semiring);' in f.read()


def _ifst(**kw):
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I_S
    g = np.load(os.path.join(GOLDEN, 'ifst_small.npz'))
    S = g['T'].shape[1]
    return FARNN_S_O_I_S(g['T'], g['O'], g['W'], np.zeros(S), g['hT'], g['h0'], None, ns(**kw), o_idx=int(g['o_idx']))


def _boom(*a, **k):
    raise AssertionError('device work before the refusal')


@pytest.mark.parametrize('value', [None, '0', 'yes'])
def test_without_the_switch_the_max_model_is_still_refused_before_device_work(monkeypatch, value):
    from re2nn_seq_amd import _lib
    if value is None:
        monkeypatch.delenv('RE2NN_ONEHOT_MAX_TRAIN', raising=False)
    else:
        monkeypatch.setenv('RE2NN_ONEHOT_MAX_TRAIN', value)
    m = _ifst(train_mode='max')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(_lib, 'OnehotTrainContext', _boom)
    monkeypatch.setattr(_lib, 'load', _boom)
    with pytest.raises(NotImplementedError, match='sum semiring') as e:
        m.enable_training()
    assert 'RE2NN_ONEHOT_MAX_TRAIN' in str(e.value)
    x = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(NotImplementedError, match='sum semiring'):
        m.forward_local(x, x, torch.tensor([3, 2]), train=True)


class _Reached(Exception):
    pass


@pytest.mark.parametrize('train_mode', ['max', 'sum'])
def test_with_the_switch_the_context_is_created_with_the_models_semiring(monkeypatch, train_mode):
    from re2nn_seq_amd import _lib
    from re2nn_seq_amd.farnn import model_onehot
    monkeypatch.setenv('RE2NN_ONEHOT_MAX_TRAIN', '1')
    m = _ifst(train_mode=train_mode)
    m._check_trainable()                           # the refusal is gone
    seen = {}

    def stub(*a, **k):
        seen.update(k)
        raise _Reached()
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(model_onehot.FARNN_S_O_I_S, '_dev', lambda self: torch.device('cpu'))
    monkeypatch.setattr(_lib, 'OnehotTrainContext', stub)
    with pytest.raises(_Reached):
        m.enable_training()
    assert seen['semiring'] == train_mode


def test_an_unknown_semiring_name_is_refused_before_a_context_exists(monkeypatch):
    from re2nn_seq_amd import _lib
    monkeypatch.setattr(_lib, 'load', _boom)
    with pytest.raises(ValueError, match='semiring'):
        _lib.OnehotTrainContext(5, 3, 2, semiring='min')
