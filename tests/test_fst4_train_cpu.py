"""CPU checks of the onehot FST training step (FARNN_S_O): the exported symbols, the C-ABI struct layouts,
the torch restatement against the loss / gradients / predictions captured from the reference, and the refusals that must
come before any device work."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import fst4_train_ref as ftr
from util import GOLDEN, check_grad, ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('farnn_fst4_train_create', 'farnn_fst4_train_destroy', 'farnn_fst4_train_step', 'farnn_fst4_train_set_profiling',
           'farnn_fst4_train_time')
N_CASES = 8


def _golden():
    with open(os.path.join(GOLDEN, 'fst4_train_small.json')) as f:
        meta = json.load(f)
    return meta['configs'], np.load(os.path.join(GOLDEN, 'fst4_train_small.npz'))


def case(k):
    """(configuration, inputs dict, captured dict) of captured configuration k; the captured language_tensor gradient is
    scattered back to [V, C, S, S] (the rows of absent words are zero: the generator asserted it)"""
    cfgs, g = _golden()
    cfg = cfgs[k]
    small = np.load(os.path.join(GOLDEN, 'fst4_small.npz'))
    if cfg['base'] == 'fst4_small':
        b = {n: small[n] for n in ('T4', 'W4', 'h0', 'hT', 'x', 'lengths')}
    else:
        b = {n: g['signed.' + n] for n in ('T4', 'W4', 'h0', 'hT', 'x', 'lengths')}
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


def test_the_library_exports_the_fst4_training_symbols():
    from re2nn_seq_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name
    with open(os.path.join(ROOT, 'include', 'farnn.h')) as f:
        hdr = f.read()
    for name in SYMBOLS:
        assert name + '(' in hdr, name


def test_ctypes_layouts_of_the_fst4_train_structs(tmp_path):
    from re2nn_seq_amd import _lib
    pairs = {'farnn_fst4_train_dims': _lib.Fst4TrainDims, 'farnn_fst4_train_weights': _lib.Fst4TrainWeights,
             'farnn_fst4_train_outputs': _lib.Fst4TrainOutputs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "farnn.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        lines.append('  printf("%s sizeof %zu\\n", "{0}", sizeof({0}));'.format(cname))
        for fname, _ in cls._fields_:
            lines.append('  printf("%s.%s %zu\\n", "{0}", "{1}", offsetof({0}, {1}));'.format(cname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = dict(line.rsplit(' ', 1) for line in out.strip().splitlines())
    for cname, cls in pairs.items():
        assert int(got[cname + ' sizeof']) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got['{}.{}'.format(cname, fname)]) == getattr(cls, fname).offset, (cname, fname)


@pytest.mark.parametrize('k', range(N_CASES))
def test_restatement_matches_the_reference_capture(k):
    """the float64 restatement against the float32 reference, at the gradient bar of tests/util.py"""
    cfg, inp, ref = case(k)
    ftr.check_gap(inp['T4'], inp['W4'], inp['h0'], inp['hT'], inp['x'], inp['lengths'])
    loss64, dT64, dW64, pred = ftr.step(dtype=torch.float64, **inp)
    loss32, dT32, dW32, pred32 = ftr.step(dtype=torch.float32, **inp)
    np.testing.assert_allclose(loss64, ref['loss'], rtol=2e-6, atol=1e-7)
    V = inp['T4'].shape[0]
    present = np.zeros(V, bool)
    present[ref['words']] = True
    assert np.abs(ref['dT4']).max() > 0
    check_grad('fst4-ref-c{}'.format(k), 'dT4', ref['dT4'], dT32, dT64, slices=0, present=present)
    if cfg['train_wildcard']:
        check_grad('fst4-ref-c{}'.format(k), 'dW4', ref['dW4'], dW32, dW64)
    assert np.array_equal(pred, ref['flat_pred']) and np.array_equal(pred32, ref['flat_pred'])


def _no_device(monkeypatch):
    """from here on no GPU is visible and any use of the HIP library fails the test"""
    from re2nn_seq_amd import _lib

    def boom(*a, **k):
        raise AssertionError('device work before the refusal')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(_lib, 'Fst4TrainContext', boom)
    monkeypatch.setattr(_lib, 'load', boom)


def _fst(**kw):
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O
    g = np.load(os.path.join(GOLDEN, 'fst4_small.npz'))
    S = g['T4'].shape[2]
    return FARNN_S_O(g['T4'], g['W4'], np.zeros((S, S)), g['hT'], g['h0'], None, ns(independent=0, **kw), o_idx=int(g['o_idx']))


def test_with_the_opt_in_and_no_device_enable_training_reports_the_missing_gpu(monkeypatch):
    from re2nn_seq_amd import _lib
    monkeypatch.setenv('RE2NN_ONEHOT_FST_TRAIN', '1')
    m = _fst()
    _no_device(monkeypatch)
    with pytest.raises(_lib.FarnnError, match='no MI355X visible'):
        m.enable_training()


def test_without_the_opt_in_the_refusal_is_unchanged(monkeypatch):
    from re2nn_seq_amd.train_onehot import check_trainable
    monkeypatch.delenv('RE2NN_ONEHOT_FST_TRAIN', raising=False)
    m = _fst()
    _no_device(monkeypatch)
    for call in (m.enable_training, lambda: check_trainable(m)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == ('training epochs are implemented for the i-FST models only (--independent 2: --method decompose, '
                                'DESIGN.md row f3, and --method onehot, row f5); FARNN_S_O has no training step, run it with '
                                '--epoch 0')


@pytest.mark.parametrize('kw,match', [(dict(train_mode='max'), 'sum semiring'), (dict(train_wildcard_wildcard=1), 'train_wildcard_wildcard'),
                                      (dict(local_loss_func='CE'), 'CE1')])
def test_uncovered_configurations_are_refused_before_device_work(monkeypatch, kw, match):
    monkeypatch.setenv('RE2NN_ONEHOT_FST_TRAIN', '1')
    m = _fst(**kw)
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError, match=match):
        m.enable_training()
    x = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(NotImplementedError, match=match):
        m.forward_local(x, x, torch.tensor([3, 2]), train=True)


def test_two_ranks_are_refused_before_device_work(monkeypatch):
    from re2nn_seq_amd import dist
    monkeypatch.setenv('RE2NN_ONEHOT_FST_TRAIN', '1')
    m = _fst()
    _no_device(monkeypatch)
    monkeypatch.setattr(dist, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='multi-GPU'):
        m.enable_training()


def test_independent_1_stays_refused_with_the_opt_in(monkeypatch):
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I
    from re2nn_seq_amd.train_onehot import check_trainable
    monkeypatch.setenv('RE2NN_ONEHOT_FST_TRAIN', '1')
    m = FARNN_S_O_I.__new__(FARNN_S_O_I)
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError, match='--epoch 0'):
        check_trainable(m)
