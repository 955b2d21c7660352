"""CPU checks of the decomposed independent=1 training step (FARNN_S_D_W_I): the exported symbols, the
C-ABI struct layouts, the torch restatement against the loss / gradients / predictions captured from the reference, and the
refusals that must come before any device work."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import decomp1_train_ref as dtr
from util import GOLDEN, assert_float_path, check_grad, ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('farnn_decomp_ind1_train_create', 'farnn_decomp_ind1_train_destroy', 'farnn_decomp_ind1_train_step',
           'farnn_decomp_ind1_train_set_profiling', 'farnn_decomp_ind1_train_time')
N_CASES = 18
PARAMS = dtr.FLOAT_KEYS + dtr.VGEN_KEYS
WORD_ROWS = ('V_embed', 'embedding.weight')
FLAGS = dict(train_wildcard=1, train_wildcard_wildcard=1, train_h0=1, train_hT=1, train_V_embed=1, train_word_embed=1,
             train_beta=1, beta=0.7)
REFUSAL = ('training epochs are implemented for the i-FST models only (--independent 2: --method decompose, '
           'DESIGN.md row f3, and --method onehot, row f5); FARNN_S_D_W_I has no training step, run it with '
           '--epoch 0')


def _golden():
    with open(os.path.join(GOLDEN, 'decomp1_train_small.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, 'decomp1_train_small.npz'))


def case(k):
    """(configuration, inputs dict, captured dict) of captured configuration k; the captured gradients of V_embed and
    embedding.weight are scattered back to all V rows (the rows of absent words are zero: the generator asserted it)"""
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


def check_all_grads(name, got, g32, g64, present):
    """util.check_grad on every tensor; the word-indexed ones by word slices"""
    for n in sorted(g64):
        check_grad(name, n, got[n], g32[n], g64[n], slices=0 if n in WORD_ROWS + ('Vgen',) else None,
                   present=present if n in WORD_ROWS + ('Vgen',) else None)


def test_the_library_exports_the_decomp_ind1_training_symbols():
    from re2nn_seq_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, 'include', 'farnn.h')) as f:
        hdr = f.read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name
        assert name + '(' in hdr, name


def test_ctypes_layouts_of_the_decomp_ind1_train_structs(tmp_path):
    from re2nn_seq_amd import _lib
    pairs = {'farnn_decomp_ind1_train_dims': _lib.Decomp1TrainDims, 'farnn_decomp_ind1_train_weights': _lib.Decomp1TrainWeights,
             'farnn_decomp_ind1_train_outputs': _lib.Decomp1TrainOutputs}
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


def test_the_captures_cover_the_configurations():
    cfgs = _golden()[0]['configs']
    want = {(b, nl, up) for b in ('decomp_ind1_small', 'signed') for nl in ('none', 'relu', 'tanh', 'relutanh') for up in (0, 1)}
    assert len(cfgs) == N_CASES
    assert {(c['base'], c['update_nonlinear'], c['use_priority']) for c in cfgs[:16]} == want
    assert cfgs[16].get('additional_states') == 2 and cfgs[17].get('additional_nonlinear') == 'tanh'


@pytest.mark.parametrize('k', range(N_CASES))
def test_restatement_matches_the_reference_capture(k):
    """the float32 and float64 restatement against the float32 reference, at the bars of tests/util.py"""
    cfg, inp, ref = case(k)
    dtr.check_gap(inp['p'], inp['P'], inp['x'], inp['lengths'], nl=inp['nl'], add_nl=inp['add_nl'], threshold=inp['threshold'],
                  min_gap=2e-5 if cfg['base'] == 'signed' else 0.0)
    loss64, g64, pred = dtr.step(dtype=torch.float64, **inp)
    loss32, g32, pred32 = dtr.step(dtype=torch.float32, **inp)
    assert_float_path(ref['loss'], loss32, loss64, err_msg='loss')
    V = inp['p']['V_embed'].shape[0]
    present = np.zeros(V, bool)
    present[ref['words']] = True
    assert set(ref['grads']) == set(PARAMS)
    for n in PARAMS:
        assert np.abs(ref['grads'][n]).max() > 0, n
    check_all_grads('decomp1-ref-c{}'.format(k), ref['grads'], g32, g64, present)
    assert np.array_equal(pred, ref['flat_pred']) and np.array_equal(pred32, ref['flat_pred'])


def test_the_chains_carry_gradient_into_the_output_factors():
    """both Osum paths: without the chains' share (dMc = 0) the output factors' gradients are other numbers"""
    _, inp, _ = case(12)
    full = dtr.step(dtype=torch.float64, **inp)[1]
    cut = dtr.step(dtype=torch.float64, detach_chains=True, **inp)[1]
    for n in ('C_output', 'S1_output', 'S2_output'):
        assert np.abs(full[n] - cut[n]).max() > 1e-3 * np.abs(full[n]).max(), n


def _no_device(monkeypatch):
    """from here on no GPU is visible and any use of the HIP library fails the test"""
    from re2nn_seq_amd import _lib

    def boom(*a, **k):
        raise AssertionError('device work before the refusal')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(_lib, 'Decomp1TrainContext', boom)
    monkeypatch.setattr(_lib, 'TrainContext', boom)
    monkeypatch.setattr(_lib, 'load', boom)


def model(k=0, **kw):
    """the mirror built from captured configuration k's parameters (every train_* flag on unless kw says otherwise)"""
    from re2nn_seq_amd.farnn.model_decompose_independent import FARNN_S_D_W_I
    cfg, inp, _ = case(k)
    p = inp['p']
    a = ns(independent=1, threshold=inp['threshold'], **dict(FLAGS, **dict({q: v for q, v in cfg.items() if q != 'base'}, **kw)))
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


def test_with_the_opt_in_and_no_device_enable_training_reports_the_missing_gpu(monkeypatch):
    from re2nn_seq_amd import _lib
    monkeypatch.setenv('RE2NN_DECOMP_IND1_TRAIN', '1')
    m = model()
    _no_device(monkeypatch)
    with pytest.raises(_lib.FarnnError, match='no MI355X visible'):
        m.enable_training()


def test_without_the_opt_in_the_model_is_refused_before_device_work(monkeypatch):
    from re2nn_seq_amd.farnn.model_decompose_independent import FARNN_S_D_W_I
    from re2nn_seq_amd.train_onehot import check_trainable
    monkeypatch.delenv('RE2NN_DECOMP_IND1_TRAIN', raising=False)
    m = model()
    bare = FARNN_S_D_W_I.__new__(FARNN_S_D_W_I)               # the refusal needs the type only
    _no_device(monkeypatch)
    x = torch.zeros((2, 3), dtype=torch.int64)
    for call in (m.enable_training, lambda: check_trainable(m), lambda: check_trainable(bare),
                 lambda: m.forward_local(x, x, torch.tensor([3, 2]), train=True)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == REFUSAL


@pytest.mark.parametrize('kw,match', [(dict(farnn=1), 'farnn 1'), (dict(farnn=2), 'farnn 2'), (dict(train_mode='max'), 'train_mode max'),
                                      (dict(use_crf=1), 'use_crf 1'), (dict(marryup_type='kd'), 'marryup_type kd'),
                                      (dict(marryup_type='pr'), 'marryup_type pr')])
def test_uncovered_configurations_are_refused_before_device_work(monkeypatch, kw, match):
    from re2nn_seq_amd.train_onehot import check_trainable
    monkeypatch.setenv('RE2NN_DECOMP_IND1_TRAIN', '1')
    m = model(**kw)
    _no_device(monkeypatch)
    x = torch.zeros((2, 3), dtype=torch.int64)
    for call in (m.enable_training, lambda: check_trainable(m), lambda: m.forward_local(x, x, torch.tensor([3, 2]), train=True)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert match in str(e.value) and 'row f9' in str(e.value), str(e.value)


def test_two_ranks_are_refused_before_device_work(monkeypatch):
    from re2nn_seq_amd import dist
    monkeypatch.setenv('RE2NN_DECOMP_IND1_TRAIN', '1')
    m = model()
    _no_device(monkeypatch)
    monkeypatch.setattr(dist, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='multi-GPU.*row f9'):
        m.enable_training()
