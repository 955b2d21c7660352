"""CPU checks of the onehot independent=1 training step (FARNN_S_O_I): the exported symbols, the C-ABI
struct layouts, the torch restatement against the loss / gradients / predictions captured from the reference, and the
refusals that must come before any device work."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import ind1_train_ref as itr
from util import GOLDEN, check_grad, ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('farnn_ind1_train_create', 'farnn_ind1_train_destroy', 'farnn_ind1_train_step', 'farnn_ind1_train_set_profiling',
           'farnn_ind1_train_time')
N_CASES = 8
REFUSAL = ('training epochs are implemented for the i-FST models only (--independent 2: --method decompose, '
           'DESIGN.md row f3, and --method onehot, row f5); FARNN_S_O_I has no training step, run it with '
           '--epoch 0')


def _golden():
    with open(os.path.join(GOLDEN, 'ind1_train_small.json')) as f:
        meta = json.load(f)
    return meta['configs'], np.load(os.path.join(GOLDEN, 'ind1_train_small.npz'))


def case(k):
    """(configuration, inputs dict, captured dict) of captured configuration k; the captured language_tensor gradient is
    scattered back to [V, S, S] (the rows of absent words are zero: the generator asserted it)"""
    cfgs, g = _golden()
    cfg = cfgs[k]
    small = np.load(os.path.join(GOLDEN, 'ind1_small.npz'))
    if cfg['base'] == 'ind1_small':
        b = dict(T=small['T'], W=small['W'], O=small['Oten'], h0=small['h0'], hT=small['hT'], x=small['x'],
                 lengths=small['lengths'])
    else:
        b = {n: g['signed.' + n] for n in ('T', 'W', 'O', 'h0', 'hT', 'x', 'lengths')}
    C = b['O'].shape[0]
    pri = np.eye(C, dtype=np.float32)
    if cfg['use_priority']:
        sp = np.load(os.path.join(GOLDEN, 'fst4_small.npz'))['priority']
        pri[:sp.shape[0], :sp.shape[0]] = sp
    inp = dict(T=b['T'].astype(np.float32), W=b['W'].astype(np.float32), O=b['O'].astype(np.float32),
               h0=b['h0'].astype(np.float32), hT=b['hT'].astype(np.float32), P=pri if cfg['use_priority'] else None,
               x=b['x'], lengths=b['lengths'], labels=g[cfg['base'] + '.labels'], mask=cfg['independent'] == 2,
               threshold=float(small['threshold']), o_idx=int(small['o_idx']))
    pre = 'c{}.'.format(k)
    dT = np.zeros(inp['T'].shape, np.float32)
    dT[g[pre + 'words']] = g[pre + 'g.language_tensor']
    ref = dict(loss=float(g[pre + 'loss']), dT=dT, words=g[pre + 'words'], flat_pred=g[pre + 'flat_pred'])
    return cfg, inp, ref


def test_the_library_exports_the_ind1_training_symbols():
    from re2nn_seq_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name
    with open(os.path.join(ROOT, 'include', 'farnn.h')) as f:
        hdr = f.read()
    for name in SYMBOLS:
        assert name + '(' in hdr, name


def test_ctypes_layouts_of_the_ind1_train_structs(tmp_path):
    from re2nn_seq_amd import _lib
    pairs = {'farnn_ind1_train_dims': _lib.Ind1TrainDims, 'farnn_ind1_train_weights': _lib.Ind1TrainWeights,
             'farnn_ind1_train_outputs': _lib.Ind1TrainOutputs}
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


def test_the_captures_cover_the_eight_configurations():
    cfgs, _ = _golden()
    want = {(b, up, ind) for b in ('ind1_small', 'signed') for up in (0, 1) for ind in (1, 2)}
    assert len(cfgs) == N_CASES and {(c['base'], c['use_priority'], c['independent']) for c in cfgs} == want


@pytest.mark.parametrize('k', range(N_CASES))
def test_restatement_matches_the_reference_capture(k):
    """the float64 restatement against the float32 reference, at the gradient bar of tests/util.py"""
    cfg, inp, ref = case(k)
    itr.check_gap(inp['T'], inp['W'], inp['O'], inp['h0'], inp['hT'], inp['x'], inp['lengths'], mask=inp['mask'])
    loss64, dT64, pred = itr.step(dtype=torch.float64, **inp)
    loss32, dT32, pred32 = itr.step(dtype=torch.float32, **inp)
    np.testing.assert_allclose(loss64, ref['loss'], rtol=2e-6, atol=1e-7)
    V = inp['T'].shape[0]
    present = np.zeros(V, bool)
    present[ref['words']] = True
    assert np.abs(ref['dT']).max() > 0
    check_grad('ind1-ref-c{}'.format(k), 'dT', ref['dT'], dT32, dT64, slices=0, present=present)
    assert np.array_equal(pred, ref['flat_pred']) and np.array_equal(pred32, ref['flat_pred'])


def test_the_mask_changes_the_signed_captures():
    """independent = 2 is another function on the signed base (on the 0/1 automaton the mask is one wherever N is not zero)"""
    assert case(4)[2]['loss'] != case(5)[2]['loss']


def _no_device(monkeypatch):
    """from here on no GPU is visible and any use of the HIP library fails the test"""
    from re2nn_seq_amd import _lib

    def boom(*a, **k):
        raise AssertionError('device work before the refusal')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(_lib, 'Ind1TrainContext', boom)
    monkeypatch.setattr(_lib, 'load', boom)


def _ind1(**kw):
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I
    g = np.load(os.path.join(GOLDEN, 'ind1_small.npz'))
    kw.setdefault('independent', 1)
    return FARNN_S_O_I(g['T'], g['Oten'], g['W'], None, g['hT'], g['h0'], None, ns(**kw), o_idx=int(g['o_idx']))


def test_with_the_opt_in_and_no_device_enable_training_reports_the_missing_gpu(monkeypatch):
    from re2nn_seq_amd import _lib
    monkeypatch.setenv('RE2NN_ONEHOT_IND1_TRAIN', '1')
    m = _ind1()
    _no_device(monkeypatch)
    with pytest.raises(_lib.FarnnError, match='no MI355X visible'):
        m.enable_training()


def test_without_the_opt_in_the_refusal_is_unchanged(monkeypatch):
    from re2nn_seq_amd.train_onehot import check_trainable
    monkeypatch.delenv('RE2NN_ONEHOT_IND1_TRAIN', raising=False)
    m = _ind1()
    _no_device(monkeypatch)
    x = torch.zeros((2, 3), dtype=torch.int64)
    for call in (m.enable_training, lambda: check_trainable(m), lambda: m.forward_local(x, x, torch.tensor([3, 2]), train=True)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == REFUSAL


def test_without_the_opt_in_a_bare_instance_is_refused_before_its_args_are_read(monkeypatch):
    """the environment variable is tested before self.args is touched: an instance without attributes gets the refusal"""
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I
    from re2nn_seq_amd.train_onehot import check_trainable
    monkeypatch.delenv('RE2NN_ONEHOT_IND1_TRAIN', raising=False)
    m = FARNN_S_O_I.__new__(FARNN_S_O_I)
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError) as e:
        check_trainable(m)
    assert str(e.value) == REFUSAL


@pytest.mark.parametrize('kw,match', [(dict(train_mode='max'), 'sum semiring'), (dict(local_loss_func='CE'), 'CE1')])
def test_uncovered_configurations_are_refused_before_device_work(monkeypatch, kw, match):
    from re2nn_seq_amd.train_onehot import check_trainable
    monkeypatch.setenv('RE2NN_ONEHOT_IND1_TRAIN', '1')
    m = _ind1(**kw)
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError, match=match):
        m.enable_training()
    with pytest.raises(NotImplementedError, match=match):
        check_trainable(m)
    x = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(NotImplementedError, match=match):
        m.forward_local(x, x, torch.tensor([3, 2]), train=True)


def test_two_ranks_are_refused_before_device_work(monkeypatch):
    from re2nn_seq_amd import dist
    monkeypatch.setenv('RE2NN_ONEHOT_IND1_TRAIN', '1')
    m = _ind1()
    _no_device(monkeypatch)
    monkeypatch.setattr(dist, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='multi-GPU'):
        m.enable_training()


def test_dense_tensors_of_an_edge_built_model_follow_the_out_of_vocabulary_rule():
    """_dense() of an edge-built model on the automaton of make_golden_oov.py (rule words outside the vocabulary): the tensors
    the reference's loader builds -- output_tensor keeps the label, language_tensor skips the edge"""
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I
    with open(os.path.join(GOLDEN, 'loader_small.json')) as f:
        meta = json.load(f)
    a = meta['automaton']
    automaton = {'states': set(a['states']), 'startstate': a['startstate'], 'finalstates': a['finalstates'],
                 'transitions': {int(fr): {int(to): set(e) for to, e in d.items()} for fr, d in a['transitions'].items()}}
    for fr, to, lab in [(0, 1, 'notaword<:>b-e1'), (2, 3, 'alsomissing<:>i-e2'), (1, 1, 'nope<:>oo')]:   # = make_golden_oov.OOV_EDGES
        automaton['transitions'].setdefault(fr, {}).setdefault(to, set()).add(lab)
    g = np.load(os.path.join(GOLDEN, 'loader_oov.npz'))
    m = FARNN_S_O_I.from_automaton(automaton, meta['t2i'], meta['s2i'], None, ns(independent=1), o_idx=meta['s2i']['o'])
    assert (m.edges[0] == -2).sum() >= 3
    T, W, O = m._dense()
    assert np.array_equal(T, g['ind.T']) and np.array_equal(W, g['ind.W']) and np.array_equal(O, g['ind.Oten'])
    sd = m.state_dict()
    assert np.array_equal(sd['language_tensor'], T) and np.array_equal(sd['output_tensor'], O)
