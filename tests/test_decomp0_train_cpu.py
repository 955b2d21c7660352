"""CPU checks of the decomposed FST's training step (FARNN_S_D_W): the exported symbols, the C-ABI struct
layouts, the torch restatement against the loss / gradients / predictions captured from the reference
(tests/golden/decomp0_train_small) and against its captured tagging scores, and the refusals that must come before any device
work."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import decomp0_train_ref as d0r
from util import GOLDEN, assert_float_path, check_grad, ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('farnn_decomp_fst_train_create', 'farnn_decomp_fst_train_destroy', 'farnn_decomp_fst_train_step',
           'farnn_decomp_fst_train_set_profiling', 'farnn_decomp_fst_train_time')
FLAGS = dict(train_wildcard=1, train_wildcard_wildcard=1, train_h0=1, train_hT=1, train_V_embed=1, train_word_embed=1,
             train_beta=1, beta=0.7)
REFUSAL = ('training epochs are implemented for the i-FST models only (--independent 2: --method decompose, '
           'DESIGN.md row f3, and --method onehot, row f5); FARNN_S_D_W has no training step, run it with '
           '--epoch 0')


N_CASES = 13
PARAMS = d0r.FLOAT_KEYS + d0r.VGEN_KEYS
WORD_ROWS = ('V_embed', 'embedding.weight')


def _golden():
    with open(os.path.join(GOLDEN, 'decomp0_train_small.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, 'decomp0_train_small.npz'))


def case(k):
    """(configuration, restatement keywords, captured dict) of captured configuration k; the captured gradients of V_embed and
    embedding.weight are scattered back to all V rows (the rows of absent words are zero: the generator asserted it)"""
    meta, g = _golden()
    cfg = meta['configs'][k]
    pre = 'c{}.'.format(k)
    names = PARAMS + d0r.gate_keys(cfg['farnn']) + ((d0r.TRANS,) if cfg['use_crf'] else ())
    p = {n: g[pre + 'p.' + n].astype(np.float32) for n in names}
    trans = p.pop(d0r.TRANS, None)
    inp = dict(p=p, P=g[pre + 'priority'].astype(np.float32) if cfg['use_priority'] else None, x=g['x'], lengths=g['lengths'],
               labels=g['labels'], nl=cfg['update_nonlinear'], add_nl=cfg['additional_nonlinear'], farnn=cfg['farnn'], k=5.0,
               threshold=float(meta['threshold']), o_idx=int(meta['o_idx']), trans=trans)
    grads = {}
    for n in names:
        gr = g[pre + 'g.' + n]
        if n in WORD_ROWS:
            full = np.zeros(p[n].shape, np.float32)
            full[g[pre + 'words']] = gr
            gr = full
        grads[n] = gr
    return cfg, inp, dict(loss=float(g[pre + 'loss']), grads=grads, words=g[pre + 'words'], flat_pred=g[pre + 'flat_pred'])


def check_all_grads(name, got, g32, g64, present):
    """util.check_grad on every tensor of g64; the word-indexed ones by word slices"""
    for n in sorted(g64):
        word = n in WORD_ROWS + ('Vgen',)
        check_grad(name, n, np.asarray(got[n]).reshape(g64[n].shape), g32[n], g64[n], slices=0 if word else None,
                   present=present if word else None)


def test_the_captures_cover_the_configurations():
    cfgs = _golden()[0]['configs']
    assert len(cfgs) == N_CASES
    assert {(c['farnn'], c['use_crf'], c['use_priority']) for c in cfgs[:12]} == {(f, c, u) for f in (0, 1, 2) for c in (0, 1) for u in (0, 1)}
    assert {c['update_nonlinear'] for c in cfgs} == {'none', 'relu', 'tanh', 'relutanh'}
    assert {c['additional_nonlinear'] for c in cfgs} == {'none', 'tanh'}
    assert cfgs[12].get('additional_states') == 2
    assert all(c.get('rand_constant', 0) > 0 for c in cfgs if c['use_crf'])


@pytest.mark.parametrize('k', range(N_CASES))
def test_restatement_matches_the_reference_capture(k):
    """the float32 and float64 restatement against the float32 reference: the loss by assert_float_path, every gradient at
    util.check_grad's default bar, the predictions by equality"""
    cfg, inp, ref = case(k)
    d0r.check_gap(**{q: v for q, v in inp.items() if q not in ('labels', 'o_idx')})
    loss64, g64, pred = d0r.step(dtype=torch.float64, **inp)
    loss32, g32, pred32 = d0r.step(dtype=torch.float32, **inp)
    assert_float_path(ref['loss'], loss32, loss64, err_msg='loss')
    present = np.zeros(inp['p']['V_embed'].shape[0], bool)
    present[ref['words']] = True
    assert set(ref['grads']) == set(g64)
    for n in g64:
        assert np.abs(ref['grads'][n]).max() > 0, n
    check_all_grads('decomp0-ref-c{}'.format(k), ref['grads'], g32, g64, present)
    assert np.array_equal(pred, ref['flat_pred']) and np.array_equal(pred32, ref['flat_pred'])


def test_the_library_exports_the_decomp_fst_training_symbols():
    from re2nn_seq_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, 'include', 'farnn.h')) as f:
        hdr = f.read()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name
        assert name + '(' in hdr, name


def test_ctypes_layouts_of_the_decomp_fst_train_structs(tmp_path):
    from re2nn_seq_amd import _lib
    pairs = {'farnn_decomp_fst_train_dims': _lib.DecompFstTrainDims, 'farnn_decomp_fst_train_weights': _lib.DecompFstTrainWeights,
             'farnn_decomp_fst_train_outputs': _lib.DecompFstTrainOutputs}
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


def test_the_restatement_scores_equal_the_captured_tagging_scores():
    """the restatement's forward pass against the reference's scores captured for the tagging path (decomp_fst_small: farnn
    0 / 1 / 2, with and without the CRF rows and the priority layer; the max-semiring capture is not this step's)"""
    import json
    with open(os.path.join(GOLDEN, 'decomp_fst_small.json')) as f:
        meta = json.load(f)
    g = np.load(os.path.join(GOLDEN, 'decomp_fst_small.npz'))
    x, lengths = g['x'], g['lengths']
    seen = 0
    for k, cfg in enumerate(meta['configs']):
        if cfg.get('train_mode', 'sum') != 'sum':
            continue
        pre = 'c{}.'.format(k)
        p = {n: torch.from_numpy(g[pre + n].astype(np.float64)) for n in d0r.FLOAT_KEYS + ('V_embed', 'embed_r_generalized', 'beta_vec')
             + d0r.gate_keys(cfg['farnn'])}
        p['embedding.weight'] = torch.from_numpy(g[pre + 'embedding'].astype(np.float64))
        P = torch.from_numpy(g[pre + 'priority_mat'].astype(np.float64)) if cfg.get('use_priority') else None
        sc, valid, _, _ = d0r.forward(p, P, x, lengths, nl=cfg['update_nonlinear'], add_nl=cfg.get('additional_nonlinear', 'none'),
                                      farnn=cfg['farnn'], k=5.0)
        ref = g[pre + 'scores']
        np.testing.assert_allclose(sc.numpy()[valid.numpy()], ref[valid.numpy()], rtol=1e-4, atol=1e-4, err_msg=str(cfg))
        seen += 1
    assert seen >= 5


def _no_device(monkeypatch):
    from re2nn_seq_amd import _lib

    def boom(*a, **k):
        raise AssertionError('device work before the refusal')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(_lib, 'DecompFstTrainContext', boom)
    monkeypatch.setattr(_lib, 'TrainContext', boom)
    monkeypatch.setattr(_lib, 'load', boom)


def model(**kw):
    from re2nn_seq_amd.farnn.model_decompose import FARNN_S_D_W
    rng = np.random.RandomState(2)
    V, S, R, Q, K, D = 12, 7, 6, 4, 5, 3
    a = ns(independent=0, **dict(FLAGS, **kw))
    f = lambda *s: rng.rand(*s).astype(np.float32)      # noqa: E731
    return FARNN_S_D_W(V=f(V, R), C=f(K, R), S1=f(S, R), S2=f(S, R), C_wildcard=f(K, Q), S1_wildcard=f(S, Q), S2_wildcard=f(S, Q),
                       wildcard_wildcard=f(S, S), final_vector=f(S), start_vector=f(S), pretrained_word_embed=f(V, D),
                       priority_mat=None, args=a, o_idx=0)


def test_without_the_opt_in_the_model_is_refused_before_device_work(monkeypatch):
    from re2nn_seq_amd.train_onehot import check_trainable
    monkeypatch.delenv('RE2NN_DECOMP_FST_TRAIN', raising=False)
    m = model()
    _no_device(monkeypatch)
    x = torch.zeros((2, 3), dtype=torch.int64)
    for call in (m.enable_training, lambda: check_trainable(m), lambda: m.forward_local(x, x, torch.tensor([3, 2]), train=True)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == REFUSAL


@pytest.mark.parametrize('kw', [dict(), dict(farnn=1), dict(farnn=2), dict(use_crf=1), dict(use_priority=1),
                                dict(update_nonlinear='relutanh')])
def test_with_the_opt_in_the_covered_cases_pass_the_check(monkeypatch, kw):
    from re2nn_seq_amd import _lib
    monkeypatch.setenv('RE2NN_DECOMP_FST_TRAIN', '1')
    m = model(**kw)
    _no_device(monkeypatch)
    m._check_trainable()
    names = [k for k, grad in m._train_decl() if grad]
    want = {'S1', 'S2', 'embed_r_generalized', 'V_embed', 'C_embed', 'C_wildcard', 'S1_wildcard', 'S2_wildcard', 'wildcard_wildcard',
            'h0', 'hT', 'beta_vec', 'embedding.weight'} | set(d0r.gate_keys(kw.get('farnn', 0))) | ({d0r.TRANS} if kw.get('use_crf') else set())
    assert set(names) == want
    with pytest.raises(_lib.FarnnError, match='no MI355X visible'):
        m.enable_training()


def test_the_train_flags_follow_the_reference(monkeypatch):
    monkeypatch.setenv('RE2NN_DECOMP_FST_TRAIN', '1')
    m = model(train_wildcard=0, train_wildcard_wildcard=0, train_h0=0, train_V_embed=0)
    grads = dict(m._train_decl())
    assert not any(grads[k] for k in ('C_wildcard', 'S1_wildcard', 'S2_wildcard', 'wildcard_wildcard', 'h0', 'V_embed'))
    assert all(grads[k] for k in ('S1', 'S2', 'C_embed', 'embed_r_generalized', 'hT'))


@pytest.mark.parametrize('kw,match', [(dict(train_mode='max'), 'train_mode max'), (dict(marryup_type='kd'), 'marryup_type kd'),
                                      (dict(marryup_type='pr'), 'marryup_type pr'), (dict(local_loss_func='ML'), 'local_loss_func ML')])
def test_uncovered_configurations_are_refused_before_device_work(monkeypatch, kw, match):
    from re2nn_seq_amd.train_onehot import check_trainable
    monkeypatch.setenv('RE2NN_DECOMP_FST_TRAIN', '1')
    m = model(**kw)
    _no_device(monkeypatch)
    x = torch.zeros((2, 3), dtype=torch.int64)
    for call in (m.enable_training, lambda: check_trainable(m), lambda: m.forward_local(x, x, torch.tensor([3, 2]), train=True)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert match in str(e.value) and 'row f11' in str(e.value), str(e.value)


def test_two_ranks_are_refused_before_device_work(monkeypatch):
    from re2nn_seq_amd import dist
    monkeypatch.setenv('RE2NN_DECOMP_FST_TRAIN', '1')
    m = model()
    _no_device(monkeypatch)
    monkeypatch.setattr(dist, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='multi-GPU.*row f11'):
        m.enable_training()
