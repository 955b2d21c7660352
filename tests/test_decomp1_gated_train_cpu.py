"""CPU checks of the gated decomposed independent=1 training step (FARNN_S_D_W_I, --farnn 1 | 2): the
exported symbol and the C-ABI struct layouts, the torch restatement (tests/decomp1_gated_train_ref.py) against the loss /
gradients / predictions captured from the reference, the planted faults the captures must see, the mirror's state dict, and
the refusals and passes of RE2NN_DECOMP_IND1_GATED_TRAIN, all before any device work."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import decomp1_gated_train_ref as dgr
import decomp1_train_ref as dtr
from test_decomp1_train_cpu import FLAGS, WORD_ROWS, _no_device, check_all_grads
from util import GOLDEN, assert_float_path, load_golden, ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CASES, N_CE = 24, 16
BASE_PARAMS = dtr.FLOAT_KEYS + dtr.VGEN_KEYS
OLD_TEXT = ('training the decomposed independent=1 model covers farnn 0, the sum semiring and the CE1 loss on one GPU; {} is not '
            'built (DESIGN.md, row f9)')


def _golden():
    with open(os.path.join(GOLDEN, 'decomp1_train_gated_small.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, 'decomp1_train_gated_small.npz'))


def params_of(cfg):
    return BASE_PARAMS + dgr.gate_keys(cfg['farnn']) + ((dgr.TRANS,) if cfg.get('use_crf') else ())


def case(k):
    """(configuration, inputs of decomp1_gated_train_ref.step, captured dict) of captured configuration k.  A parameter the
    generator stored with the first configuration of the same base only is read from there; the captured gradients of V_embed
    and embedding.weight are scattered back to all V rows."""
    meta, g = _golden()
    cfgs = meta['configs']
    cfg = cfgs[k]
    pre = 'c{}.'.format(k)
    first = 'c{}.'.format(next(j for j, c in enumerate(cfgs) if c['base'] == cfg['base']))
    crf = bool(cfg.get('use_crf'))

    def param(n):
        return g[(pre if pre + 'p.' + n in g.files else first) + 'p.' + n].astype(np.float32)
    p = {n: param(n) for n in BASE_PARAMS + dgr.gate_keys(cfg['farnn'])}
    inp = dict(p=p, P=g[pre + 'priority'].astype(np.float32) if cfg['use_priority'] else None, x=g[cfg['base'] + '.x'],
               lengths=g[cfg['base'] + ('.lengths_crf' if crf else '.lengths')], labels=g[cfg['base'] + '.labels'],
               nl=cfg['update_nonlinear'], farnn=cfg['farnn'], k=float(cfg.get('sigmoid_exponent', 5)),
               threshold=float(meta['threshold']), o_idx=int(meta['o_idx']), trans=param(dgr.TRANS) if crf else None)
    grads = {}
    for n in params_of(cfg):
        gr = g[pre + 'g.' + n]
        if n in WORD_ROWS:
            full = np.zeros(p[n].shape, np.float32)
            full[g[pre + 'words']] = gr
            gr = full
        grads[n] = gr
    return cfg, inp, dict(loss=float(g[pre + 'loss']), grads=grads, words=g[pre + 'words'], flat_pred=g[pre + 'flat_pred'])


def present_of(inp, ref):
    present = np.zeros(inp['p']['V_embed'].shape[0], bool)
    present[ref['words']] = True
    return present


def test_the_library_exports_the_gated_step_and_the_binding_mirrors_its_structs(tmp_path):
    from re2nn_seq_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert 'farnn_decomp_ind1_gated_train_step' in _lib.SIGNATURES and lib.farnn_decomp_ind1_gated_train_step is not None
    pairs = {'farnn_decomp_ind1_gate_weights': _lib.Decomp1GateWeights, 'farnn_decomp_ind1_gate_outputs': _lib.Decomp1GateOutputs}
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
    assert len(cfgs) == N_CASES
    for farnn in (1, 2):
        ce = [c for c in cfgs[:N_CE] if c['farnn'] == farnn]
        assert len(ce) == 8 and not any(c.get('use_crf') for c in ce)
        assert {c['update_nonlinear'] for c in ce if c['base'] == 'signed'} == {'none', 'relu', 'tanh', 'relutanh'}
        for key, val in (('use_priority', 1), ('additional_states', 2), ('xavier', 1), ('sigmoid_exponent', 1)):
            assert sum(c.get(key, 0) == val for c in ce) == 1, key
        crf = [c for c in cfgs[N_CE:] if c['farnn'] == farnn]
        assert all(c.get('use_crf') == 1 for c in crf)
        assert sorted((c['base'], c['use_priority']) for c in crf) == [(b, u) for b in ('decomp_ind1_small', 'signed') for u in (0, 1)]
    g = _golden()[1]
    assert (g['signed.lengths'] == 0).any() and (g['signed.lengths_crf'] > 0).all()


@pytest.mark.parametrize('k', range(N_CASES))
def test_restatement_matches_the_reference_capture(k):
    """the float32 and float64 restatement against the float32 reference, at the bars of tests/util.py"""
    cfg, inp, ref = case(k)
    dgr.check_gap(min_gap=2e-5 if cfg['base'] == 'signed' else 0.0, **{q: v for q, v in inp.items() if q != 'labels'})
    loss64, g64, pred = dgr.step(dtype=torch.float64, **inp)
    loss32, g32, pred32 = dgr.step(dtype=torch.float32, **inp)
    assert_float_path(ref['loss'], loss32, loss64, err_msg='loss')
    assert set(ref['grads']) == set(params_of(cfg)) == set(g64)
    for n in ref['grads']:
        assert np.abs(ref['grads'][n]).max() > 0, n
    check_all_grads('decomp1-gated-ref-c{}'.format(k), ref['grads'], g32, g64, present_of(inp, ref))
    assert np.array_equal(pred, ref['flat_pred']) and np.array_equal(pred32, ref['flat_pred'])
    assert inp['p']['bs1'].shape == (1, inp['p']['S1'].shape[0])


@pytest.mark.parametrize('fault', dgr.FAULTS)
def test_a_planted_fault_breaks_a_capture_it_applies_to(fault):
    """each wrong statement of the restatement misses the captured gradients on at least one configuration it applies to"""
    seen = 0
    for k in range(N_CE):
        cfg, inp, ref = case(k)
        if fault in dgr.FARNN2_ONLY and cfg['farnn'] != 2:
            continue
        g32, g64 = (dgr.step(dtype=dt, fault=fault, **inp)[1] for dt in (torch.float32, torch.float64))
        try:
            check_all_grads('planted {} c{}'.format(fault, k), ref['grads'], g32, g64, present_of(inp, ref))
        except AssertionError:
            seen += 1
    assert seen > 0, fault


def test_the_one_minus_r_share_of_dh0_is_far_above_the_bar():
    """every farnn 2 capture: dh0 without the (1 - r) term is more than ten gradient bars away (the generator asserted it)"""
    for k in range(N_CASES):
        cfg, inp, _ = case(k)
        if cfg['farnn'] != 2:
            continue
        full = dgr.step(dtype=torch.float64, **inp)[1]['h0']
        cut = dgr.step(dtype=torch.float64, fault='no_init_share', **inp)[1]['h0']
        assert np.abs(full - cut).max() > 10 * 1e-4 * np.abs(full).max(), k


def build(k, from_capture=True, **kw):
    """the mirror of captured configuration k.  from_capture: built from the captured (already padded) parameters and loaded
    with them, every train_* flag on unless kw says otherwise; else built as the generator built the reference -- the base's
    unpadded inputs, the configuration's own arguments, the generator's seed."""
    from re2nn_seq_amd.farnn.model_decompose_independent import FARNN_S_D_W_I
    meta, g = _golden()
    cfg, inp, _ = case(k)
    args = dict(FLAGS, **dict({q: v for q, v in cfg.items() if q != 'base'}, **kw))
    a = ns(independent=1, threshold=inp['threshold'], bias_init=float(meta['bias_init']), **args)
    if from_capture:
        p = inp['p']
        a.additional_states, a.rand_constant = 0, 0.0
    else:
        plain = next(j for j, c in enumerate(meta['configs'])
                     if c['base'] == cfg['base'] and not c.get('additional_states') and not c.get('use_crf'))
        p = case(plain)[1]['p']
        torch.manual_seed(900 + k)
    S = p['S1'].shape[0]
    C_o = p['C_output'][:-2] if from_capture and a.use_crf else p['C_output']
    m = FARNN_S_D_W_I(V=p['V_embed'], S1=p['S1'], S2=p['S2'], C_output=C_o, S1_output=p['S1_output'],
                      S2_output=p['S2_output'], wildcard_mat=p['wildcard_mat'], wildcard_output=np.zeros((S, S), np.float32),
                      final_vector=p['hT'], start_vector=p['h0'], pretrained_word_embed=p['embedding.weight'],
                      priority_mat=load_golden('decomp_ind1_small')['priority_in'], args=a, o_idx=inp['o_idx'])
    if from_capture:
        sd = {n: torch.from_numpy(v) for n, v in p.items()}
        if inp['trans'] is not None:
            sd[dgr.TRANS] = torch.from_numpy(inp['trans'])
        m.load_state_dict(sd)
        if inp['P'] is not None:
            m.priority_full = inp['P']
    return m


@pytest.mark.parametrize('k', [0, 5, 6, 8, 13, 14, 16, 22])
def test_the_mirror_builds_the_state_dict_the_reference_built(k):
    """same seed, same arguments: the gates (xavier on bs1 under farnn 1 included), the padded states and the START / STOP rows
    come out as the reference drew them, bit for bit"""
    cfg, inp, _ = case(k)
    sd = build(k, from_capture=False).state_dict()
    for n in BASE_PARAMS + dgr.gate_keys(cfg['farnn']):
        assert tuple(sd[n].shape) == inp['p'][n].shape, n
        if n == 'embed_r_generalized':       # a pseudo-inverse: LAPACK's rounding, not a draw, and not the same on every host
            np.testing.assert_allclose(sd[n].numpy(), inp['p'][n], rtol=1e-4, atol=1e-6)
            continue
        assert np.array_equal(sd[n].numpy(), inp['p'][n]), n
    assert ('Wss2' in sd) == (cfg['farnn'] == 2) and tuple(sd['bs1'].shape) == (1, inp['p']['S1'].shape[0])
    assert (dgr.TRANS in sd) == bool(cfg.get('use_crf'))


def _calls(m):
    from re2nn_seq_amd.train_onehot import check_trainable
    x = torch.zeros((2, 3), dtype=torch.int64)
    return (m.enable_training, lambda: check_trainable(m), lambda: m.forward_local(x, x, torch.tensor([3, 2]), train=True))


@pytest.mark.parametrize('k', [0, 8])
def test_without_the_new_switch_a_gated_model_gets_todays_refusal(monkeypatch, k):
    monkeypatch.setenv('RE2NN_DECOMP_IND1_TRAIN', '1')
    monkeypatch.delenv('RE2NN_DECOMP_IND1_GATED_TRAIN', raising=False)
    m = build(k)
    _no_device(monkeypatch)
    for call in _calls(m):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == OLD_TEXT.format('the gated recurrences (--farnn {})'.format(m.args.farnn))


@pytest.mark.parametrize('k', [0, 8, 16, 22])
def test_with_the_switch_a_gated_model_passes_the_check_and_asks_for_the_gpu(monkeypatch, k):
    from re2nn_seq_amd import _lib
    from re2nn_seq_amd.train_onehot import check_trainable
    for name in ('DECOMP_IND1_TRAIN', 'DECOMP_IND1_GATED_TRAIN', 'DECOMP_IND1_CRF_TRAIN'):
        monkeypatch.setenv('RE2NN_' + name, '1')
    m = build(k)
    _no_device(monkeypatch)
    check_trainable(m)
    with pytest.raises(_lib.FarnnError, match='no MI355X visible'):
        m.enable_training()
    assert [n for n, _ in m._train_decl()][-3 * m.args.farnn - bool(m.use_crf):] == \
        list(dgr.gate_keys(m.args.farnn)) + ([dgr.TRANS] if m.use_crf else [])


@pytest.mark.parametrize('kw,why', [(dict(train_mode='max'), 'the max semiring (--train_mode max)'),
                                    (dict(marryup_type='kd'), 'the KD / PR teacher terms (--marryup_type kd)'),
                                    (dict(marryup_type='pr'), 'the KD / PR teacher terms (--marryup_type pr)'),
                                    (dict(farnn=3), 'the gated recurrences (--farnn 3)'),
                                    (dict(use_crf=1), 'the CRF (--use_crf 1)')])
def test_with_the_switch_the_uncovered_configurations_stay_refused(monkeypatch, kw, why):
    """--train_mode max on a gated model also with the bucketed max switch set; the CRF without its own switch"""
    monkeypatch.setenv('RE2NN_DECOMP_IND1_TRAIN', '1')
    monkeypatch.setenv('RE2NN_DECOMP_IND1_GATED_TRAIN', '1')
    monkeypatch.setenv('RE2NN_BUCKETED_MAX_TRAIN', '1')
    monkeypatch.delenv('RE2NN_DECOMP_IND1_CRF_TRAIN', raising=False)
    m = build(16 if 'use_crf' in kw else 8, **kw)
    if 'farnn' in kw:
        m.args.farnn = kw['farnn']
    _no_device(monkeypatch)
    for call in _calls(m):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == OLD_TEXT.format(why)


def test_the_new_switch_alone_opens_nothing(monkeypatch):
    from test_decomp1_train_cpu import REFUSAL
    monkeypatch.delenv('RE2NN_DECOMP_IND1_TRAIN', raising=False)
    monkeypatch.setenv('RE2NN_DECOMP_IND1_GATED_TRAIN', '1')
    m = build(8)
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError) as e:
        m.enable_training()
    assert str(e.value) == REFUSAL
