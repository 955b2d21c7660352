"""CPU checks of the gated decomposed independent=1 training step in the max semiring (FARNN_S_D_W_I, --farnn 1 | 2
--train_mode max): the exported symbol, the torch restatement (tests/decomp1_gated_max_train_ref.py) against
the loss / gradients / predictions captured from the reference, the planted faults the captures must see, and the refusals and
passes of RE2NN_DECOMP_IND1_GATED_MAX_TRAIN, all before any device work."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import decomp1_gated_max_train_ref as dgm
import decomp1_train_ref as dtr
from test_decomp1_gated_train_cpu import OLD_TEXT
from test_decomp1_train_cpu import FLAGS, WORD_ROWS, _no_device, check_all_grads
from util import GOLDEN, assert_float_path, load_golden, ns

N_CASES, N_CE = 24, 16
BASE_PARAMS = dtr.FLOAT_KEYS + dtr.VGEN_KEYS
SWITCHES = ('DECOMP_IND1_TRAIN', 'DECOMP_IND1_GATED_TRAIN', 'BUCKETED_MAX_TRAIN', 'DECOMP_IND1_CRF_TRAIN', 'DECOMP_IND1_GATED_MAX_TRAIN')
MAX_REFUSAL = OLD_TEXT.format('the max semiring (--train_mode max)')


def _golden():
    with open(os.path.join(GOLDEN, 'decomp1_train_gated_max_small.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, 'decomp1_train_gated_max_small.npz'))


def params_of(cfg):
    return BASE_PARAMS + dgm.gate_keys(cfg['farnn']) + ((dgm.TRANS,) if cfg.get('use_crf') else ())


def relu_gap_of(cfg):
    return 2e-5 if cfg['base'] == 'signed' else 0.0


def case(k):
    """(configuration, inputs of decomp1_gated_max_train_ref.step, captured dict) of captured configuration k, laid out as
    test_decomp1_gated_train_cpu.case lays the sum fixture out"""
    meta, g = _golden()
    cfgs = meta['configs']
    cfg = cfgs[k]
    pre = 'c{}.'.format(k)
    first = 'c{}.'.format(next(j for j, c in enumerate(cfgs) if c['base'] == cfg['base']))
    crf = bool(cfg.get('use_crf'))

    def param(n):
        return g[(pre if pre + 'p.' + n in g.files else first) + 'p.' + n].astype(np.float32)
    p = {n: param(n) for n in BASE_PARAMS + dgm.gate_keys(cfg['farnn'])}
    inp = dict(p=p, P=g[pre + 'priority'].astype(np.float32) if cfg['use_priority'] else None, x=g[cfg['base'] + '.x'],
               lengths=g[cfg['base'] + ('.lengths_crf' if crf else '.lengths')], labels=g[cfg['base'] + '.labels'],
               nl=cfg['update_nonlinear'], farnn=cfg['farnn'], k=float(cfg.get('sigmoid_exponent', 5)),
               threshold=float(meta['threshold']), o_idx=int(meta['o_idx']), trans=param(dgm.TRANS) if crf else None)
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


def test_the_library_exports_the_gated_max_step():
    from re2nn_seq_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    name = 'farnn_decomp_ind1_gated_max_train_step'
    assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES['farnn_decomp_ind1_gated_train_step']      # the same argument list
    assert callable(_lib.Decomp1TrainContext.gated_max_step)


def test_the_captures_cover_the_configurations():
    meta, g = _golden()
    cfgs = meta['configs']
    assert len(cfgs) == N_CASES and meta['train_mode'] == 'max'
    for farnn in (1, 2):
        ce = [c for c in cfgs[:N_CE] if c['farnn'] == farnn]
        assert len(ce) == 8 and not any(c.get('use_crf') for c in ce)
        assert {c['update_nonlinear'] for c in ce if c['base'] == 'signed'} == {'none', 'relu', 'tanh', 'relutanh'}
        assert sum(c['use_priority'] for c in ce) == 1
        crf = [c for c in cfgs[N_CE:] if c['farnn'] == farnn]
        assert all(c.get('use_crf') == 1 for c in crf)
        assert sorted((c['base'], c['use_priority']) for c in crf) == [(b, u) for b in ('decomp_ind1_small', 'signed') for u in (0, 1)]
    assert (g['signed.lengths'] == 0).any() and (g['signed.lengths_crf'] > 0).all()
    sum_fixture = load_golden('decomp1_train_gated_small')             # the gated fixture's base shapes
    for n in ('S1', 'V_embed', 'C_output', 'S1_output'):
        assert g['c0.p.' + n].shape == sum_fixture['c0.p.' + n].shape, n
    assert g['signed.x'].shape == sum_fixture['signed.x'].shape


def test_one_state_is_an_exact_copy_of_another_in_every_tensor():
    """the planted twin: the factors, the initial vectors, wildcard_mat and the gates' columns"""
    i, j = _golden()[0]['twin']
    for k in (0, 8, 5, 13):
        p = case(k)[1]['p']
        for n in ('S1', 'S2', 'S1_output', 'S2_output'):
            assert np.array_equal(p[n][i], p[n][j]), n
        for n in ('h0', 'hT'):
            assert p[n][i] == p[n][j], n
        if not case(k)[0].get('additional_states'):           # (the padded rows and columns of wildcard_mat are random)
            assert np.array_equal(p['wildcard_mat'][i], p['wildcard_mat'][j]) and np.array_equal(p['wildcard_mat'][:, i], p['wildcard_mat'][:, j])
        for n in dgm.gate_keys(case(k)[0]['farnn']):
            assert np.array_equal(p[n][:, i], p[n][:, j]), n


@pytest.mark.parametrize('k', range(N_CASES))
def test_restatement_matches_the_reference_capture(k):
    """the float32 and float64 restatement against the float32 reference, at the bars of tests/util.py"""
    cfg, inp, ref = case(k)
    dgm.check_gap(min_gap=2e-5, relu_gap=relu_gap_of(cfg), **{q: v for q, v in inp.items() if q != 'labels'})
    loss64, g64, pred = dgm.step(dtype=torch.float64, **inp)
    loss32, g32, pred32 = dgm.step(dtype=torch.float32, **inp)
    assert_float_path(ref['loss'], loss32, loss64, err_msg='loss')
    assert set(ref['grads']) == set(params_of(cfg)) == set(g64)
    for n in ref['grads']:
        assert np.abs(ref['grads'][n]).max() > 0, n
    check_all_grads('decomp1-gated-max-ref-c{}'.format(k), ref['grads'], g32, g64, present_of(inp, ref))
    assert np.array_equal(pred, ref['flat_pred']) and np.array_equal(pred32, ref['flat_pred'])


@pytest.mark.parametrize('fault', dgm.FAULTS)
def test_a_planted_fault_breaks_a_capture_it_applies_to(fault):
    """each wrong statement of the restatement misses the captured gradients on at least one configuration it applies to"""
    seen = 0
    for k in range(N_CE):
        cfg, inp, ref = case(k)
        if fault in dgm.FARNN2_ONLY and cfg['farnn'] != 2:
            continue
        g32, g64 = (dgm.step(dtype=dt, fault=fault, **inp)[1] for dt in (torch.float32, torch.float64))
        try:
            check_all_grads('planted {} c{}'.format(fault, k), ref['grads'], g32, g64, present_of(inp, ref))
        except AssertionError:
            seen += 1
    assert seen > 0, fault


def test_sum_chains_are_far_above_the_bar_on_every_configuration():
    """the generator's second condition: with sum chains a stored gradient moves by more than ten gradient bars"""
    for k in range(N_CASES):
        cfg, inp, _ = case(k)
        g = dgm.step(dtype=torch.float64, **inp)[1]
        gs = dgm.step(dtype=torch.float64, fault='sum', **inp)[1]
        assert any(np.abs(gs[n] - g[n]).max() > 10 * 1e-4 * np.abs(g[n]).max() for n in g), k


def build(k, **kw):
    """the mirror of captured configuration k, built from the captured (already padded) parameters and loaded with them,
    --train_mode max and every train_* flag on unless kw says otherwise"""
    from re2nn_seq_amd.farnn.model_decompose_independent import FARNN_S_D_W_I
    meta, g = _golden()
    cfg, inp, _ = case(k)
    args = dict(FLAGS, **dict({q: v for q, v in cfg.items() if q != 'base'}, **dict(dict(train_mode='max'), **kw)))
    a = ns(independent=1, threshold=inp['threshold'], bias_init=float(meta['bias_init']), **args)
    p = inp['p']
    a.additional_states, a.rand_constant = 0, 0.0
    S = p['S1'].shape[0]
    C_o = p['C_output'][:-2] if a.use_crf else p['C_output']
    m = FARNN_S_D_W_I(V=p['V_embed'], S1=p['S1'], S2=p['S2'], C_output=C_o, S1_output=p['S1_output'],
                      S2_output=p['S2_output'], wildcard_mat=p['wildcard_mat'], wildcard_output=np.zeros((S, S), np.float32),
                      final_vector=p['hT'], start_vector=p['h0'], pretrained_word_embed=p['embedding.weight'],
                      priority_mat=load_golden('decomp_ind1_small')['priority_in'], args=a, o_idx=inp['o_idx'])
    sd = {n: torch.from_numpy(v) for n, v in p.items()}
    if inp['trans'] is not None:
        sd[dgm.TRANS] = torch.from_numpy(inp['trans'])
    m.load_state_dict(sd)
    if inp['P'] is not None:
        m.priority_full = inp['P']
    return m


def _calls(m):
    from re2nn_seq_amd.train_onehot import check_trainable
    x = torch.zeros((2, 3), dtype=torch.int64)
    return (m.enable_training, lambda: check_trainable(m), lambda: m.forward_local(x, x, torch.tensor([3, 2]), train=True))


def _set(monkeypatch, *names):
    for n in SWITCHES:
        monkeypatch.delenv('RE2NN_' + n, raising=False)
    for n in names:
        monkeypatch.setenv('RE2NN_' + n, '1')


@pytest.mark.parametrize('k', [0, 8, 16, 22])
def test_with_the_switch_a_gated_max_model_passes_the_check_and_asks_for_the_gpu(monkeypatch, k):
    from re2nn_seq_amd import _lib
    from re2nn_seq_amd.train_onehot import check_trainable
    _set(monkeypatch, *SWITCHES)
    m = build(k)
    assert m.args.train_mode == 'max' and m._semiring() == 'max'
    _no_device(monkeypatch)
    check_trainable(m)
    with pytest.raises(_lib.FarnnError, match='no MI355X visible'):
        m.enable_training()


@pytest.mark.parametrize('k', [0, 8, 16])
def test_without_the_new_switch_a_gated_max_model_gets_todays_refusal(monkeypatch, k):
    _set(monkeypatch, *[n for n in SWITCHES if n != 'DECOMP_IND1_GATED_MAX_TRAIN'])
    m = build(k)
    _no_device(monkeypatch)
    for call in _calls(m):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == MAX_REFUSAL


@pytest.mark.parametrize('missing,why', [('DECOMP_IND1_GATED_TRAIN', 'the gated recurrences (--farnn 2)'),
                                         ('BUCKETED_MAX_TRAIN', 'the max semiring (--train_mode max)'),
                                         ('DECOMP_IND1_CRF_TRAIN', 'the CRF (--use_crf 1)')])
def test_the_new_switch_counts_only_beside_the_others(monkeypatch, missing, why):
    _set(monkeypatch, *[n for n in SWITCHES if n != missing])
    m = build(22)                          # farnn 2 with the CRF
    _no_device(monkeypatch)
    for call in _calls(m):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == OLD_TEXT.format(why)


def test_the_new_switch_alone_opens_nothing(monkeypatch):
    from test_decomp1_train_cpu import REFUSAL
    _set(monkeypatch, 'DECOMP_IND1_GATED_MAX_TRAIN')
    m = build(8)
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError) as e:
        m.enable_training()
    assert str(e.value) == REFUSAL


def test_the_new_switch_opens_no_other_train_mode(monkeypatch):
    _set(monkeypatch, *SWITCHES)
    m = build(8, train_mode='hybrid')
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError) as e:
        m.enable_training()
    assert str(e.value) == OLD_TEXT.format('the max semiring (--train_mode hybrid)')
