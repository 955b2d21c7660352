"""CPU checks of the decomposed independent=1 training step under the CRF (FARNN_S_D_W_I, --use_crf 1): the
torch restatement (tests/decomp1_crf_train_ref.py) against the loss / gradients / predictions captured from the reference, the
planted faults every capture they apply to must see, and the refusals that must come before any device work."""
import json
import os

import numpy as np
import pytest
import torch

import decomp1_crf_train_ref as dcr
import decomp1_train_ref as dtr
from test_decomp1_train_cpu import FLAGS, REFUSAL, WORD_ROWS, _no_device, check_all_grads
from util import GOLDEN, assert_float_path, ns

N_CASES = 16
PARAMS = dtr.FLOAT_KEYS + dtr.VGEN_KEYS
NAMED = PARAMS + (dcr.TRANS,)
CRF_REFUSAL = ('training the decomposed independent=1 model covers farnn 0, the sum semiring and the CE1 loss on one GPU; '
               'the CRF (--use_crf 1) is not built (DESIGN.md, row f9)')
SYMBOL = 'farnn_decomp_ind1_crf_train_step'


def _golden():
    with open(os.path.join(GOLDEN, 'decomp1_train_crf_small.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, 'decomp1_train_crf_small.npz'))


def case(k):
    """(configuration, inputs of decomp1_crf_train_ref.step, captured dict) of captured configuration k; the captured
    gradients of V_embed and embedding.weight are scattered back to all V rows"""
    meta, g = _golden()
    cfg = meta['configs'][k]
    pre = 'c{}.'.format(k)
    p = {n: g[pre + 'p.' + n].astype(np.float32) for n in PARAMS}
    inp = dict(p=p, P=g[pre + 'priority'].astype(np.float32) if cfg['use_priority'] else None,
               trans=g[pre + 'p.' + dcr.TRANS].astype(np.float32), x=g[cfg['base'] + '.x'], lengths=g[cfg['base'] + '.lengths'],
               labels=g[cfg['base'] + '.labels'], nl=cfg['update_nonlinear'], threshold=float(meta['threshold']),
               o_idx=int(meta['o_idx']), semiring=cfg['train_mode'])
    grads = {}
    for n in NAMED:
        gr = g[pre + 'g.' + n]
        if n in WORD_ROWS:
            full = np.zeros(p[n].shape, np.float32)
            full[g[pre + 'words']] = gr
            gr = full
        grads[n] = gr
    return cfg, inp, dict(loss=float(g[pre + 'loss']), grads=grads, words=g[pre + 'words'], flat_pred=g[pre + 'flat_pred'])


def _present(inp, ref):
    present = np.zeros(inp['p']['V_embed'].shape[0], bool)
    present[ref['words']] = True
    return present


def compare(name, inp, ref, fault=None):
    """the float32 and float64 restatement against the capture, at the bars of tests/util.py"""
    loss64, g64, pred = dcr.step(dtype=torch.float64, fault=fault, **inp)
    loss32, g32, pred32 = dcr.step(dtype=torch.float32, fault=fault, **inp)
    assert_float_path(ref['loss'], loss32, loss64, err_msg='loss')
    assert set(ref['grads']) == set(NAMED)
    check_all_grads(name, ref['grads'], g32, g64, _present(inp, ref))
    assert np.array_equal(pred, ref['flat_pred']) and np.array_equal(pred32, ref['flat_pred'])


def test_the_captures_cover_the_configurations():
    meta, g = _golden()
    cfgs = meta['configs']
    assert len(cfgs) == N_CASES
    signed = {(c['update_nonlinear'], c['use_priority'], c['train_mode']) for c in cfgs if c['base'] == 'signed'}
    assert signed == {(nl, up, tm) for nl in ('none', 'relu', 'tanh') for up in (0, 1) for tm in ('sum', 'max')}
    assert sum(c['base'] == 'decomp_ind1_small' for c in cfgs) == 4
    for b in ('signed', 'decomp_ind1_small'):
        assert g[b + '.lengths'].min() >= 1, 'the reference cannot run an empty sequence through the CRF'
    for k in range(N_CASES):
        tr, C = g['c{}.p.{}'.format(k, dcr.TRANS)], g['c{}.p.C_output'.format(k)].shape[0]
        assert tr.shape == (C, C) and np.abs(g['c{}.p.C_output'.format(k)][-2:]).min() > 0
        assert (tr[:, C - 2] == -10000.0).all() and (tr[C - 1, :] == -10000.0).all()


@pytest.mark.parametrize('k', range(N_CASES))
def test_restatement_matches_the_reference_capture(k):
    cfg, inp, ref = case(k)
    dcr.check_gap(min_gap=2e-5 if cfg['base'] == 'signed' else 0.0, **{q: v for q, v in inp.items() if q != 'labels'})
    for n in NAMED:
        assert np.abs(ref['grads'][n]).max() > 0, n
    compare('decomp1-crf-ref-c{}'.format(k), inp, ref)


def _clamp_decides(inp):
    """the clamp of column C-3 changes the float64 restatement's decode on these inputs"""
    with torch.no_grad():
        pt = dtr._params(inp['p'], torch.float64)
        Pt = None if inp['P'] is None else dtr._t(inp['P'], torch.float64)
        x, lens = dtr._ints(inp['x']), dtr._ints(inp['lengths'])
        em = dcr.emissions(pt, Pt, x, lens, inp['nl'], 'none', inp['semiring']).numpy()
    tr = inp['trans'].astype(np.float64)
    return not np.array_equal(dcr.viterbi(em, tr, lens.numpy(), inp['threshold'], inp['o_idx']),
                              dcr.viterbi(em, tr, lens.numpy(), np.inf, inp['o_idx']))


@pytest.mark.parametrize('fault', ['mean', 'no_stop', 'clamp_last', 'no_gold_counts'])
def test_a_planted_fault_fails_every_capture_it_applies_to(fault):
    """mean instead of sum; the STOP transition dropped from the gold score; the clamp on column C-1 instead of C-3 (the
    captures whose decode the clamp decides); the transitions' gradient without the gold counts"""
    applies = 0
    for k in range(N_CASES):
        _, inp, ref = case(k)
        if fault == 'clamp_last' and not _clamp_decides(inp):
            continue
        applies += 1
        with pytest.raises(AssertionError):
            compare('c{} with {}'.format(k, fault), inp, ref, fault=fault)
    assert applies >= (1 if fault == 'clamp_last' else N_CASES)


def test_the_last_index_on_a_planted_exact_viterbi_tie_is_seen():
    """two predecessors offer position 1 exactly the same score: torch.max takes the first, and the paths differ"""
    C = 6                                       # labels 0..3 (3 = C-3 is the clamped one, untouched here), START, STOP
    tr = dcr.default_transitions(C).astype(np.float64)
    em = np.zeros((1, 2, C))
    em[0, 0, :3] = [1.0, 1.0, 0.25]             # labels 0 and 1 tie at position 0 ...
    em[0, 1, :3] = [0.0, 0.5, 2.0]              # ... and nothing at position 1 tells them apart
    lens = np.array([2])
    first = dcr.viterbi(em, tr, lens, 9.0, 0)
    last = dcr.viterbi(em, tr, lens, 9.0, 0, fault='last_tie')
    assert first.tolist() == [0, 2] and last.tolist() == [1, 2]
    with pytest.raises(dcr.GapError):
        dcr.viterbi(em, tr, lens, 9.0, 0, check=True)


def test_an_empty_sequence_contributes_nothing_to_the_restatement():
    _, inp, _ = case(0)
    lengths = inp['lengths'].copy()
    keep = np.flatnonzero(lengths > 0)[1:]
    a = dcr.step(dtype=torch.float64, **dict(inp, x=inp['x'][keep], lengths=lengths[keep], labels=inp['labels'][keep]))
    lengths[np.flatnonzero(lengths > 0)[0]] = 0
    b = dcr.step(dtype=torch.float64, **dict(inp, lengths=lengths))
    assert a[0] == pytest.approx(b[0], rel=1e-12) and np.array_equal(a[2], b[2])
    for n in NAMED:
        np.testing.assert_allclose(a[1][n], b[1][n], rtol=1e-9, atol=1e-12, err_msg=n)


def test_the_library_exports_the_crf_step():
    import ctypes
    from re2nn_seq_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(os.path.dirname(GOLDEN), '..', 'include', 'farnn.h')) as f:
        assert SYMBOL + '(' in f.read()
    assert SYMBOL in _lib.SIGNATURES and getattr(lib, SYMBOL) is not None
    assert hasattr(_lib.Decomp1TrainContext, 'step_crf')


def model(k=0, **kw):
    """the mirror built from captured configuration k's parameters, use_crf = 1 (every train_* flag on unless kw says otherwise)"""
    from re2nn_seq_amd.farnn.model_decompose_independent import FARNN_S_D_W_I
    cfg, inp, _ = case(k)
    p = inp['p']
    fields = dict(FLAGS, use_crf=1)
    fields.update({q: v for q, v in cfg.items() if q != 'base'})
    fields.update(kw)
    a = ns(independent=1, threshold=inp['threshold'], **fields)
    a.additional_states, a.rand_constant = 0, 0.0
    S = p['S1'].shape[0]
    use_crf = bool(a.use_crf)
    Cout = p['C_output'][:-2] if use_crf else p['C_output']    # the constructor appends the START / STOP rows itself
    m = FARNN_S_D_W_I(V=p['V_embed'], S1=p['S1'], S2=p['S2'], C_output=Cout, S1_output=p['S1_output'],
                      S2_output=p['S2_output'], wildcard_mat=p['wildcard_mat'], wildcard_output=np.zeros((S, S), np.float32),
                      final_vector=p['hT'], start_vector=p['h0'], pretrained_word_embed=p['embedding.weight'],
                      priority_mat=None, args=a, o_idx=inp['o_idx'])
    sd = {n: torch.from_numpy(Cout if n == 'C_output' else p[n]) for n in PARAMS}
    if use_crf:
        sd['C_output'] = torch.from_numpy(p['C_output'])
        sd[dcr.TRANS] = torch.from_numpy(inp['trans'])
    m.load_state_dict(sd)
    if inp['P'] is not None:
        m.priority_full = inp['P'] if use_crf else inp['P'][:-2, :-2]
    return m


def _calls(m):
    from re2nn_seq_amd.train_onehot import check_trainable
    x = torch.zeros((2, 3), dtype=torch.int64)
    return (m.enable_training, lambda: check_trainable(m), lambda: m.forward_local(x, x, torch.tensor([3, 2]), train=True))


def test_without_the_crf_switch_use_crf_is_refused_with_the_old_text(monkeypatch):
    monkeypatch.setenv('RE2NN_DECOMP_IND1_TRAIN', '1')
    monkeypatch.delenv('RE2NN_DECOMP_IND1_CRF_TRAIN', raising=False)
    m = model()
    _no_device(monkeypatch)
    for call in _calls(m):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == CRF_REFUSAL
    monkeypatch.delenv('RE2NN_DECOMP_IND1_TRAIN')
    monkeypatch.setenv('RE2NN_DECOMP_IND1_CRF_TRAIN', '1')      # the CRF switch alone opens nothing
    for call in _calls(m):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == REFUSAL


def test_with_both_switches_and_no_device_enable_training_reports_the_missing_gpu(monkeypatch):
    from re2nn_seq_amd import _lib
    monkeypatch.setenv('RE2NN_DECOMP_IND1_TRAIN', '1')
    monkeypatch.setenv('RE2NN_DECOMP_IND1_CRF_TRAIN', '1')
    m = model()
    _no_device(monkeypatch)
    with pytest.raises(_lib.FarnnError, match='no MI355X visible'):
        m.enable_training()


@pytest.mark.parametrize('kw,match', [(dict(farnn=1), 'farnn 1'), (dict(marryup_type='kd'), 'marryup_type kd'),
                                      (dict(local_loss_func='CE'), 'local_loss_func CE')])
def test_with_the_crf_switch_the_uncovered_configurations_stay_refused(monkeypatch, kw, match):
    monkeypatch.setenv('RE2NN_DECOMP_IND1_TRAIN', '1')
    monkeypatch.setenv('RE2NN_DECOMP_IND1_CRF_TRAIN', '1')
    m = model(**kw)
    _no_device(monkeypatch)
    for call in _calls(m):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert match in str(e.value) and 'row f9' in str(e.value), str(e.value)


def test_with_the_crf_switch_two_ranks_stay_refused(monkeypatch):
    from re2nn_seq_amd import dist
    monkeypatch.setenv('RE2NN_DECOMP_IND1_TRAIN', '1')
    monkeypatch.setenv('RE2NN_DECOMP_IND1_CRF_TRAIN', '1')
    m = model()
    _no_device(monkeypatch)
    monkeypatch.setattr(dist, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='multi-GPU.*row f9'):
        m.enable_training()


@pytest.mark.parametrize('use_crf', [0, 1])
def test_the_state_dict_holds_crf_transitions_exactly_when_use_crf(use_crf):
    """(named_parameters() needs the device: tests/test_gpu_decomp1_crf_train.py asks the same of it)"""
    m = model(use_crf=use_crf)
    assert (dcr.TRANS in m.state_dict()) == bool(use_crf)
    if use_crf:
        assert np.array_equal(m.state_dict()[dcr.TRANS].numpy(), case(0)[1]['trans'])
