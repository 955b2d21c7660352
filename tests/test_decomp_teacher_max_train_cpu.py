"""The KD / PR teacher step of the decomposed i-FST in the MAX semiring without a GPU: the restatement
(tests/decomp_teacher_max_train_ref.py) reproduces the reference's captures, the fixture's conditions hold on the stored data,
every planted fault is seen, and the model mirror's switch and refusals come before any device work.

Bars: the loss within 2e-5 max(1, |ref|), every gradient at the close() bar of tests/test_gpu_train_max.py, the flat
predictions equal -- the bars tests/test_gpu_decomp_teacher_max_train.py applies to the library."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import decomp_teacher_max_train_ref as dxr  # noqa: E402
import decomp_teacher_train_ref as dtr  # noqa: E402
from util import GOLDEN, ns  # noqa: E402

PARAMS = ('S1', 'S2', 'V_embed', 'embed_r_generalized', 'C_output_mat', 'wildcard_mat', 'h0', 'hT', 'beta_vec',
          'embedding.weight')
GATES = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')
N_CONFIGS = 12


def load():
    with open(os.path.join(GOLDEN, 'decomp_train_teacher_max_small.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, 'decomp_train_teacher_max_small.npz')), np.load(os.path.join(GOLDEN, 'decomp_small.npz'))


META, G, BASE = load()


def bar(ref, rtol=2e-3, atol=2e-6, frac=2e-4):
    """what tests/test_gpu_train_max.py::close accepts at each entry of ref"""
    return atol + frac * max(float(np.abs(ref).max()), 1e-6) + rtol * np.abs(ref)


def names_of(k):
    pre = 'c{}.'.format(k)
    return PARAMS + tuple(n for n in ('crf.transitions',) + GATES if pre + 'w.' + n in G.files)


def params_of(k):
    pre = 'c{}.'.format(k)
    p = {n: G[pre + 'w.' + n] for n in names_of(k)}
    p['priority_mat'] = G[pre + 'w.priority_mat']
    return p


def kw_of(cfg):
    return dict(nl=cfg['update_nonlinear'], farnn=cfg['farnn'], sig_k=float(cfg.get('sigmoid_exponent', 5)))


_CACHE = {}


def restate(k, dtype=torch.float64, fault=None, masked=False):
    """(loss, grads, scores) of configuration k, computed once per (k, dtype, fault)"""
    key = (k, dtype, fault, masked)
    if key not in _CACHE:
        cfg = META['configs'][k]
        _CACHE[key] = dxr.train_step(params_of(k), BASE['x'], BASE['lengths'], G['labels'], G['re_tags'], cfg['marryup_type'],
                                     cfg['c1_kdpr'], cfg['c2_kdpr'], cfg.get('c3_pr', 1.0),
                                     additional_nonlinear=cfg.get('additional_nonlinear', 'none'),
                                     use_priority=bool(cfg.get('use_priority')), dtype=dtype, fault=fault,
                                     min_gap=None if fault else META['min_gap'], **kw_of(cfg))
    return _CACHE[key]


def worst_miss(k, loss, grads):
    """the largest (difference / bar) over the loss and every stored gradient of configuration k"""
    pre = 'c{}.'.format(k)
    ref_loss = float(G[pre + 'loss'])
    w = abs(loss - ref_loss) / (2e-5 * max(1.0, abs(ref_loss)))
    for n in names_of(k):
        ref = G[pre + 'g.' + n]
        w = max(w, float((np.abs(grads[n].reshape(ref.shape) - ref) / bar(ref)).max()))
    return w


def flat_pred(k, scores):
    """decode of the reference (:302): arg-max with the threshold on the last real column, or Viterbi under the CRF -- the
    CRF configurations are compared through the mirror on the GPU; here the arg-max ones"""
    lengths = BASE['lengths']
    s = np.concatenate([scores[b, :int(lengths[b])] for b in range(len(lengths))]).copy()
    s[:, -1] = np.minimum(s[:, -1], META['threshold'])
    want = s.argmax(1)
    want[want == s.shape[1] - 1] = META['o_idx']
    return want


# ---- the restatement against the reference's captures -------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('k', range(N_CONFIGS))
def test_restatement_reproduces_the_reference(k, dtype):
    loss, grads, scores = restate(k, dtype)
    assert set(grads) == set(names_of(k))
    assert worst_miss(k, loss, grads) <= 1.0
    if not META['configs'][k]['use_crf']:
        assert np.array_equal(flat_pred(k, scores), G['c{}.flat_pred'.format(k)])


# ---- the fixture's conditions, from the stored data ---------------------------------------------------------------------------
def test_the_fixture_has_the_twelve_configurations_and_short_sequences():
    lengths = BASE['lengths']
    assert (lengths.max() - lengths >= 2).any()
    assert G['re_tags'].shape[1] > lengths.max()
    cfgs = META['configs']
    assert len(cfgs) == N_CONFIGS and META['train_flags']['train_mode'] == 'max'
    with open(os.path.join(GOLDEN, 'decomp_train_max_small.json')) as f:
        assert META['min_gap'] == json.load(f)['min_gap']
    with open(os.path.join(GOLDEN, 'decomp_train_teacher_small.json')) as f:
        sum_cfgs = json.load(f)['configs']
    family = lambda c: (c['marryup_type'], c['farnn'], c['use_crf'], c.get('use_priority', 0), c.get('additional_states', 0))  # noqa: E731
    assert [family(c) for c in cfgs] == [family(c) for c in sum_cfgs]
    pr = [c for c in cfgs if c['marryup_type'] == 'pr']
    assert any(c['c3_pr'] < c['c2_kdpr'] for c in pr) and any(c['c3_pr'] > c['c2_kdpr'] for c in pr)


@pytest.mark.parametrize('k', range(N_CONFIGS))
def test_masking_the_pads_moves_a_stored_gradient_by_ten_bars(k):
    """condition 1, restated: the float64 restatement with the pads masked out of the KL against the STORED gradients"""
    cfg = META['configs'][k]
    keep = dtr.kl_term
    dtr.kl_term = lambda s, re, mode, c1, lengths, fault=None: keep(s, re, mode, c1, lengths, 'mask_pads')
    try:
        loss, grads, _ = dxr.train_step(params_of(k), BASE['x'], BASE['lengths'], G['labels'], G['re_tags'], cfg['marryup_type'],
                                        cfg['c1_kdpr'], cfg['c2_kdpr'], cfg.get('c3_pr', 1.0),
                                        additional_nonlinear=cfg.get('additional_nonlinear', 'none'),
                                        use_priority=bool(cfg.get('use_priority')), **kw_of(cfg))
    finally:
        dtr.kl_term = keep
    pre = 'c{}.'.format(k)
    worst = max(float((np.abs(grads[n].reshape(G[pre + 'g.' + n].shape) - G[pre + 'g.' + n]) / bar(G[pre + 'g.' + n])).max())
                for n in names_of(k))
    assert worst > 10.0, worst


@pytest.mark.parametrize('k', range(N_CONFIGS))
def test_the_gap_rule_holds_at_every_step_of_every_sequence(k):
    """condition 2: float32 and float64, all L steps of both chains, the pad steps included"""
    cfg = META['configs'][k]
    Lmax = int(BASE['lengths'].max())
    w = dxr.table_of(params_of(k), cfg.get('additional_nonlinear', 'none'), bool(cfg.get('use_priority')))
    dxr.check_gap(w, BASE['x'][:, :Lmax], BASE['lengths'], min_gap=META['min_gap'], **kw_of(cfg))


# ---- planted faults ------------------------------------------------------------------------------------------------------------
def applies(fault, k):
    if fault == 'last':               # where exact ties decide something (recorded by the generator from the float64 restatement)
        return k in META['last_seen']
    return fault in ('stop_at_len', 'pad_row', 'sum')     # 'tail_reversed': the fixtures' pad tokens are all the pad word (below)


@pytest.mark.parametrize('fault', ['stop_at_len', 'pad_row', 'sum', 'last'])
def test_planted_faults_miss_every_fixture_they_apply_to(fault):
    hit = 0
    for k in range(N_CONFIGS):
        if not applies(fault, k):
            continue
        hit += 1
        loss, grads, _ = restate(k, torch.float64, fault)
        assert worst_miss(k, loss, grads) > 1.0, (fault, k)
    assert hit >= 2, fault


def drawn_case(seed, S=9, R=7, K=5, V=13, B=4, L=6, farnn=1, crf=False, prio=True, nl='tanh'):
    from test_gpu_train_max import draw
    for s in range(seed, seed + 40):
        w, x, lengths, labels = draw(S, R, K, V, B, L, nl, farnn, crf, prio, seed=s)
        lengths[:] = [L, 0, 1, L - 3][:B]
        try:
            dxr.check_gap(w, x, lengths, nl=nl, farnn=farnn)
        except dxr.GapError:
            continue
        re = (np.random.RandomState(s).rand(B, L, K) * 1.0).astype(np.float32)
        return w, x, lengths, labels, re
    raise AssertionError('no draw keeps the gap rule')


@pytest.mark.parametrize('mode', ['kd', 'pr'])
def test_a_reversed_tail_is_seen_on_distinct_pad_tokens(mode):
    """The fixtures pad with one word, so the order of the backward chain's tail cannot show there; on a drawn batch whose pad
    positions hold distinct words it moves gradients by far more than the bar of tests/util.py::check_grad (1e-4 of the scale)."""
    w, x, lengths, labels, re = drawn_case(3)
    assert len(set(x[3, 3:])) > 1
    _, good, _ = dxr.step_on_table(w, x, lengths, labels, re, mode, 2.0, 0.3, nl='tanh', farnn=1)
    _, bad, _ = dxr.step_on_table(w, x, lengths, labels, re, mode, 2.0, 0.3, nl='tanh', farnn=1, fault='tail_reversed')
    assert max(float(np.abs(bad[n] - good[n]).max() / np.abs(good[n]).max()) for n in good) > 1e-2


@pytest.mark.parametrize('fault', [f for f in dxr.FAULTS if f != 'last'])
def test_every_other_fault_is_seen_on_a_drawn_case(fault):
    """the cases the GPU test draws (distinct pad words, an empty sequence) see the planted faults far above check_grad's bar
    (1e-4 of the scale); 'last' needs exact ties that decide something, which the fixtures have (last_seen) and a random draw
    has not"""
    w, x, lengths, labels, re = drawn_case(5)
    _, good, _ = dxr.step_on_table(w, x, lengths, labels, re, 'kd', 2.0, 0.3, nl='tanh', farnn=1)
    _, bad, _ = dxr.step_on_table(w, x, lengths, labels, re, 'kd', 2.0, 0.3, nl='tanh', farnn=1, fault=fault)
    assert max(float(np.abs(bad[n] - good[n]).max() / np.abs(good[n]).max()) for n in good) > 1e-3


def test_pad_word_rows_of_dvgen_are_not_zero():
    w, x, lengths, labels, re = drawn_case(4)
    valid = np.arange(x.shape[1])[None, :] < lengths[:, None]
    only_pad = sorted(set(x[~valid]) - set(x[valid]))
    assert only_pad
    _, g, _ = dxr.step_on_table(w, x, lengths, labels, re, 'kd', 2.0, 0.3, nl='tanh', farnn=1)
    assert all(np.abs(g['Vgen'][t]).max() > 0 for t in only_pad)
    _, g1, _ = dxr.step_on_table(w, x, lengths, labels, re, 'kd', 2.0, 1.0, nl='tanh', farnn=1)      # pi = 1: the plain step
    assert all(np.abs(g1['Vgen'][t]).max() == 0 for t in only_pad)


# ---- the mirror's switch and refusals: before any device work, so they need no GPU ---------------------------------------------
def mirror(**kw):
    from re2nn_seq_amd.farnn.model_decompose_single import FARNN_S_D_W_I_S
    torch.manual_seed(0)
    return FARNN_S_D_W_I_S(V=BASE['V_in'], S1=BASE['S1_in'], S2=BASE['S2_in'], C_output_mat=BASE['O_in'], wildcard_mat=BASE['W_in'],
                           wildcard_output_vector=BASE['Ow_in'], final_vector=BASE['final_in'], start_vector=BASE['start_in'],
                           pretrained_word_embed=BASE['E_in'], priority_mat=BASE['priority_in'], args=ns(**kw), o_idx=META['o_idx'])


def batch():
    return (torch.from_numpy(BASE['x']), torch.from_numpy(G['labels']), torch.from_numpy(BASE['lengths']),
            torch.from_numpy(G['re_tags']))


TODAY_MAX = ('the KD / PR teacher terms are built for the sum semiring only; --train_mode max walks the valid positions only '
             '(DESIGN.md, row f3)')
TODAY = ('the HIP training step covers the sum and max semirings and the CE1 loss (with or without the CRF), no KD/PR teachers '
         '(DESIGN.md, row f3)')


@pytest.mark.parametrize('mode', ['kd', 'pr'])
def test_without_the_new_switch_the_refusal_is_todays(mode, monkeypatch):
    monkeypatch.setenv('RE2NN_DECOMP_TEACHER_TRAIN', '1')
    monkeypatch.delenv('RE2NN_DECOMP_TEACHER_MAX_TRAIN', raising=False)
    x, lab, lengths, re = batch()
    with pytest.raises(NotImplementedError) as e:
        mirror(marryup_type=mode, train_mode='max').forward_local(x, lab, lengths, train=True, re_tags=re)
    assert str(e.value) == TODAY_MAX


def test_the_new_switch_alone_opens_nothing(monkeypatch):
    monkeypatch.delenv('RE2NN_DECOMP_TEACHER_TRAIN', raising=False)
    monkeypatch.setenv('RE2NN_DECOMP_TEACHER_MAX_TRAIN', '1')
    x, lab, lengths, re = batch()
    with pytest.raises(NotImplementedError) as e:
        mirror(marryup_type='kd', train_mode='max').forward_local(x, lab, lengths, train=True, re_tags=re)
    assert str(e.value) == TODAY


@pytest.mark.parametrize('mode', ['kd', 'pr'])
def test_with_both_switches_the_check_passes(mode, monkeypatch):
    monkeypatch.setenv('RE2NN_DECOMP_TEACHER_TRAIN', '1')
    monkeypatch.setenv('RE2NN_DECOMP_TEACHER_MAX_TRAIN', '1')
    x, lab, lengths, re = batch()
    m = mirror(marryup_type=mode, train_mode='max')
    assert m._check_trainable(re) is True
    with pytest.raises(ValueError, match='needs the RE teacher'):
        m._check_trainable(None)
    with pytest.raises(NotImplementedError) as e:
        mirror(marryup_type='input', train_mode='max').forward_local(x, lab, lengths, train=True)
    assert str(e.value) == TODAY


def test_the_new_entry_is_declared_bound_and_exported():
    import ctypes
    import re as regex
    from re2nn_seq_amd import _lib
    name = 'farnn_decomp_ifst_teacher_max_train_step'
    with open(os.path.join(ROOT, 'include', 'farnn.h')) as f:
        text = regex.sub(r'/\*.*?\*/', '', f.read(), flags=regex.S)
    assert regex.search(r'\bint\s+' + name + r'\s*\(', text)
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES['farnn_decomp_ifst_teacher_train_step']
    assert os.path.exists(_lib.LIB_PATH), 'run __graft_entry__.build() first'
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
