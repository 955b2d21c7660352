"""The training step of the vector-input tagger (FARNN_S_SF), the parts that need no GPU: the oracle
restatement against the reference's own forward(train=True) + backward() (tests/golden/sf_train_small.npz), the GPU cases' own
well-drawnness, the refusals of the Python surface, and a planted-fault check of the comparison itself."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sf_train_ref as sr  # noqa: E402
from oracle import farnn_train_oracle as to  # noqa: E402
from util import GOLDEN, check_grad, ns  # noqa: E402


def fixture():
    with open(os.path.join(GOLDEN, 'sf_train_small.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, 'sf_train_small.npz'))


FIX_KEYS = ('S1', 'S2', 'C_output_mat', 'wildcard_mat', 'h0', 'hT', 'Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2', 'crf.transitions')


@pytest.mark.parametrize('k', range(9))
def test_oracle_restatement_matches_the_reference(k):
    """oracle train_step with Vgen := v.reshape(B L, R) and x = arange(B L) against FARNN_S_SF.forward(train=True) +
    loss.backward() of the reference: the loss, every parameter's gradient and input.grad."""
    meta, g = fixture()
    cfg = meta['configs'][k]
    pre = 'c{}.'.format(k)
    v, lengths, labels = g['v'], g['lengths'], g['labels']
    p = {n: torch.from_numpy(g[pre + 'w.' + n]) for n in FIX_KEYS if pre + 'w.' + n in g.files}
    p['priority_mat'] = torch.from_numpy(g[pre + 'w.priority_mat'])
    case = dict(nl=cfg.get('update_nonlinear', 'none'), prio=bool(cfg.get('use_priority', 0)), farnn=cfg.get('farnn', 0),
                crf=bool(cfg.get('use_crf', 0)))
    assert sr.SIG_K == ns().sigmoid_exponent
    loss, grads, _ = sr.oracle_step(p, v, lengths, labels, case)
    ref_loss = float(g[pre + 'loss'])
    assert abs(loss - ref_loss) < 2e-5 * max(1.0, abs(ref_loss))
    checked = 0
    for n in FIX_KEYS + ('v',):
        if pre + 'g.' + n not in g.files:
            continue
        ref = g[pre + 'g.' + n]
        scale = max(float(np.abs(ref).max()), 1e-6)
        np.testing.assert_allclose(grads[n].reshape(ref.shape), ref, rtol=2e-3, atol=2e-6 + 2e-4 * scale, err_msg=n)
        checked += 1
    assert checked >= 4 and pre + 'g.v' in g.files
    mask = sr.valid_mask(lengths, v.shape[1])
    assert not g[pre + 'g.v'][~mask].any() and not grads['v'][~mask].any()          # the reference itself leaves the pads' rows zero


@pytest.mark.parametrize('name', sr.CASE_IDS)
def test_gpu_cases_are_well_drawn(name):
    """check_grad's own conditions, from the references alone: the float32 oracle judged as if it were the kernel passes, so it
    sits within tol / 10 of float64 on every tensor, and at most 1 % of the valid positions' rows of dv fall back."""
    case = sr.by_name(name)
    p, v, lengths, labels, ref32, ref64 = sr.refs(name)
    got = {n: ref32[1][sr.ORACLE_KEY[n]] for n in sr.grad_names(case)}
    got['v'] = ref32[1]['v']
    sr.check_all(case, ref32[0], got, ref32, ref64, lengths, check_grad)
    assert int(np.asarray(lengths).sum()) > 0
    # and the tags: the float64 scores decide (tests/sf_tag_ref.decided) at least half of the valid positions, so that every case
    # compares tags (relutanh leaves exact zeros, whose ties are real; one close CRF path leaves its whole sequence out)
    mask = sr.valid_mask(lengths, v.shape[1])
    decided = sr.decided_tags(ref64[2], lengths, v.shape[1], 0.5, p['crf.transitions'].numpy() if case['crf'] else None)
    assert decided[mask].mean() >= 0.5


def test_the_cases_cover_what_the_kernels_branch_on():
    cs = sr.CASES
    assert {(c['S'], c['R']) for c in cs} == set(sr.SHAPES)
    assert {c['B'] for c in cs} == {1, 3, 5} and {c['L'] for c in cs} == {1, 2, 9}
    assert any({0, 1, c['L']} <= set(c['lengths']) for c in cs) and any(min(c['lengths']) == c['L'] > 1 for c in cs)
    assert {(c['farnn'], c['crf']) for c in cs} == {(f, c) for f in (0, 1, 2) for c in (False, True)}
    assert {(c['nl'], c['prio']) for c in cs} >= {(n, q) for n in ('none', 'tanh', 'relutanh') for q in (False, True)}


def sf_model(**cfg):
    from re2nn_seq_amd.farnn.model_decompose_single import FARNN_S_SF
    g = np.load(os.path.join(GOLDEN, 'decomp_small.npz'))
    with open(os.path.join(GOLDEN, 'decomp_small.json')) as f:
        meta = json.load(f)
    m = FARNN_S_SF(S1=g['S1_in'], S2=g['S2_in'], C_output_mat=g['O_in'], wildcard_mat=g['W_in'], wildcard_output_vector=g['Ow_in'],
                   final_vector=g['final_in'], start_vector=g['start_in'], priority_mat=g['priority_in'],
                   args=ns(independent=2, threshold=meta['threshold'], **cfg), o_idx=meta['o_idx'])
    v = torch.zeros(2, 3, m.R)
    return m, v, torch.zeros(2, 3, dtype=torch.int64), torch.tensor([3, 1])


def test_training_is_opt_in(monkeypatch):
    """Without RE2NN_SF_TRAIN=1, train=True raises what it raised before the step existed."""
    monkeypatch.delenv('RE2NN_SF_TRAIN', raising=False)
    m, v, lab, ln = sf_model()
    with pytest.raises(NotImplementedError, match='is not built \\(DESIGN.md, row f14\\); call forward\\(..., train=False\\)'):
        m.forward(v, lab, ln, train=True)
    assert list(m.parameters()) == []


TEACHER_REFUSAL = 'KD / PR teacher terms .* are not built.*DESIGN.md, row f14'


@pytest.mark.parametrize('marryup', ['kd', 'pr'])
def test_marryup_types_are_refused(monkeypatch, marryup):
    """--marryup_type kd | pr under the switch, with or without re_tags: the teacher's own refusal (not the opt-in's), before any
    device work."""
    monkeypatch.setenv('RE2NN_SF_TRAIN', '1')
    m, v, lab, ln = sf_model(marryup_type=marryup)
    for re_tags in (None, torch.zeros(2, 3, 3)):
        with pytest.raises(NotImplementedError, match=TEACHER_REFUSAL):
            m.forward(v, lab, ln, train=True, re_tags=re_tags)
    assert getattr(m, '_tc', None) is None


def test_re_tags_are_refused(monkeypatch):
    """re_tags given under --marryup_type none: the same refusal, never a silently dropped teacher term."""
    monkeypatch.setenv('RE2NN_SF_TRAIN', '1')
    m, v, lab, ln = sf_model()
    with pytest.raises(NotImplementedError, match=TEACHER_REFUSAL):
        m.forward(v, lab, ln, train=True, re_tags=torch.zeros(2, 3, 3))
    assert getattr(m, '_tc', None) is None


def test_train_flags_follow_the_reference():
    """requires_grad of FARNN_S_SF's parameters (ref model_decompose_single.py:343-401) and of EmbedAggregator's (bert_embeddings.py:50-71)."""
    from re2nn_seq_amd.farnn.embed_aggregator import EmbedAggregator
    m, *_ = sf_model(farnn=2, use_crf=1, train_h0=1, train_wildcard=0, train_c_output=1)
    assert dict(m._train_decl()) == {'S1': True, 'S2': True, 'C_output_mat': True, 'wildcard_mat': False, 'h0': True, 'hT': False,
                                     'Wss1': True, 'Wrs1': True, 'bs1': True, 'Wss2': True, 'Wrs2': True, 'bs2': True,
                                     'crf.transitions': True}
    g = np.load(os.path.join(GOLDEN, 'decomp_small.npz'))
    agg = EmbedAggregator(ns(train_V_embed=0, train_beta=1), g['V_in'], g['E_in'])
    assert list(agg.parameters()) == []
    agg.requires_grad_()
    assert [k for k, _ in agg.named_parameters()] == ['embed_r_generalized', 'beta_vec']
    agg.encoder = torch.nn.Linear(3, 4)
    assert [k for k, _ in agg.named_parameters()] == ['embed_r_generalized', 'beta_vec', 'encoder.weight', 'encoder.bias']
    assert list(agg.requires_grad_(False).parameters()) == list(agg.encoder.parameters())


@pytest.mark.parametrize('name', ['S9R7-B5L9-f2-relutanh', 'S70R70-B5L9-f1-relutanh-crf'])
def test_the_comparison_sees_planted_faults(name):
    """dv split into the three terms sf_dv_kernel adds: their sum passes check_grad against the oracle; the backward chain's row
    taken at t instead of len - t, or the gate term dropped, does not."""
    case = sr.by_name(name)
    assert case['farnn'] >= 1 and len(set(case['lengths'])) > 2
    p, v, lengths, labels, ref32, ref64 = sr.refs(name)
    loss, DVf, DVb, GT = sr.split_dv(p, v, lengths, labels, case)
    assert abs(loss - ref64[0]) < 1e-9 * max(1.0, abs(ref64[0]))
    B, L, R = v.shape
    present = sr.valid_mask(lengths, L).reshape(-1)
    flat = lambda a: a.reshape(B * L, R)      # noqa: E731

    def judge(dv):
        check_grad(name, 'dv', flat(dv), flat(ref32[1]['v']), flat(ref64[1]['v']), slices=0, present=present)
    good = sr.assemble_dv(DVf, DVb, GT, lengths)
    np.testing.assert_allclose(good, ref64[1]['v'], rtol=0, atol=1e-9 * np.abs(ref64[1]['v']).max())
    judge(good)
    with pytest.raises(AssertionError, match='dv'):
        judge(sr.assemble_dv(DVf, DVb, GT, lengths, backward_row='t'))
    with pytest.raises(AssertionError, match='dv'):
        judge(sr.assemble_dv(DVf, DVb, GT, lengths, gate=False))
