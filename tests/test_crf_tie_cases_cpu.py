"""The INPUTS of tests/test_gpu_crf_ties.py (tests/crf_tie_cases.py), judged by the oracle alone: the planted scores are what the
oracle computes, exact ties really occur where the kernels' work splits care about them, and a decode that breaks the first-index
rule (viterbi_last_index) really gives other tags.  Nothing here touches the library.  Run with -s for the per-case counts.

The floors are conditions on the inputs; a draw that misses one is redrawn (crf_tie_cases.SEED_BUMP), the floor stays:
  per case   at least 25 % of the back-trace steps are ties; dense cases with more than 32 real tags: at least 10 steps tie across
             two 32-source blocks; the last-index decode differs from the oracle's in at least half of the sequences;
  the grid   every tag count with more than 64 real tags has a tie across two 64-lane slices; every tag count with a real tag among
             its leftover sources (K % 32 >= 3) has a tie that involves one; a tie involves the clamped column K - 3; a terminal
             arg-max is tied.
"Real tags" (C = K - 2), not K: START and STOP are never maximal sources -- tr[STOP, :] = -10000, and part[START] carries the
-10000 of tr[:, START] -- so at K = 33, 34 no tie can cross a block, at K = 65, 66 none can cross a slice, and where the leftover
sources are START / STOP alone (K % 32 in 1, 2) none can involve a leftover.
"""
import numpy as np
import pytest

from oracle import farnn_oracle as fo
import crf_tie_cases as tc

IDS = [tc.case_id(c) for c in tc.CASES]


def _viterbi_float64(feats, lengths, tr):
    """crf.py:102-195 restated from its description, in float64 and on its own (no code of fo.viterbi_paths): the partition of a tag
    is the best score of a path that ends in it; the back-pointer is the FIRST best previous tag; the path ends in the first best
    tag under the transition to STOP and follows the back-pointers."""
    feats = np.asarray(feats, np.float64); tr = np.asarray(tr, np.float64)
    Bn, L, K = feats.shape
    start, stop = K - 2, K - 1
    out = np.zeros((Bn, L), np.int64)
    for b in range(Bn):
        n = int(lengths[b])
        if n == 0:
            continue
        score = feats[b, 0] + tr[start]
        back = []
        for t in range(1, n):
            cand = feats[b, t][None, :] + tr + score[:, None]           # [previous tag i, tag j]
            best, bp = cand[0].copy(), np.zeros(K, np.int64)
            for i in range(1, K):                           # a scan over the previous tags, every tag j at once
                up = cand[i] > best                         # strictly greater: the first index stays
                best[up] = cand[i][up]
                bp[up] = i
            score = best
            back.append(bp)
        end = np.asarray(score) + tr[:, stop]
        tag = 0
        for i in range(1, K):
            if end[i] > end[tag]:
                tag = i
        for t in range(n - 1, -1, -1):
            out[b, t] = tag
            if t > 0:
                tag = back[t - 1][tag]
    return out


@pytest.mark.parametrize('c', tc.CASES, ids=IDS)
def test_case_inputs_and_floors(c):
    r = tc.reference(c)
    T, W, O, h0, hT = r.model
    C = c.K - 2
    assert len(c.lengths) == tc.B and max(c.lengths) == c.L
    assert c.L == 130 or {0, 1, 2, 3} <= set(c.lengths)
    assert c.o_idx not in (0, c.K - 3)
    assert (O.sum(0) == 1).all() and O.shape == (C, c.S)
    one_hot = bool((((O == 1).sum(0) == 1) & ((O != 0).sum(0) == 1)).all())
    assert one_hot == (c.o_kind == 'labelmap')             # (the dense ones must not qualify as a label map)
    # the oracle's scores ARE the planted columns, exactly, and small integers
    assert np.array_equal(r.scores[r.mask], tc.planted_scores(O, r.smap, r.x, r.lengths)[r.mask])
    assert np.array_equal(r.scores, np.round(r.scores)) and float(np.abs(r.scores).max()) < 64
    assert float(np.abs(r.tr[:C, :C]).max()) <= 1
    # tie_stats walked the oracle's own path
    st = r.stats
    paths = np.array(st.paths)
    paths[paths == c.K - 3] = c.o_idx
    assert np.array_equal(paths[r.mask], r.want[r.mask])
    assert st.steps == sum(max(n - 1, 0) for n in c.lengths)
    print('{:<44} steps {:>4}  tied {:>4}  cross-block {:>4}  cross-slice {:>4}  leftover {:>4}  K-3 {:>4}  terminal {}/{}'.format(
        tc.case_id(c), st.steps, st.tied, st.cross_block, st.cross_slice, st.leftover, st.clamp_col, st.terminal, tc.B))
    assert tc.unmet_floors(c, r) == []


def test_grid_floors():
    by_k = {}
    for c in tc.CASES:
        by_k.setdefault(c.K, []).append(tc.reference(c).stats)
    assert sorted(by_k) == sorted(tc.TAG_COUNTS)
    for K in (4, 33, 34, 64, 65, 66, 75, 96, 97, 128, 129, 130, 131, 160, 161, 192, 193, 223, 224, 256):
        assert K in by_k
    for K, sts in by_k.items():
        if K - 2 > 64:
            assert sum(s.cross_slice for s in sts) >= 1, K
        if K % 32 >= 3:
            assert sum(s.leftover for s in sts) >= 1, K
        else:                                              # the leftover sources are START / STOP (or there is none)
            assert all(i >= K - 2 for i in range(32 * (K // 32), K)), K
    assert sum(s.clamp_col for sts in by_k.values() for s in sts) >= 1
    assert sum(s.terminal for sts in by_k.values() for s in sts) >= 1
    thr = [c.threshold for c in tc.CASES]
    assert 0.35 <= thr.count(1.0) / len(thr) <= 0.65 and set(thr) == {0.5, 1.0}
    assert {c.S for c in tc.CASES} == {16, 72, 104} and any(c.K == 75 and c.S == 104 for c in tc.CASES)
    assert not any(c.o_kind == 'labelmap' and c.tr_kind == 'default' for c in tc.CASES)
    for K in (k for k in tc.TAG_COUNTS if k <= 75):
        assert any(c.K == K and c.lengths == tc.EDGE_LENGTHS and c.L == 130 for c in tc.CASES), K
    assert all(c.L <= 64 for c in tc.CASES if c.K > 75)


def test_every_kernel_form_is_reached():
    """the restated LDS condition sends the grid through every instantiation: the history form with the scores inside and behind
    the score kernel at every block count 0..6, the back-pointer kernel at each of its five block sizes"""
    forms = {}
    for c in tc.CASES:
        for sw in ((), ('FARNN_VITERBI_UNFUSED',), ('FARNN_VITERBI_BP', 'FARNN_VITERBI_UNFUSED')):
            forms.setdefault(tc.expected_form(c.K, c.S, c.L, sw), set()).add(c.K)
    assert {k // 32 for k in forms[tc.FUSED]} == set(range(7))
    assert {k // 32 for k in forms[tc.HISTORY]} == set(range(7))
    need = lambda K: ((K + 3) // 4 + 3) // 4                # noqa: E731  (csrc/score_decode.hip.h: viterbi_ib4)
    sizes = {2 if need(k) <= 2 else 4 if need(k) <= 4 else 9 if need(k) <= 9 else 13 if need(k) <= 13 else 16 for k in forms[tc.BACKPOINTERS]}
    assert sizes == {2, 4, 9, 13, 16}
    # without a switch: K >= 224 has no history instantiation, K = 223's table alone is past the budget, K = 75 at L = 130 fits
    assert tc.expected_form(224, 16, 64) == tc.expected_form(223, 104, 64) == tc.BACKPOINTERS
    assert tc.expected_form(75, 104, 130) == tc.FUSED and tc.expected_form(130, 72, 64) == tc.FUSED
    assert tc.expected_form(193, 72, 6) == tc.HISTORY and tc.expected_form(193, 72, 64) == tc.BACKPOINTERS


@pytest.mark.parametrize('c', tc.CASES, ids=IDS)
def test_oracle_decode_against_a_float64_restatement(c):
    """integers: float32 and float64 are both exact, so this checks the oracle's decode itself (first index at every arg-max)"""
    r = tc.reference(c)
    ext, lengths, tr, want, mask = r.ext, r.lengths, r.tr, r.want, r.mask
    own = _viterbi_float64(tc.clamped(ext, c.threshold), lengths, tr)
    own[own == c.K - 3] = c.o_idx
    mask = tc.valid_mask(lengths, c.L)
    assert np.array_equal(own[mask], want[mask])


def test_last_index_decode_is_a_different_decode():
    """viterbi_last_index equals the oracle wherever nothing ties (random float transitions) and nowhere else in general"""
    c = tc.CASES[5]
    r = tc.reference(c)
    rng = np.random.RandomState(1)
    tr = fo.crf_default_transitions(c.K - 2) + rng.randn(c.K, c.K).astype(np.float32)
    a = tc.viterbi_last_index(r.ext, r.lengths, tr, c.threshold, c.o_idx)
    assert np.array_equal(a[r.mask], fo.decode_crf(r.ext, r.lengths, tr, c.threshold, c.o_idx)[r.mask])
    b = tc.viterbi_last_index(r.ext, r.lengths, r.tr, c.threshold, c.o_idx)
    assert not np.array_equal(b[r.mask], r.want[r.mask])


@pytest.mark.parametrize('a', tc.ARGMAX_CASES, ids=[tc.argmax_case_id(a) for a in tc.ARGMAX_CASES])
def test_argmax_case_inputs(a):
    """the non-CRF decode of the same models: the clamped last column ties a label in front of it (dense: threshold 1.0; a label
    map: threshold 0.0 -- a one-hot row has nothing equal to 1), and the C port of the oracle decodes like the numpy one"""
    from oracle import c_port
    r, g = tc.reference(a.case), tc.argmax_reference(a)
    print('{:<28} positions {:>4}  threshold ties {:>3}'.format(tc.argmax_case_id(a), int(r.mask.sum()), g.threshold_ties))
    if a.case.o_kind == 'dense' or a.threshold == 0.0:
        assert g.threshold_ties >= 1
    T, W, O, h0, hT = r.model
    tags, scores, _ = c_port.onehot_ifst_tag(T + W, O, h0, hT, r.x, r.lengths, 0, 0, a.threshold, a.case.o_idx, want_scores=True, nthreads=2)
    assert np.array_equal(scores[r.mask], r.scores[r.mask])
    assert np.array_equal(tags[r.mask].astype(np.int64), g.want[r.mask]) and (tags[~r.mask] == -1).all()
