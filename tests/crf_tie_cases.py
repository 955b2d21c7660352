"""Planted tie cases for the CRF decode (plain numpy, no GPU): onehot i-FST models whose scores are small integers that depend on
the token's word alone, so that every form of the library computes them bit for bit and the decode alone is under test, with
transitions (the reference's initial CRF, or small integers on top of it) under which many candidates of an arg-max are EQUAL.
Every arg-max of the decode then has to follow torch.max's rule -- the first index of the maximum (crf.py:147-149).

The model (S states, C labels, V words, the last word the pad):
    T[w][:, s(w)] = 1 for a random map s: word -> state, everything else 0;  W = 0;  h0 = e_0;  hT = 1;
    O [C, S] with every column summing to 1 (the recurrence multiplies by O.sum(0), model_onehot.py:368).
Then alpha_t = e_{s(x_t)}, beta_t = 1 and score[b, t, :] = O[:, s(x_t)] at every valid position.  All sums stay far below 2**24:
every float32 expression on either side is exact, and the tolerance is none.

Two kinds of O: `dense` (entries from {0, 1, 2}, +-1 corrections until a column sums to 1: the matrix-core score path) and
`labelmap` (one 1 per column: the label-map scan).  Two kinds of transitions: `default` (crf.py:31-46: zeros and the two -10000
barriers) and `int` (default + randint(-1, 2), barriers restored).

tie_stats counts, along the oracle's decoded path, the ties the kernels' work splits care about; viterbi_last_index is the same
decode taking the LAST maximal index: a wrong decode of the kind a kernel could fall into.
"""
import collections
import functools

import numpy as np

from oracle import farnn_oracle as fo

F32 = np.float32
B = 8
V = 48                                                     # words of every planted model, the last one the pad
LDS_LIMIT = 158 * 1024                                     # the history form's LDS budget (csrc/farnn_hip.hip: launch_viterbi)

Case = collections.namedtuple('Case', 'K S L lengths o_kind tr_kind threshold o_idx seed')


def case_id(c):
    return 'K{}-S{}-L{}-{}-{}-thr{}'.format(c.K, c.S, c.L, c.o_kind, c.tr_kind, c.threshold)


# ------------------------------------------------------------------------------------------------ the planted model
def _dense_output(C, S, rng):
    if C <= 3:                                             # small C: columns written directly (each sums to 1, none a label map's only)
        cols = {2: [(1, 0), (0, 1), (2, -1), (-1, 2), (1, 0)], 3: [(1, 0, 0), (0, 0, 1), (1, 1, -1), (2, 0, -1), (0, 2, -1), (-1, 1, 1)]}[C]
        O = np.array([cols[i] for i in rng.randint(0, len(cols), size=S)], F32).T
        O[:, 0] = cols[2]                                  # (never a label map: a weight of 2)
        return np.ascontiguousarray(O)
    p2 = min(0.1, 3.0 / C)                                 # (a few 2s per column at any C: small sets of maximal sources, spread over the blocks)
    O = rng.choice([0, 1, 2], size=(C, S), p=[0.6, 0.4 - p2, p2]).astype(np.int64)
    for s in range(S):
        d = 1 - int(O[:, s].sum())
        rows = rng.randint(0, C, size=abs(d))
        np.add.at(O[:, s], rows, 1 if d > 0 else -1)
    assert (O.sum(0) == 1).all()
    return O.astype(F32)


def _labelmap_output(C, S, rng):
    O = np.zeros((C, S), F32)
    O[rng.randint(0, C, size=S), np.arange(S)] = 1.0
    return O


def planted_model(c):
    """(T, W, O, h0, hT, smap) of a case; V = len(smap) + 1 words, the last one the pad (an all-zero block)."""
    rng = np.random.RandomState(c.seed)
    C, S = c.K - 2, c.S
    smap = rng.randint(0, S, size=V - 1)
    T = np.zeros((V, S, S), F32)
    T[np.arange(V - 1), :, smap] = 1.0
    W = np.zeros((S, S), F32)
    O = _dense_output(C, S, rng) if c.o_kind == 'dense' else _labelmap_output(C, S, rng)
    h0 = np.zeros(S, F32); h0[0] = 1.0
    hT = np.ones(S, F32)
    return T, W, O, h0, hT, smap


def batch(c):
    rng = np.random.RandomState(c.seed + 1)
    lengths = np.asarray(c.lengths, np.int64)
    x = np.full((len(lengths), c.L), V - 1, np.int64)
    for b, n in enumerate(lengths):
        x[b, :n] = rng.randint(0, V - 1, size=int(n))
    return x, lengths


def transitions(c):
    C = c.K - 2
    tr = fo.crf_default_transitions(C)
    if c.tr_kind == 'int':
        rng = np.random.RandomState(c.seed + 2)
        tr = tr + rng.randint(-1, 2, size=tr.shape).astype(F32)
        tr[:, c.K - 2] = -10000.0
        tr[c.K - 1, :] = -10000.0
    return tr


def planted_scores(O, smap, x, lengths):
    """[B, L, C]: O[:, s(x_t)] at the valid positions, zero at the pads."""
    Bn, L = x.shape
    out = np.zeros((Bn, L, O.shape[0]), F32)
    for b in range(Bn):
        n = int(lengths[b])
        out[b, :n] = O[:, smap[x[b, :n]]].T
    return out


def valid_mask(lengths, L):
    return np.arange(L)[None, :] < np.asarray(lengths)[:, None]


def clamped(ext_scores, threshold):
    """the decode's view of the extended scores: column K-3 capped at the threshold (model_decompose.py:353)"""
    s = np.array(ext_scores, F32, copy=True)
    K = s.shape[-1]
    s[..., K - 3] = np.minimum(s[..., K - 3], F32(threshold))
    return s


# ------------------------------------------------------------------------------------------------ decodes of its own
def _steps(feats_b, n, tr):
    """the oracle's dynamic programme over one sequence: [cur_1 .. cur_{n-1}] ([K, K] candidates of every step) and `last`"""
    part = (feats_b[0] + tr[tr.shape[0] - 2]).astype(F32)
    curs = []
    for t in range(1, n):
        cur = (feats_b[t][None, :] + tr) + part[:, None]
        curs.append(cur)
        part = cur.max(axis=0).astype(F32)
    return curs, (part[:, None] + tr)[:, tr.shape[0] - 1]


def _last_argmax(v):
    return len(v) - 1 - int(np.argmax(v[::-1]))


def viterbi_last_index(ext_scores, lengths, tr, threshold, o_idx):
    """fo.decode_crf with the LAST maximal index at every arg-max (the terminal one and every back-pointer)."""
    feats = clamped(ext_scores, threshold)
    tr = np.asarray(tr, F32)
    Bn, L, K = feats.shape
    out = np.zeros((Bn, L), np.int64)
    for b in range(Bn):
        n = int(lengths[b])
        if n == 0:
            continue
        curs, last = _steps(feats[b], n, tr)
        ptr = _last_argmax(last)
        out[b, n - 1] = ptr
        for t in range(n - 1, 0, -1):
            ptr = _last_argmax(curs[t - 1][:, ptr])
            out[b, t - 1] = ptr
    out[out == K - 3] = o_idx
    return out


TieStats = collections.namedtuple('TieStats', 'steps tied cross_block cross_slice leftover clamp_col terminal paths')


def tie_stats(feats, lengths, tr):
    """Walks the oracle's Viterbi (first index) over `feats` (the CLAMPED extended scores) and counts along the decoded path:
    steps       back-trace steps (n - 1 per sequence)
    tied        ... with two or more maximal sources
    cross_block ... whose first two maximal sources lie in different 32-source blocks
    cross_slice ... in different 64-slices
    leftover    ... where a maximal source is a leftover source (index >= 32 * (K // 32)) of a tie
    clamp_col   ... where a maximal source of a tie is K - 3 (the column clamped to the threshold)
    terminal    sequences whose terminal arg-max is tied
    paths       the decoded tags [B, L] (zeros at pads), before K - 3 is mapped to o_idx"""
    feats = np.asarray(feats, F32); tr = np.asarray(tr, F32)
    Bn, L, K = feats.shape
    n_steps = tied = xb = xs = lo = cc = term = 0
    paths = np.zeros((Bn, L), np.int64)
    for b in range(Bn):
        n = int(lengths[b])
        if n == 0:
            continue
        curs, last = _steps(feats[b], n, tr)
        term += int((last == last.max()).sum() >= 2)
        ptr = int(last.argmax())
        paths[b, n - 1] = ptr
        for t in range(n - 1, 0, -1):
            col = curs[t - 1][:, ptr]
            M = np.flatnonzero(col == col.max())
            n_steps += 1
            if len(M) >= 2:
                tied += 1
                xb += int(M[0] // 32 != M[1] // 32)
                xs += int(M[0] // 64 != M[1] // 64)
                lo += int(M[-1] >= 32 * (K // 32))
                cc += int(K - 3 in M)
            ptr = int(M[0])
            paths[b, t - 1] = ptr
    return TieStats(n_steps, tied, xb, xs, lo, cc, term, paths)


# ------------------------------------------------------------------------------------------------ which kernel a case takes
def _products_stride(SP):
    q = (SP + 15) & ~15
    return q if (q >> 2) & 1 else q + 4


def _hist_floats(Kp, SP, L, fused):
    return max(L * Kp, ((L + 15) & ~15) * _products_stride(SP) if fused else 0)


def _table_pieces(K, Kp, SP, L, fused):
    tr_pieces = (K * Kp * 4 + 1023) // 1024
    if not fused:
        return tr_pieces
    otm_pieces = ((K + 15) >> 4) * ((SP + 15) >> 4)
    if otm_pieces <= tr_pieces:
        return tr_pieces
    with_image = _hist_floats(Kp, SP, L, True) * 4 + (L * Kp * 4 + 1023) // 1024 * 1024 + otm_pieces * 1024
    return otm_pieces if with_image <= LDS_LIMIT else tr_pieces


def viterbi_hist_lds_bytes(K, S, L, fused):
    """csrc/viterbi_hist.hip.h restated: the partitions' history (the fused form first stages its products there), the sequence's
    scores in whole KiB, and the transposed transition table (or the output matrix's image where that is larger and fits)."""
    Kp, SP = (K + 3) & ~3, (S + 3) & ~3
    return _hist_floats(Kp, SP, L, fused) * 4 + (L * Kp * 4 + 1023) // 1024 * 1024 + _table_pieces(K, Kp, SP, L, fused) * 1024


FUSED, HISTORY, BACKPOINTERS = 'fused-history', 'history', 'backpointers'


def expected_form(K, S, L, switches=()):
    """the Viterbi kernel launch_score_decode / launch_viterbi pick (csrc/farnn_hip.hip): the history form wherever
    viterbi_hist_lds_bytes <= 158 KiB (and K < 224), with the scores computed inside it unless switched off; else the
    stored-back-pointer kernel"""
    bp, unfused = 'FARNN_VITERBI_BP' in switches, 'FARNN_VITERBI_UNFUSED' in switches
    if bp:
        return BACKPOINTERS
    if K // 32 > 6:
        return BACKPOINTERS
    if not unfused and K <= 256 and viterbi_hist_lds_bytes(K, S, L, True) <= LDS_LIMIT:
        return FUSED
    return HISTORY if viterbi_hist_lds_bytes(K, S, L, False) <= LDS_LIMIT else BACKPOINTERS


# ------------------------------------------------------------------------------------------------ the grid
# tag counts K = C + 2: the smallest; one block + leftovers; the slice boundary; the shipped configuration; the block boundary; the
# tail pair (START / STOP at K = 130); larger IB4; the last size with a history instantiation; the back-pointer kernel
# (40, 68, 164: one block, two, five + leftover sources that are real tags -- at 33, 34, 65, 66, 97, 129, 130, 161, 193 the leftover
#  sources are START / STOP alone, which the -10000 barriers keep from ever being maximal)
TAG_COUNTS = (4, 33, 34, 40, 64, 65, 66, 68, 75, 96, 97, 128, 129, 130, 131, 160, 161, 164, 192, 193, 223, 224, 256)
STATE_COUNTS = (16, 72, 104)
EDGE_LENGTHS = (63, 64, 65, 66, 127, 128, 129, 130)        # the back-trace's blocks of 64 positions, two steps per trip


def _history_length(K, S):
    """the longest L <= 64 (of a few) at which the history form still holds a K-tag table beside L rows, fused or not"""
    for L in (64, 40, 24, 12, 6):
        if viterbi_hist_lds_bytes(K, S, L, True) <= LDS_LIMIT and viterbi_hist_lds_bytes(K, S, L, False) <= LDS_LIMIT:
            return L
    for L in (12, 6):                                      # (K = 193: the history beside the score kernel only)
        if viterbi_hist_lds_bytes(K, S, L, False) <= LDS_LIMIT:
            return L
    return 64                                              # no history at any length (K >= 223: the table alone is 195 KiB)


def _lengths(L, rng):
    """eight ragged lengths: 1, 2, 3 and an empty sequence in every batch, L itself, three more (L < 8: all four at L)"""
    rest = [L] + ([L] * 3 if L < 8 else [int(v) for v in rng.randint(4, L + 1, size=3)])
    ls = [min(v, L) for v in (1, 2, 3, 0)] + rest
    return tuple(int(ls[i]) for i in rng.permutation(len(ls)))


# Draws that missed a coverage floor of tests/test_crf_tie_cases_cpu.py (conditions on the inputs, judged by the oracle alone) were
# redrawn with the next seed: (K, L, o_kind, tr_kind) -> how many seeds further.
SEED_BUMP = {(4, 64, 'dense', 'int'): 9, (4, 64, 'labelmap', 'int'): 2, (40, 64, 'dense', 'int'): 3, (192, 6, 'dense', 'int'): 36, (193, 6, 'dense', 'default'): 2,
             (193, 6, 'dense', 'int'): 24, (4, 130, 'dense', 'int'): 19}


def _case(K, S, L, lengths, o_kind, tr_kind, thr, seed):
    o_idx = 1 if K > 4 else K - 1                          # neither 0 nor K - 3
    return Case(K, S, L, tuple(lengths), o_kind, tr_kind, thr, o_idx, seed + SEED_BUMP.get((K, L, o_kind, tr_kind), 0))


def _grid():
    cases = []
    for i, K in enumerate(TAG_COUNTS):
        S = 104 if K == 75 else STATE_COUNTS[i % 3]
        L = _history_length(K, S)
        # (two labels: a column (a, 1 - a) never holds two equal entries, clamped or not -- default transitions cannot tie there;
        #  a label map under default transitions: a one-hot emission leaves a unique maximum)
        kinds = [('dense', 'default'), ('dense', 'int'), ('labelmap', 'int')] if K > 4 else [('dense', 'int'), ('labelmap', 'int')]
        for j, (ok, tk) in enumerate(kinds):
            seed = 1000 * K + 10 * j
            thr = 1.0 if (i + j) % 2 == 0 or K == 4 else 0.5
            cases.append(_case(K, S, L, _lengths(L, np.random.RandomState(seed + 3)), ok, tk, thr, seed))
        if K in (160, 192, 193) and L < 64:                        # ... and at L = 64, where these tag counts leave the history form
            cases.append(_case(K, S, 64, _lengths(64, np.random.RandomState(7 * K)), 'dense', 'int', 1.0, 1000 * K + 50))
    # the shipped tag count over the other state counts
    for S in (16, 72):
        cases.append(_case(75, S, 64, _lengths(64, np.random.RandomState(75 + S)), 'dense', 'default', 1.0, 75000 + S))
    # the back-trace's block edges: K <= 75, L = 130, odd and even n at both edges
    for i, K in enumerate(k for k in TAG_COUNTS if k <= 75):
        S = 104 if K == 75 else STATE_COUNTS[(i + 1) % 3]
        tk = 'default' if i % 2 == 0 and K > 4 else 'int'
        cases.append(_case(K, S, 130, EDGE_LENGTHS, 'dense', tk, 1.0 if i % 2 or K == 4 else 0.5, 2000 * K + 7))
    cases.append(_case(75, 104, 130, EDGE_LENGTHS, 'labelmap', 'int', 1.0, 150027))
    assert len(set(cases)) == len(cases) and len({case_id(c) for c in cases}) == len(cases)
    return tuple(cases)


CASES = _grid()

Reference = collections.namedtuple('Reference', 'model smap x lengths tr scores ext want flat mask stats')


def _freeze(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(c):
    """Everything the oracle says about a case, computed once and read-only: the model, the batch, the transitions, the oracle's
    scores [B, L, C] and their CRF extension, the decoded tags and their flat form, the valid mask, the tie counts."""
    T, W, O, h0, hT, smap = planted_model(c)
    x, lengths = batch(c)
    tr = transitions(c)
    scores = fo.onehot_ifst_scores(T, W, O, h0, hT, x, lengths)
    ext = fo.onehot_crf_extension_scores(scores)
    want = fo.decode_crf(ext, lengths, tr, c.threshold, c.o_idx)
    flat = fo.flatten(want, lengths)
    mask = valid_mask(lengths, c.L)
    stats = tie_stats(clamped(ext, c.threshold), lengths, tr)
    _freeze(stats.paths)
    model = tuple(_freeze(a) for a in (T, W, O, h0, hT))
    return Reference(model, _freeze(smap), _freeze(x), _freeze(lengths), _freeze(tr), _freeze(scores), _freeze(ext), _freeze(want),
                     _freeze(flat), _freeze(mask), stats)


def unmet_floors(c, r):
    """The coverage floors of ONE case (conditions on the inputs; the oracle alone decides): the names of those it misses.
    C = K - 2 real tags: START and STOP are never maximal sources (the -10000 barriers), so a tie across two 32-source blocks
    needs C > 32."""
    st, C = r.stats, c.K - 2
    out = []
    if 4 * st.tied < st.steps or st.steps == 0:
        out.append('tie share {}/{} below 25 %'.format(st.tied, st.steps))
    if c.o_kind == 'dense' and C > 32 and st.cross_block < 10:
        out.append('{} cross-block ties, below 10'.format(st.cross_block))
    last = viterbi_last_index(r.ext, r.lengths, r.tr, c.threshold, c.o_idx)
    differ = sum(int((last[b][r.mask[b]] != r.want[b][r.mask[b]]).any()) for b in range(len(r.lengths)))
    if 2 * differ < len(r.lengths):
        out.append('the last-index decode differs in {} of {} sequences only'.format(differ, len(r.lengths)))
    return out


# ------------------------------------------------------------------------------------------------ the non-CRF decode of the same models
# use_crf = False: C columns, the LAST one clamped to the threshold (model_onehot.py:148-180).  Threshold 1.0: a dense model's last
# column of 2 ties the labels that score 1.  A label map's row holds one 1, which no threshold of 1.0 ties: there 0.0 as well --
# where the last label is the hot one the clamped row is all zeros, and the first index (0) must win over the clamped column.
ArgmaxCase = collections.namedtuple('ArgmaxCase', 'case threshold')
_ARGMAX_PICK = ((33, 'dense', 'int'), (65, 'dense', 'int'), (75, 'dense', 'default'), (97, 'dense', 'int'), (131, 'dense', 'default'),
                (192, 'dense', 'int'), (256, 'dense', 'default'),                      # one to four 64-column chunks per lane
                (33, 'labelmap', 'int'), (34, 'labelmap', 'int'), (66, 'labelmap', 'int'), (129, 'labelmap', 'int'))
ARGMAX_CASES = tuple(ArgmaxCase(c, thr) for c in CASES if c.L == 64 and (c.K != 75 or c.S == 104) and (c.K, c.o_kind, c.tr_kind) in _ARGMAX_PICK
                     for thr in ((1.0,) if c.o_kind == 'dense' else (1.0, 0.0)))

ArgmaxReference = collections.namedtuple('ArgmaxReference', 'scores want flat threshold_ties')


def argmax_case_id(a):
    return 'C{}-S{}-{}-thr{}'.format(a.case.K - 2, a.case.S, a.case.o_kind, a.threshold)


@functools.lru_cache(maxsize=None)
def argmax_reference(a):
    """the oracle's non-CRF decode of a planted model at every position, and the number of valid positions where the clamped last
    column equals the row's maximum AND a label in front of it does too (the label must win)"""
    r = reference(a.case)
    want = fo.decode_argmax(r.scores, a.threshold, a.case.o_idx)
    s = np.array(r.scores, F32, copy=True)
    s[..., -1] = np.minimum(s[..., -1], F32(a.threshold))
    top = s.max(-1)
    ties = (s[..., -1] == top) & ((s[..., :-1] == top[..., None]).any(-1)) & r.mask
    return ArgmaxReference(r.scores, _freeze(want), _freeze(fo.forward_local_tags(r.scores, r.lengths, a.threshold, a.case.o_idx)),
                           int(ties.sum()))
