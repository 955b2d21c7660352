"""Cases for the tagging path of the two dense onehot layouts (plain numpy, no GPU): FARNN_S_O (--independent 0, `fst4`) and
FARNN_S_O_I (--independent 1 / 2, `ind1`) -- the chain kernel on the label-summed tensor and K3, fst4_score_kernel<NCH>
(csrc/fst4_score.hip.h), on SIGNED weights and at the sizes where launch_fst4_score changes what a lane does.

Two generators:
    signed  non-zero entries with density about 2.5 / S per row (spread over the C label slices of the 4-D tensor), uniform in
            [-0.5, 1.0); h0, hT in [0.1, 1.0); density 1 for S <= 4 (the sparse draw is all-zero there).  The relu inside the 4-D
            sum (model_onehot.py:119-121) and the relu of both recurrences bite.  Compared by tests/util.py: assert_float_path.
    exact   every value from {-1, -0.5, 0, 0.5, 1, 2}: every sum is exact in float32 whatever its order (exact_bits proves it
            for a case), so the kernels must EQUAL the float32 oracle.
V is 5..7 words, the last one the pad.  Planted ties (exact models only): the label slice of column c2 is a copy of c1's, c1's
dominates every other column, and the first index must win; and one model per layout where a column scores exactly the threshold
0.5 while the last column exceeds it.

A mutant is the oracle's scoring step with one planted error (score_step(..., mutant=)): 'a' the clip after the sum, 'b'
alpha_{i+1} for alpha_i, 'c' beta one row off, 'd' W4 / W left out.  tests/test_fst4_tag_cases_cpu.py holds every case to: each
mutant FAILS the case's comparator.  A case that cannot tell one from the oracle was redrawn (SEED_BUMP), never excused, except
EXEMPT: S <= 4 at density 1 or L = 1.
"""
import collections
import functools
import json
import os
import zlib

import numpy as np

from oracle import farnn_oracle as fo
from util import assert_float_path

TOL = 1e-4                                                 # assert_float_path's default: the project's stated bar
THRESHOLD = 0.5
EXACT_VALUES = (-1.0, -0.5, 0.0, 0.5, 1.0, 2.0)
MUTANTS = ('a', 'b', 'c', 'd')

Case = collections.namedtuple('Case', 'layout kind S C V B L lengths semiring prio mask tie seed edge')


def case_id(c):
    s = '{}-{}-S{}-C{}-B{}-L{}-{}-p{}'.format(c.layout, c.kind, c.S, c.C, c.B, c.L, 'max' if c.semiring else 'sum', c.prio)
    if c.layout == 'ind1':
        s += '-m{}'.format(int(c.mask))
    if not any(c.lengths):
        s += '-len0'
    if c.tie is not None:
        s += '-tie' + ('thr' if c.tie == 'threshold' else '{}.{}'.format(*c.tie))
    return s


def o_idx(c):
    return c.C + 1                                          # no column's index: a mapped last column is told from every label


# ------------------------------------------------------------------------------------------------ the launcher, restated
def round_up(a, b):
    return (a + b - 1) // b * b


K3Geometry = collections.namedtuple('K3Geometry', 'SP CPR LPR G NCH idle')


def k3_geometry(S):
    """launch_fst4_score (csrc/fst4_score.hip.h): a lane owns a 16-byte column chunk; CPR chunks per row; G rows per wavefront pass
    where a row fits 64 lanes, else NCH chunks per lane (instantiated: 1, 2, 4); `idle` lanes at the wavefront's end"""
    SP = round_up(S, 4)
    CPR = SP // 4
    if CPR <= 64:
        LPR, G, NCH = CPR, 64 // CPR, 1
    else:
        LPR, G, NCH = 64, 1, {2: 2, 3: 4, 4: 4}[(CPR + 63) // 64]
    return K3Geometry(SP, CPR, LPR, G, NCH, 64 - G * LPR)


def k3_lds_bytes(S, C, ind1):
    """the launcher's lds = (SP + 2 Kp + S SP) 4, the last term for independent=1 only; farnn_tag passes the label columns
    rounded up to 64 as Kp"""
    SP, Kp = round_up(S, 4), round_up(C, 64)
    return (SP + 2 * Kp + (S * SP if ind1 else 0)) * 4


LDS_ATTRIBUTE, LDS_LIMIT = 48 * 1024, 160 * 1024            # above the first: hipFuncSetAttribute; above the second: refused


def largest_S_within(limit, C):
    S = 1
    while k3_lds_bytes(S + 1, C, True) <= limit:
        S += 1
    return S


def chain_form(S):
    """the recurrence in front of K3 (launch_chain, csrc/farnn_hip.hip), by its documented ranges"""
    return 'chain: register-fed' if S <= 72 else 'chain: register-fed wide' if S <= 128 else 'chain: LDS ring'


# ------------------------------------------------------------------------------------------------ models
def _signed(rng, shape, p):
    return ((rng.rand(*shape) < p) * (rng.rand(*shape) * 1.5 - 0.5)).astype(np.float32)


def _exact(rng, shape, p, values=(1.0, -1.0, 0.5, -0.5, 2.0), weights=(0.5, 0.25, 0.1, 0.07, 0.08)):
    return ((rng.rand(*shape) < p) * rng.choice(values, size=shape, p=weights)).astype(np.float32)


def _density(S):
    return 1.0 if S <= 4 else min(1.0, 2.5 / S)


def _priority(c, rng):
    """a non-identity signed corner (priority.py:6-18: expand_priority); None without"""
    if not c.prio:
        return None
    n = min(c.C, 3)
    if c.kind == 'exact':
        pm = rng.choice([-0.5, 0.0, 0.5, 1.0, -1.0], size=(n, n), p=[0.15, 0.3, 0.2, 0.25, 0.1]) + np.eye(n)
        pm[pm == 1.5] = 2.0
    else:
        pm = rng.rand(n, n) * 1.5 - 0.5 + np.eye(n)
    return fo.expand_priority(c.C, pm)


def model(c):
    """fst4: (T4 [V,C,S,S], W4 [C,S,S], h0, hT);  ind1: (T [V,S,S], W [S,S], Oten [C,S,S], h0, hT);  and P [C,C] or None"""
    rng = np.random.RandomState(c.seed)
    S, C, V = c.S, c.C, c.V
    d = _density(S)
    if c.kind == 'signed':
        h0, hT = ((rng.rand(S) * 0.9 + 0.1).astype(np.float32) for _ in range(2))
        if c.layout == 'fst4':
            ps = d if S <= 4 else d / C
            m = (_signed(rng, (V, C, S, S), ps), _signed(rng, (C, S, S), ps if S <= 4 else ps * 0.5), h0, hT)
        else:
            m = (_signed(rng, (V, S, S), d), _signed(rng, (S, S), d if S <= 4 else d * 0.5), _signed(rng, (C, S, S), min(0.3, 2.0 / C)), h0, hT)
    else:
        # sparser than the signed draw and few start states: exact_bits() allows 24 mantissa bits over L + 3 factors
        h0 = np.zeros(S, np.float32); h0[rng.permutation(S)[:min(S, 3)]] = rng.choice([0.5, 1.0, 2.0], size=min(S, 3))
        hT = rng.choice([0.0, 0.5, 1.0], size=S, p=[0.3, 0.3, 0.4]).astype(np.float32); hT[rng.randint(S)] = 1.0
        de = min(1.0, 1.8 / S) / (3 if isinstance(c.tie, tuple) else 1)          # (a tie's c1 and c2 carry every slice's entries)
        pos = (1.0, 0.5, 2.0), (0.6, 0.2, 0.2)
        if c.layout == 'fst4':
            ps = de / C
            T4, W4 = _exact(rng, (V, C, S, S), ps), _exact(rng, (C, S, S), ps * 0.5 if S > 1 else ps)
            if isinstance(c.tie, tuple):                   # c1 dominates: max_c |A[., c]| entry by entry; c2 copies it
                c1, c2 = c.tie
                T4[:, c1] = np.abs(T4).max(1); W4[c1] = np.abs(W4).max(0)
                T4[:, c2] = T4[:, c1]; W4[c2] = W4[c1]
            m = (T4, W4, h0, hT)
        else:
            tied = isinstance(c.tie, tuple)                # (no relu in this layout's score: non-negative T, W keep c1 dominant)
            T = _exact(rng, (V, S, S), de, *(pos if tied else ()))
            W = _exact(rng, (S, S), de * 0.5 if S > 1 else de, *(pos if tied else ()))
            O = _exact(rng, (C, S, S), min(0.3, 2.0 / C))
            if tied:
                c1, c2 = c.tie
                O[c1] = np.abs(O).max(0); O[c2] = O[c1]
            m = (T, W, O, h0, hT)
    return m, _priority(c, rng)


def batch(c):
    rng = np.random.RandomState(c.seed + 1)
    lengths = np.asarray(c.lengths, np.int64)
    x = np.full((c.B, c.L), c.V - 1, np.int64)
    for b, n in enumerate(lengths):
        x[b, :n] = rng.randint(0, c.V, size=int(n))
    return x, lengths


# ------------------------------------------------------------------------------------------------ the oracle, and its scoring step apart
def oracle_scores(c, m, P, x, lengths, dtype=np.float32):
    m = tuple(a.astype(dtype) for a in m)
    P = None if P is None else P.astype(dtype)
    with fo.precision(dtype):
        if c.layout == 'fst4':
            return fo.onehot_fst4_scores(*m, x, lengths, semiring=c.semiring, P=P)
        return fo.onehot_ind1_scores(*m, x, lengths, semiring=c.semiring, P=P, mask_by_output=c.mask)


def chains(c, m, x, lengths, dtype=np.float32):
    """(fw, rb): both recurrences of the oracle (model_onehot.py:88-110 / :255-285), fw[:, i] the state BEFORE token i"""
    m = tuple(a.astype(dtype) for a in m)
    with fo.precision(dtype):
        if c.layout == 'fst4':
            T4, W4, h0, hT = m
            Ts = T4.sum(1) + W4.sum(0)
        else:
            T, W, O, h0, hT = m
            Ts = (T + W) * O.sum(0) if c.mask else T + W
        B, L = x.shape
        xb = fo.reverse_prefix(x, lengths)
        hf = np.repeat(h0[None], B, 0); hb = np.repeat(hT[None], B, 0)
        fw = np.zeros((B, L + 1, c.S), dtype); fw[:, 0] = h0
        bw = np.zeros((B, L + 1, c.S), dtype); bw[:, 0] = hT
        for i in range(L):
            hf = np.maximum(fo.semiring_vm(hf, Ts[x[:, i]], c.semiring), dtype(0)); fw[:, i + 1] = hf
            hb = np.maximum(fo.semiring_vm(hb, Ts[xb[:, i]].transpose(0, 2, 1), c.semiring), dtype(0)); bw[:, i + 1] = hb
        return fw, fo.reverse_prefix(bw, np.asarray(lengths) + 1)


def score_step(c, m, P, fw, rb, x, mutant=None, dtype=np.float32, terms=None):
    """the oracle's scoring step (model_onehot.py:115-127 / :229-233) on given chains; mutant: one planted error.
    terms: a list that receives every A a b term of the 4-D sum (for the share of negative ones)"""
    m = tuple(a.astype(dtype) for a in m)
    P = None if P is None else P.astype(dtype)
    B, L = x.shape
    out = np.zeros((B, L, c.C), dtype)
    with fo.precision(dtype):
        for i in range(L):
            al = fw[:, i + 1] if mutant == 'b' else fw[:, i]
            be = rb[:, i] if mutant == 'c' else rb[:, i + 1]
            if c.layout == 'fst4':
                T4, W4 = m[0], m[1]
                A = T4 if mutant == 'd' else T4 + W4
                tmp = A[x[:, i]] * al[:, None, :, None]
                tmp = tmp * be[:, None, None, :]
                if terms is not None:
                    terms.append(tmp)
                sc = np.maximum(tmp.sum(axis=(2, 3)), dtype(0)) if mutant == 'a' else np.maximum(tmp, dtype(0)).sum(axis=(2, 3))
                sc = sc.astype(dtype)
            else:
                T, W, O = m[0], m[1], m[2]
                Tf = T if mutant == 'd' else T + W
                abt = (al[:, :, None] * be[:, None, :]) * Tf[x[:, i]]
                sc = np.einsum('csj,bsj->bc', O, abt).astype(dtype)
            out[:, i] = sc if P is None else fo.priority(sc, P)
    return out


def _bits(terms, axes):
    """log2 of (sum |t|) / (the largest power of two dividing every t), the worst over the reductions along `axes` of a float64
    array of terms: the mantissa bits the widest partial sum of such a reduction can need, in any order"""
    t = np.abs(np.asarray(terms, np.float64))
    mant, e = np.frexp(t)
    mi = np.round(mant * 2.0 ** 53).astype(np.int64)
    low = np.where(mi > 0, np.log2(np.maximum(mi & -mi, 1).astype(np.float64)) + e - 53, np.inf)      # exponent of the lowest set bit
    tot, g = t.sum(axis=axes), low.min(axis=axes)
    live = tot > 0
    return float((np.log2(tot[live]) - g[live]).max()) if live.any() else 0.0


def exact_bits(c, m, P, x, lengths):
    """An exact model's proof: every reduction of the oracle (the label sum of the blocks, every recurrence step, the scoring sum,
    the priority product) re-evaluated in float64 with its terms kept; the widest partial sum any order of any of them can form,
    in mantissa bits.  At or below 24 every float32 sum on either side is exact.  (The max semiring's recurrence forms no sums: its
    terms are judged one by one.)"""
    f = np.float64
    m = tuple(a.astype(f) for a in m)
    worst = 0.0
    if c.layout == 'fst4':
        T4, W4, h0, hT = m
        worst = max(worst, _bits(np.concatenate([T4, np.broadcast_to(W4, T4.shape)], 1), 1))
        Ts = T4.sum(1) + W4.sum(0)
    else:
        T, W, O, h0, hT = m
        worst = max(worst, _bits(O, 0), _bits(np.stack([T, np.broadcast_to(W, T.shape)]), 0))
        Ts = (T + W) * O.sum(0) if c.mask else T + W
        worst = max(worst, _bits(Ts[None], 0))
    B, L = x.shape
    xb = fo.reverse_prefix(x, lengths)
    hf = np.repeat(h0[None], B, 0); hb = np.repeat(hT[None], B, 0)
    axes = 1 if c.semiring == fo.SEMIRING_SUM else ()
    with fo.precision(f):
        for i in range(L):
            tf = hf[:, :, None] * Ts[x[:, i]]
            tb = hb[:, :, None] * Ts[xb[:, i]].transpose(0, 2, 1)
            worst = max(worst, _bits(tf, axes) if axes != () else _bits(tf[None], 0), _bits(tb, axes) if axes != () else _bits(tb[None], 0))
            hf = np.maximum(fo.semiring_vm(hf, Ts[x[:, i]], c.semiring), 0.0)
            hb = np.maximum(fo.semiring_vm(hb, Ts[xb[:, i]].transpose(0, 2, 1), c.semiring), 0.0)
    fw, rb = chains(c, m, x, lengths, f)
    for i in range(L):
        al, be = fw[:, i], rb[:, i + 1]
        if c.layout == 'fst4':
            t = (T4 + W4)[x[:, i]] * al[:, None, :, None] * be[:, None, None, :]
            worst = max(worst, _bits(t, (2, 3)))
            sc = np.maximum(t, 0.0).sum(axis=(2, 3))
        else:
            z = (al[:, :, None] * be[:, None, :]) * (T + W)[x[:, i]]
            t = O[None] * z[:, None]
            worst = max(worst, _bits(t, (2, 3)))
            sc = t.sum(axis=(2, 3))
        if P is not None:
            worst = max(worst, _bits(sc[:, :, None] * P.astype(f)[None], 1))
    return worst


def clamped(scores, threshold=THRESHOLD):
    s = np.array(scores, copy=True)
    s[..., -1] = np.minimum(s[..., -1], s.dtype.type(threshold))
    return s


def decode_last_index(scores, c):
    """fo.decode_argmax taking the LAST maximal index: a wrong decode of the kind a kernel could fall into"""
    s = clamped(np.asarray(scores, np.float32))
    pred = (c.C - 1 - s[..., ::-1].argmax(-1)).astype(np.int64)
    pred[pred == c.C - 1] = o_idx(c)
    return pred


Reference = collections.namedtuple('Reference', 'model P x lengths mask ref32 ref64 want want64 flat near band near_share')


def _freeze(a):
    if a is not None:
        a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=6)
def reference(c):
    """Everything the oracle says about a case, read-only: float32 and float64 scores [B, L, C] (all L positions, as forward_score),
    the decode of either, the flat tags, and the near-tied positions: top two clamped float64 scores within 2 tol (1 + |top|);
    band[b, i, k]: column k lies inside that band."""
    m, P = model(c)
    x, lengths = batch(c)
    ref32 = oracle_scores(c, m, P, x, lengths)
    ref64 = oracle_scores(c, m, P, x, lengths, np.float64)
    mask = np.arange(c.L)[None, :] < lengths[:, None]
    want = fo.decode_argmax(ref32, THRESHOLD, o_idx(c))
    with fo.precision(np.float64):
        want64 = fo.decode_argmax(ref64, THRESHOLD, o_idx(c))
    s = clamped(ref64)
    top = np.sort(s, -1)
    width = 2 * TOL * (1 + np.abs(top[..., -1]))
    near = top[..., -1] - top[..., -2] <= width
    band = s >= (top[..., -1] - width)[..., None]
    share = float(near[mask].mean()) if mask.any() else 0.0
    return Reference(tuple(_freeze(a) for a in m), _freeze(P), _freeze(x), _freeze(lengths), _freeze(mask), _freeze(ref32), _freeze(ref64),
                     _freeze(want), _freeze(want64), _freeze(fo.flatten(want, lengths)), _freeze(near), _freeze(band), share)


def mismatch(c, got, r):
    """None where `got` [B, L, C] passes the case's comparator, else what it said"""
    if c.kind == 'exact':
        return None if np.array_equal(got, r.ref32) else 'differs from the float32 oracle'
    try:
        assert_float_path(got, r.ref32, r.ref64, TOL)
    except AssertionError as e:
        return str(e)
    return None


def tags_allowed(c, r, tags, where):
    """signed cases: `tags` equal the float64 decode wherever the position is not near-tied, and name a column inside the band
    where it is (the last column as o_idx).  `where`: bool [B, L], the positions to judge."""
    col = np.where(tags == o_idx(c), c.C - 1, tags)
    ok = (col >= 0) & (col < c.C)
    inband = np.zeros(tags.shape, bool)
    inband[ok] = np.take_along_axis(r.band, np.clip(col, 0, c.C - 1)[..., None], -1)[..., 0][ok]
    good = np.where(r.near, inband, tags == r.want64)
    return bool(good[where].all())


def tied_threshold_positions(r):
    """valid positions where a label scores exactly the threshold, the last column exceeds it, and nothing else reaches it"""
    s = r.ref32
    lab = s[..., :-1]
    return (lab.max(-1) == np.float32(THRESHOLD)) & (s[..., -1] > np.float32(THRESHOLD)) & r.mask


def unmet(c, r=None):
    """The conditions on the INPUTS of one case, from the references alone: the ones it misses (tests/test_fst4_tag_cases_cpu.py)."""
    r = r or reference(c)
    out = []
    m, P, x, lengths = r.model, r.P, r.x, r.lengths
    fw, rb = chains(c, m, x, lengths)
    if not np.array_equal(score_step(c, m, P, fw, rb, x), r.ref32):
        out.append('score_step restates another scoring step than the oracle\'s')
    if c.kind == 'signed':
        e = np.abs(r.ref32.astype(np.float64) - r.ref64) / (1 + np.abs(r.ref64))
        if e.max() > TOL / 10:
            out.append('float32 oracle {:.2e} from float64, bar {:.0e}'.format(e.max(), TOL / 10))
        if r.mask.any() and not (np.abs(r.ref64[r.mask]).max(-1) > 0).all():
            out.append('a valid position with an all-zero score row')
        if r.near_share > 0.10:
            out.append('near-tied share {:.3f} above 0.10'.format(r.near_share))
        if c.layout == 'fst4':
            terms = []
            fw64, rb64 = chains(c, m, x, lengths, np.float64)
            score_step(c, m, None, fw64, rb64, x, dtype=np.float64, terms=terms)
            t = np.concatenate([a.ravel() for a in terms])
            nz = t != 0
            if not nz.any() or (t[nz] < 0).mean() < 0.20:
                out.append('negative share of the non-zero terms {:.3f} below 0.20'.format((t[nz] < 0).mean() if nz.any() else 0.0))
    else:
        bits = exact_bits(c, m, P, x, lengths)
        if bits > 24:
            out.append('an exact sum may need {:.1f} mantissa bits, above 24'.format(bits))
        if not np.array_equal(r.ref32.astype(np.float64), r.ref64):
            out.append('the float32 oracle is not the float64 oracle')
    for mu in MUTANTS:
        if mu == 'a' and not (c.kind == 'signed' and c.layout == 'fst4'):
            continue
        if (case_id(c), mu) in EXEMPT:
            continue
        if mismatch(c, score_step(c, m, P, fw, rb, x, mutant=mu), r) is None:
            out.append('mutant ({}) passes'.format(mu))
    if isinstance(c.tie, tuple):
        c1, c2 = c.tie
        if not np.array_equal(r.ref32[..., c1], r.ref32[..., c2]):
            out.append('the planted columns are not bit-equal')
        d = (decode_last_index(r.ref32, c) != r.want)[r.mask]
        won = (r.want == c1)[r.mask]
        if 2 * d.sum() < d.size or 2 * won.sum() < won.size:
            out.append('last-index decode differs at {} of {} valid positions, c1 wins {}'.format(int(d.sum()), d.size, int(won.sum())))
    if c.tie == 'threshold':
        n = int(tied_threshold_positions(r).sum())
        if n < 1:
            out.append('no position tied at the threshold')
    return out


# ------------------------------------------------------------------------------------------------ the grid
SUM, MAX = fo.SEMIRING_SUM, fo.SEMIRING_MAX

# S for both layouts (independent=1: up to 132) -> the edge it is
S_EDGES = collections.OrderedDict([
    (1, 'CPR 1, G 64: one lane per row'), (4, 'CPR 1: SP = S'), (5, 'CPR 2, G 32: SP = S + 3'), (8, 'CPR 2: SP = S'),
    (9, 'CPR 3, G 21: one idle lane'), (12, 'CPR 3, G 21: one idle lane, SP = S'),
    (17, 'CPR 5, G 12: four idle lanes'), (20, 'CPR 5, G 12: four idle lanes, SP = S'),
    (61, 'CPR 16, G 4'), (64, 'CPR 16, G 4: SP = S'), (65, 'CPR 17, G 3: thirteen idle lanes'), (68, 'CPR 17, G 3: thirteen idle lanes, SP = S'),
    (71, 'the chain\'s narrow form, shipped size'), (72, 'the chain\'s last narrow size'), (73, 'the chain\'s first wide size'),
    (127, 'CPR 32, G 2; wide chain'), (128, 'CPR 32, G 2; the wide chain\'s last size'), (129, 'CPR 33, G 1; the LDS-ring chain\'s first size'),
    (132, 'CPR 33, G 1: SP = S'),
    (256, 'CPR 64, NCH 1: the last size with one chunk per lane'), (257, 'CPR 65: NCH 2'),
    (512, 'CPR 128: the last NCH 2'), (513, 'CPR 129: NCH 3 runs as fst4_score_kernel<4>'),
])
IND1_S_MAX = 132
C_EDGES = collections.OrderedDict([
    (2, 'two columns: one label and the clamped one'), (3, 'fewer columns than wavefronts'), (4, 'one column per wavefront'),
    (5, 'a second column for wavefront 0'), (64, 'decode: one pass, every lane'), (65, 'decode: a second pass for lane 0'),
    (129, 'decode: a third pass, Kp 192'), (256, 'decode: four passes, Kp 256'), (257, 'Kp 320'), (300, 'Kp 320, five passes'),
])
C_AT_S = (5, 71)
TIE_PAIRS = ((3, 67), (0, 64), (63, 64), (1, 130), (2, 258))   # same lane; lanes 0 / 0 across passes; lanes 63 / 0; 1 / 2; 2 / 2 (C >= 260)

# Draws that missed a condition of unmet() were redrawn with a later seed: case id -> how many seeds further; and the (case id,
# mutant) pairs that a case cannot tell from the oracle BY CONSTRUCTION: S = 1, where a sum has one term (the clip after the sum IS
# the clip per term) and a state that stays put makes alpha_{i+1} = alpha_i.  tests/golden/fst4_tag_seeds.json: recorded results.
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fst4_tag_seeds.json')) as _f:
    _SEEDS = json.load(_f)
SEED_BUMP = _SEEDS['seed_bump']
EXEMPT = frozenset((a, b) for a, b in _SEEDS['exempt'])


def _lengths(B, L, seed):
    """1, L, 0 and one drawn length in every batch of four; smaller batches: L first"""
    rng = np.random.RandomState(seed)
    if B == 1:
        return (L,)
    if B == 2:
        return (L, max(1, L // 2))
    if B == 3:
        return (max(1, L // 2), L, 1)
    if B == 4:
        return (1, L, 0, int(rng.randint(2, L)) if L > 2 else L)
    ls = rng.randint(0, L + 1, size=B)
    ls[0], ls[1], ls[-1] = L, 0, 1
    return tuple(int(v) for v in ls)


def _mk(layout, kind, S, C, semiring, prio, mask=False, V=6, B=4, L=9, lengths=None, tie=None, edge='', seed=None):
    lengths = tuple(lengths) if lengths is not None else _lengths(B, L, 31 * S + C)
    c = Case(layout, kind, S, C, V, B, L, lengths, semiring, prio, bool(mask), tie, 0, edge)
    cid = case_id(c)
    return c._replace(seed=(zlib.crc32(cid.encode()) % (2 ** 30) if seed is None else seed) + SEED_BUMP.get(cid, 0))


def _variants(layout, kind, i):
    """(semiring, prio, mask): signed cases take the whole cross; exact cases two opposite corners of it, alternating"""
    masks = (False, True) if layout == 'ind1' else (False,)
    if kind == 'signed':
        return [(s, p, m) for s in (SUM, MAX) for p in (0, 1) for m in masks]
    pair = [(SUM, 0), (MAX, 1)] if i % 2 == 0 else [(SUM, 1), (MAX, 0)]
    return [(s, p, masks[(i + j) % len(masks)]) for j, (s, p) in enumerate(pair)]


def _shape_kw(S):
    # S = 513: about 11 MB of blocks at V = 5, C = 2, and an oracle that finishes in seconds
    return dict(V=5, C=2, B=2, L=3, lengths=(3, 1)) if S == 513 else dict(C=3)


def _grid():
    cases = []
    for layout in ('fst4', 'ind1'):
        ind1 = layout == 'ind1'
        shapes = []                                          # (S, C, extra kw, edge)
        for S, edge in S_EDGES.items():
            if ind1 and S > IND1_S_MAX:
                continue
            g = k3_geometry(S)
            kw = _shape_kw(S)
            shapes.append((S, kw.pop('C'), kw, 'S: {} [CPR {} G {} NCH {} idle {}; {}]'.format(edge, g.CPR, g.G, g.NCH, g.idle, chain_form(S))))
        if ind1:
            a, b = largest_S_within(LDS_ATTRIBUTE, 3), largest_S_within(LDS_LIMIT, 3)
            shapes.append((a, 3, dict(V=5), 'LDS: the largest S within 48 KiB ({} bytes)'.format(k3_lds_bytes(a, 3, True))))
            shapes.append((a + 1, 3, dict(V=5), 'LDS: the first S above 48 KiB ({} bytes): hipFuncSetAttribute'.format(k3_lds_bytes(a + 1, 3, True))))
            shapes.append((b, 3, dict(V=5), 'LDS: the largest S within 160 KiB ({} bytes)'.format(k3_lds_bytes(b, 3, True))))
        for S in C_AT_S:
            for C, edge in C_EDGES.items():
                if C > 256 and (ind1 or S != 5):
                    continue
                if C != 3:
                    shapes.append((S, C, dict(V=5), 'C: {} [Kp {}]'.format(edge, round_up(C, 64))))
        # batch geometry at S = 5, C = 3
        for kw, edge in ((dict(B=1, L=1), 'B 1, L 1: one workgroup'), (dict(B=2), 'B 2: no launch order'), (dict(B=3), 'B 3: the first sorted batch'),
                         (dict(lengths=(0, 0, 0, 0)), 'every length 0: no valid position'),
                         (dict(B=1100, L=3), 'B 1100: batch_prep_kernel\'s counting sort and flat offsets')):
            shapes.append((5, 3, kw, 'batch: ' + edge))
        for i, (S, C, kw, edge) in enumerate(shapes):
            for kind in ('signed', 'exact'):
                for s, p, m in _variants(layout, kind, i):
                    cases.append(_mk(layout, kind, S, C, s, p, m, edge=edge, **kw))
    assert len({case_id(c) for c in cases}) == len(cases)
    return tuple(cases)


def _tie_grid():
    cases = []
    for layout in ('fst4', 'ind1'):
        for c1, c2 in TIE_PAIRS:
            if c2 == 258 and layout == 'ind1':
                continue
            C = 260 if c2 == 258 else c2 + 2                 # (c2 is never the clamped last column)
            for s in (SUM, MAX):
                cases.append(_mk(layout, 'exact', 5, C, s, 0, False, V=5, tie=(c1, c2), edge='tie: columns {} and {} bit-equal'.format(c1, c2)))
        for s in (SUM, MAX):
            cases.append(_mk(layout, 'exact', 5, 3, s, 0, False, V=7, B=4, L=9, lengths=(9, 9, 7, 9), tie='threshold',
                             edge='tie: a label at the threshold against the clamped last column'))
    assert len({case_id(c) for c in cases}) == len(cases)
    return tuple(cases)


CASES = _grid()
TIE_CASES = _tie_grid()
# the chain forms in front of K3, each under the default dispatch and under FARNN_NOREGS=1 (the LDS-ring kernel at every S)
CHAIN_CASES = tuple(_mk(layout, kind, S, 3, s, 0, layout == 'ind1' and S == 104, edge='chain form: ' + chain_form(S))
                    for layout in ('fst4', 'ind1') for S in (71, 104, 130) for kind, s in (('signed', SUM), ('signed', MAX), ('exact', SUM)))
# one handle, varying shapes: the same model (one seed) under four batches; the stash stride changes with L
VARYING_SHAPES = ((4, 9), (2, 3), (7, 12), (4, 9))
VARYING_CASES = tuple(tuple(_mk(layout, 'signed', 17, 5, SUM, 1, False, B=B, L=L, seed=1717, edge='one handle: B {} L {}'.format(B, L))
                            for B, L in VARYING_SHAPES) for layout in ('fst4', 'ind1'))
ALL_CASES = CASES + TIE_CASES + tuple(c for c in CHAIN_CASES if c not in CASES) + tuple(c for cs in VARYING_CASES for c in cs[:3])


def refused_ind1_S(C=3):
    """the first S whose independent=1 scoring does not fit 160 KiB: refused at create"""
    return largest_S_within(LDS_LIMIT, C) + 1
