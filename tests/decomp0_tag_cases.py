"""Cases for the tagging path of the decomposed FST (FARNN_S_D_W, --independent 0, farnn_decomp_fst_create; plain numpy / torch
on the CPU, no GPU): the recurrence on Vgen * sum_c C and S1w diag(sum_c Cw) S2w^T + WW, then decomp0_score_kernel
(csrc/decomp1_score.hip.h) on the UNSCALED Vgen, at the sizes where that kernel changes what a thread does.

References.  Sum semiring: tests/decomp0_train_ref.py: forward in float32 and float64 is the (ref32, ref64) pair, its check_gap
the gap rule (the float32 and the float64 decode agree, no relu pre-activation sits at 0); oracle/farnn_oracle.py:
decomp_fst_scores in float64 is a second restatement, written apart.  Max semiring: fo.decomp_fst_scores and its float64
evaluation are the pair, and max_gap() applies the decode half of the gap rule to them.

The draw starts from decomp0_train_ref.signed_base and changes it where that generator fails at these shapes:
    zeros of a factor are refilled along a dimension of four or fewer (S = R = RW = 1 drew an all-zero score row);
    C_embed / C_wildcard are dense and drawn from 160 values, so that at K = 256 columns lie apart;
    the recurrence is scaled until its float64 states keep their length over the batch's L steps (_normalise: signed_base's mean
    absolute row sum in [1, 2) let `none` run to 1e4 over 17 steps and S = 129 die within three);
    the scores are brought to [4, 8) almost WITHOUT touching the recurrence, which sees the label factors through their column
    sums only: C <- s C - (s - 1) colsum(C) / K, rounded to 1 / 256, keeps every column sum to within K / 512;
    the clamped column (K - 1, under the CRF K - 3) is made 1.25 times the column that wins most often, so that the clamp decides
    positions (mutant f);
    tie cases take |.| of every factor and the elementwise maximum of all label rows as row c1, copied to c2: every term of every
    score is non-negative, so c1 and c2 dominate every position.
A draw that misses a condition of unmet() is redrawn with a later seed (tests/golden/decomp0_tag_seeds.json records how many
seeds further; `PYTHONPATH=. python tests/decomp0_tag_cases.py` searches them again), never excused.

A mutant is the scoring step with one planted error (score_step(..., mutant=)): 'a' the state after token i for the state before
it, 'b' the backward row one off, 'c' the wildcard term left out, 'd' the recurrence's table Vgen * csum for Vgen, 'e' the columns
R - R % 4 .. R - 1 of the language term (and likewise of RW) left out, 'f' the clamp on column K - 1 under the CRF in place of
K - 3, and no clamp without it.  The only exemptions are by construction (exemption_allowed): 'b' at L = 1, 'e' where R and RW
are multiples of 4 (it is then no error at all), 'a' at S = 1 where a state that stays put makes it invisible.
"""
import collections
import functools
import json
import os
import zlib

import numpy as np
import torch

import decomp0_train_ref as d0r
from oracle import farnn_oracle as fo
from util import assert_float_path, in_float64

TOL = 1e-4                                                 # assert_float_path's default: the project's stated bar
THRESHOLD = 0.5
SIG_K = 5.0
MUTANTS = ('a', 'b', 'c', 'd', 'e', 'f')
SUM, MAX = fo.SEMIRING_SUM, fo.SEMIRING_MAX
LOCAL, FULL = 'local', 'full'
GATES = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')

Case = collections.namedtuple('Case', 'S R RW K V B L lengths nl farnn semiring prio crf mode seed edge tie')


def case_id(c):
    s = 'S{}-R{}-Q{}-K{}-B{}-L{}-{}-f{}-{}-p{}-crf{}-{}'.format(c.S, c.R, c.RW, c.K, c.B, c.L, c.nl, c.farnn, 'max' if c.semiring else 'sum',
                                                              c.prio, c.crf, c.mode)
    if not any(c.lengths):
        s += '-len0'
    if c.tie is not None:
        s += '-tie{}.{}'.format(*c.tie)
    return s


def o_idx(c):
    return c.K + 1                                          # no column's index: a mapped last column is told from every label


def clamp_col(c):
    return c.K - 3 if c.crf else c.K - 1


# ------------------------------------------------------------------------------------------------ the launcher, restated
def round_up(a, b):
    return (a + b - 1) // b * b


D0_TOK = 8
D0_STATIC_LDS = 4 * D0_TOK                                  # tokid[]: static LDS beside the dynamic tile, inside the same 160 KiB
LDS_ATTRIBUTE, LDS_LIMIT = 48 * 1024, 160 * 1024            # above the first: hipFuncSetAttribute; above the second: refused
K_MAX, R_MAX = 256, 4096                                    # farnn_decomp_fst_create refuses more label columns / a higher rank

D0Geometry = collections.namedtuple('D0Geometry', 'SP Rp RWp Kc lds wgs col_passes label_passes decode_passes')


def d0_geometry(S, R, RW, K, L):
    """launch_decomp0_score (csrc/farnn_hip.hip) and decomp0_score_lds_bytes: LDS = 8 (2 SP + Rp + RWp + 2 Kc) floats, ceil(L / 8)
    workgroups per sequence; the 128-lane column loop runs over R + RW, the label loop over K, the decode in passes of 64"""
    SP, Rp, RWp, Kc = round_up(S, 4), round_up(R, 4), round_up(RW, 4), round_up(K, 64)
    return D0Geometry(SP, Rp, RWp, Kc, D0_TOK * (2 * SP + Rp + RWp + 2 * Kc) * 4, (L + D0_TOK - 1) // D0_TOK,
                      (R + RW + 127) // 128, (K + 127) // 128, (K + 63) // 64)


def lds_shapes(S=4, K=3):
    """(R, RW) of the largest shape within 48 KiB, the first above it, the largest within 160 KiB and the first refused, at the
    smallest S with SP = S: by the rank, and by the wildcard rank once R is at the create's limit"""
    out = []
    for limit in (LDS_ATTRIBUTE, LDS_LIMIT - D0_STATIC_LDS):          # (the attribute step is taken by the dynamic bytes alone)
        units = (limit // (4 * D0_TOK) - 2 * round_up(S, 4) - 2 * round_up(K, 64)) // 4 * 4       # what is left for Rp + RWp
        R = min(R_MAX, units - 4)
        RW = units - R
        out += [(R, RW), (R + 1, RW) if R < R_MAX else (R, RW + 1)]
    return out


def chain_form(c):
    """the recurrence in front of the score kernel (plan_decomp_recurrence, csrc/farnn_hip.hip), by its documented ranges"""
    if c.semiring == MAX:
        return 'decomp_chain_kernel'
    return 'decomp_regs_kernel (rank <= 64, farnn 0) / decomp_rows_kernel'


# ------------------------------------------------------------------------------------------------ the draw
_VALS = np.array([-1.0, -0.5, -0.25, 0.25, 0.5, 0.75, 1.0, 1.25], np.float32)
_CVALS = np.array([v / 64.0 for v in range(-64, 97) if v], np.float32)         # 160 values in [-1, 1.5], none of them 0


def _refill(a, rng):
    z = a == 0
    a[z] = rng.choice(_VALS, size=int(z.sum()))


def _fo_params(c, p):
    q = {'Vgen': p['Vgen'], 'C': p['C_embed'], 'S1': p['S1'], 'S2': p['S2'], 'Cw': p['C_wildcard'], 'S1w': p['S1_wildcard'],
         'S2w': p['S2_wildcard'], 'WW': p['wildcard_wildcard'], 'h0': p['h0'], 'hT': p['hT'], 'farnn': c.farnn, 'nl': fo.NL_CODES[c.nl],
         'semiring': c.semiring, 'sig_k': SIG_K}
    q.update({g: p[g] for g in GATES if g in p})
    return q


def _pad_L(a, L):
    out = np.zeros((a.shape[0], L, a.shape[2]), a.dtype)
    out[:, :a.shape[1]] = a
    return out


def oracle_scores(c, p, P, x, lengths, wide=False):
    """fo.decomp_fst_scores [B, L, K] (zero rows behind the longest sequence, where the oracle stops)"""
    q = _fo_params(c, p)
    sc = in_float64(fo.decomp_fst_scores, q, x, lengths, P=P) if wide else fo.decomp_fst_scores(q, x, lengths, P=P)
    return _pad_L(sc, c.L)


def restated_scores(c, p, P, x, lengths, dtype):
    """d0r.forward's scores [B, L, K] as numpy (sum semiring)"""
    with torch.no_grad():
        sc = d0r.forward(d0r._params(p, dtype), None if P is None else d0r._t(P, dtype), x, lengths, nl=c.nl, farnn=c.farnn, k=SIG_K)[0]
    return sc.numpy()


def reference_pair(c, p, P, x, lengths):
    if c.semiring == MAX:
        return oracle_scores(c, p, P, x, lengths), oracle_scores(c, p, P, x, lengths, wide=True)
    return restated_scores(c, p, P, x, lengths, torch.float32), restated_scores(c, p, P, x, lengths, torch.float64)


def _scale_recurrence(p, s):
    for n in ('Vgen', 'S1_wildcard', 'wildcard_wildcard'):       # every term of a word's transition matrix carries one of them
        p[n] = (p[n] * np.float32(s)).astype(np.float32)


def _normalise(c, p, x):
    """Neither chain dies nor blows up over the L steps of this batch: first the root-mean-square row norm of a word's transition
    matrix to 1 (what a signed matrix does to a state's length; signed_base's mean absolute row sum lets S = 129 shrink a state
    sixfold a step), then from the float64 chains themselves: the per-step growth of |state| to 1 (the bounded nonlinearities: only
    where the states shrink below a third)."""
    cs, cw = p['C_embed'].sum(0), p['C_wildcard'].sum(0)
    M = np.einsum('wr,ir,jr->wij', p['Vgen'] * cs, p['S1'], p['S2']) + (p['S1_wildcard'] * cw) @ p['S2_wildcard'].T + p['wildcard_wildcard']
    rows = np.sqrt((M.astype(np.float64) ** 2).sum(2)).mean()
    if rows > 0:
        _scale_recurrence(p, 1.0 / rows)
    L = x.shape[1]
    full = np.full(x.shape[0], L, np.int64)
    for _ in range(3):
        F, Bs = chains(c, p, x, full, np.float64)
        end, start = np.linalg.norm(F[:, L]) * np.linalg.norm(Bs[:, L]), np.linalg.norm(F[:, 0]) * np.linalg.norm(Bs[:, 0])
        if not (np.isfinite(end) and end > 0 and start > 0):
            break
        if c.nl in ('tanh', 'relutanh') and end >= start / 3:
            break
        _scale_recurrence(p, float(np.clip((start / end) ** (0.5 / L), 0.25, 4.0)))


def _rescale_scores(p, s):
    """scores times about s (a power of two), every column sum of the label factors (all the recurrence sees of them) kept to
    within K / 512: every entry stays a multiple of 1 / 256, so the create-time folds' column sums are exact in float32 in ANY
    order (at K = 256 a sequential float32 sum of unrounded entries moved the scores by 5e-4: unmet() holds every case to both
    sequential orders)"""
    for n in ('C_embed', 'C_wildcard'):
        a = p[n].astype(np.float64)
        p[n] = (s * a - np.round((s - 1.0) * a.sum(0) / a.shape[0] * 256.0) / 256.0).astype(np.float32)


def default_trans(K, rng):
    tr = rng.uniform(-0.5, 0.5, size=(K, K)).astype(np.float32)
    tr[:, K - 2] = -10000.0
    tr[K - 1, :] = -10000.0
    return tr


def batch(c):
    """every position holds a drawn word: FULL mode computes all of them"""
    rng = np.random.RandomState(c.seed + 1)
    return rng.randint(0, c.V, size=(c.B, c.L)).astype(np.int64), np.asarray(c.lengths, np.int64)


def _tuned_on(c):
    """the case whose batch the draw is tuned on: its own, but the first batch's for the model that one handle serves"""
    if not c.edge.startswith('one handle'):
        return c
    B, L = VARYING_SHAPES[0]
    return c._replace(B=B, L=L, lengths=_lengths(B, L, c.S + c.R + c.RW + c.K))


def model(c):
    """({restatement name: float32 array}, P [K, K] or None, crf transitions [K, K] or None)"""
    rng = np.random.RandomState(c.seed)
    S, R, RW, K = c.S, c.R, c.RW, c.K
    p = d0r.signed_base(c.V, S, R, RW, K, rng, farnn=c.farnn)
    p['C_embed'] = rng.choice(_CVALS, size=(K, R)).astype(np.float32)
    p['C_wildcard'] = rng.choice(_CVALS, size=(K, RW)).astype(np.float32)
    if S <= 4:
        for n in ('S1', 'S2', 'S1_wildcard', 'S2_wildcard', 'wildcard_wildcard', 'h0', 'hT'):
            _refill(p[n], rng)
    if R <= 4:
        for n in ('Vgen', 'S1', 'S2'):
            _refill(p[n], rng)
    if RW <= 4:
        for n in ('S1_wildcard', 'S2_wildcard'):
            _refill(p[n], rng)
    P = None
    if c.prio:
        P = (np.eye(K) + rng.choice([0.0, 0.25, -0.25], size=(K, K), p=[0.7, 0.15, 0.15])).astype(np.float32)
    trans = default_trans(K, rng) if c.crf else None
    if c.tie is not None:
        c1, c2 = c.tie
        p = {n: (np.abs(a) if n not in GATES else a) for n, a in p.items()}
        for n in ('C_embed', 'C_wildcard'):                  # (the clamped last column above the pair: without its clamp it would win)
            p[n][c1] = p[n].max(0)
            p[n][c2] = p[n][c1]
            p[n][K - 1] = np.float32(1.25) * p[n][c1]
    x, lengths = batch(_tuned_on(c))
    _normalise(c, p, x)
    valid = np.arange(x.shape[1])[None, :] < lengths[:, None]
    c = _tuned_on(c)
    if c.tie is None and valid.any():
        sc = reference_pair(c, p, None, x, lengths)[1]
        labels = clamp_col(c)                                # the columns in front of the clamped one
        if labels > 0:
            win = np.bincount(sc[valid][:, :labels].argmax(1), minlength=labels).argmax()
            for n in ('C_embed', 'C_wildcard'):
                p[n][clamp_col(c)] = np.float32(1.25) * p[n][win]
            _normalise(c, p, x)
    for _ in range(3):
        top = float(np.abs(reference_pair(c, p, P, x, lengths)[1][valid]).max()) if valid.any() else 0.0
        if not top > 0 or 4.0 <= top < 8.0 or K == 2:       # (two columns: the shift that keeps the column sums IS their difference)
            break
        _rescale_scores(p, 2.0 ** (2 - np.floor(np.log2(top))))
    return p, P, trans


# ------------------------------------------------------------------------------------------------ the chains, and the scoring step apart
def _fold_order(p, order):
    """p with the label rows permuted: the column sums of the create-time folds taken in another order (float32 cumsum is sequential)"""
    if order is None:
        return None
    return {n: np.cumsum(p[n][::order], axis=0, dtype=np.float32)[-1] for n in ('C_embed', 'C_wildcard')}


def chains(c, p, x, lengths, dtype=np.float32, colsums=None):
    """colsums: {'C_embed': [R], 'C_wildcard': [RW]} to use in place of the references' own column sums.
    (F, Bs) [B, L + 1, S]: F[:, t] the forward state after t tokens (the state BEFORE token t), Bs[:, t] the backward state after
    t tokens from the sequence's end.  Sum semiring: decomp0_train_ref.forward's steps, op for op (torch); max: the oracle's."""
    B, L = x.shape
    if c.semiring == MAX:
        q = {k: (np.asarray(v, dtype) if isinstance(v, np.ndarray) else v) for k, v in _fo_params(c, p).items()}
        with fo.precision(dtype):
            Wsum, csum = fo.decomp_fst_wildcard_sum(q), q['C'].sum(0).astype(dtype)
            if colsums is not None:
                csum = colsums['C_embed'].astype(dtype)
                Wsum = (np.einsum('sr,rj->js', q['S2w'], (colsums['C_wildcard'].astype(dtype)[:, None] * q['S1w'].T)) + q['WW']).astype(dtype)
            xb = fo.reverse_prefix(x, lengths)
            h0b, hTb = np.repeat(q['h0'][None], B, 0), np.repeat(q['hT'][None], B, 0)
            hf, hb = h0b.copy(), hTb.copy()
            F = np.zeros((B, L + 1, c.S), dtype); F[:, 0] = q['h0']
            Bs = np.zeros((B, L + 1, c.S), dtype); Bs[:, 0] = q['hT']
            for i in range(L):
                hf = fo.decomp_fst_step(hf, q['Vgen'][x[:, i]], h0b, csum, Wsum, q, True); F[:, i + 1] = hf
                hb = fo.decomp_fst_step(hb, q['Vgen'][xb[:, i]], hTb, csum, Wsum, q, False); Bs[:, i + 1] = hb
        return F, Bs
    td = torch.float32 if dtype == np.float32 else torch.float64
    q = d0r._params(p, td)
    xt, lens = torch.from_numpy(x), torch.from_numpy(lengths).clamp(0, L)
    cs, cw = (q[n].sum(0) if colsums is None else d0r._t(colsums[n], td) for n in ('C_embed', 'C_wildcard'))
    rtab = q['Vgen'] * cs
    W = (q['S1_wildcard'] * cw) @ q['S2_wildcard'].t() + q['wildcard_wildcard']
    idx = torch.arange(L)
    xr = torch.gather(xt, 1, torch.where(idx[None, :] < lens[:, None], lens[:, None] - 1 - idx[None, :], idx[None, :]))

    def step(h, hin, r, M1, M2, Wm):
        z = None
        if c.farnn >= 1:
            z = torch.sigmoid(SIG_K * (h @ q['Wss1'] + r @ q['Wrs1'] + q['bs1'].reshape(1, -1)))
        hbar = h
        if c.farnn == 2:
            g = torch.sigmoid(SIG_K * (h @ q['Wss2'] + r @ q['Wrs2'] + q['bs2'].reshape(1, -1)))
            hbar = (1 - g) * hin + g * h
        n = d0r.apply_nl(((hbar @ M1) * r) @ M2.t() + hbar @ Wm, c.nl)
        return n if z is None else (1 - z) * h + z * n

    h0, hT = q['h0'].expand(B, -1), q['hT'].expand(B, -1)
    f, b = [h0], [hT]
    for t in range(L):
        f.append(step(f[-1], h0, rtab[xt[:, t]], q['S1'], q['S2'], W))
        b.append(step(b[-1], hT, rtab[xr[:, t]], q['S2'], q['S1'], W.t()))
    return torch.stack(f, 1).numpy(), torch.stack(b, 1).numpy()


def score_step(c, p, P, ch, x, lengths, mutant=None, dtype=np.float32):
    """The scoring step (decomp0_train_ref.forward's on the sum semiring, fo.decomp_fst_scores' on the max semiring) on given
    chains; scores [B, L, K].  Without a mutant it equals the float32 reference bit for bit at every valid position (the sum
    semiring's everywhere).  'f' changes the decode alone: decode(..., mutant='f')."""
    F, Bs = ch
    B, L = x.shape
    R, RW = c.R, c.RW
    lens = np.clip(lengths, 0, L)
    i = np.arange(L)[None, :]
    bidx = np.clip(lens[:, None] - 1 - i, 0, None) + (1 if mutant == 'b' else 0)
    if c.semiring == MAX:
        q = {k: (np.asarray(v, dtype) if isinstance(v, np.ndarray) else v) for k, v in _fo_params(c, p).items()}
        Vg = q['Vgen'] * q['C'].sum(0).astype(dtype) if mutant == 'd' else q['Vgen']
        out = np.zeros((B, L, c.K), dtype)
        for t in range(L):
            al, be = F[:, t + 1] if mutant == 'a' else F[:, t], Bs[np.arange(B), bidx[:, t]]
            ab = ((al @ q['S1']) * (be @ q['S2'])).astype(dtype)
            abw = ((al @ q['S1w']) * (be @ q['S2w'])).astype(dtype)
            if mutant == 'e':
                ab[:, R - R % 4:] = 0
                abw[:, RW - RW % 4:] = 0
            sc = np.einsum('bcr,br->bc', np.einsum('br,cr->bcr', Vg[x[:, t]], q['C']), ab)
            out[:, t] = sc.astype(dtype) if mutant == 'c' else (sc + abw @ q['Cw'].T).astype(dtype)
        if P is not None:
            with fo.precision(dtype):
                out = fo.priority(out, P.astype(dtype))
        return out
    td = torch.float32 if dtype == np.float32 else torch.float64
    q = d0r._params(p, td)
    Ft, Bt = torch.from_numpy(np.ascontiguousarray(F)).to(td), torch.from_numpy(np.ascontiguousarray(Bs)).to(td)
    alpha = Ft[:, 1:L + 1] if mutant == 'a' else Ft[:, :L]
    beta = torch.gather(Bt, 1, torch.from_numpy(bidx).unsqueeze(-1).expand(B, L, Bt.shape[-1]))
    v = q['Vgen'] * q['C_embed'].sum(0) if mutant == 'd' else q['Vgen']
    u = v[torch.from_numpy(x)] * (alpha @ q['S1']) * (beta @ q['S2'])
    uw = (alpha @ q['S1_wildcard']) * (beta @ q['S2_wildcard'])
    if mutant == 'e':
        u, uw = u.clone(), uw.clone()
        u[..., R - R % 4:] = 0
        uw[..., RW - RW % 4:] = 0
    sc = u @ q['C_embed'].t()
    if mutant != 'c':
        sc = sc + uw @ q['C_wildcard'].t()
    if P is not None:
        sc = sc @ d0r._t(P, td)
    return sc.numpy()


def clamped(c, scores, col=None):
    s = np.array(scores, copy=True)
    col = clamp_col(c) if col is None else col
    s[..., col] = np.minimum(s[..., col], s.dtype.type(THRESHOLD))
    return s


def decode(c, scores, lengths, trans, mutant=None, last=False):
    """tags [B, L] int64 (pads -1) in the dtype of `scores`: the first maximal index of the clamped row, the last column as o_idx;
    under the CRF d0r.crf_decode's Viterbi path with column K - 3 clamped.  mutant 'f': the clamp on column K - 1 under the CRF,
    none without it.  last: the LAST maximal index (a wrong decode of the kind a kernel could fall into)."""
    B, L, K = scores.shape
    lens = np.clip(lengths, 0, L)
    valid = np.arange(L)[None, :] < lens[:, None]
    out = np.full((B, L), -1, np.int64)
    if c.crf:
        t = torch.from_numpy(np.array(scores))
        if mutant == 'f':                                    # d0r.crf_decode clamps K - 3: undo it there, clamp K - 1 here
            t[:, :, K - 1] = torch.clamp(t[:, :, K - 1], max=THRESHOLD)
            path = _crf_paths(t, lens, d0r._t(trans, t.dtype), c, clamp=False)
        else:
            path = d0r.crf_decode(t, torch.from_numpy(lens), d0r._t(trans, t.dtype), THRESHOLD, o_idx(c))
        out[valid] = path
        return out
    s = np.array(scores, copy=True) if mutant == 'f' else clamped(c, scores)
    pred = (K - 1 - s[..., ::-1].argmax(-1)) if last else s.argmax(-1)
    pred = pred.astype(np.int64)
    pred[pred == K - 1] = o_idx(c)
    out[valid] = pred[valid]
    return out


def _crf_paths(t, lens, tr, c, clamp):
    """d0r.crf_decode without its clamp: a threshold no score reaches"""
    big = float(t.abs().max()) + 1.0
    return d0r.crf_decode(t, torch.from_numpy(lens), tr, big, o_idx(c))


def max_gap(c, ref32, ref64, valid, margin=1e-4):
    """the decode half of d0r.check_gap on given scores (the max semiring's gap rule): the reason it fails, or None"""
    for sc in (ref32, ref64):
        flat = sc[valid]
        if not flat.size:
            continue
        K = flat.shape[1]
        last = flat[:, K - 1]
        d = clamped(c, flat, K - 1)
        if K > 1:
            top = np.sort(d, 1)[:, -2:]
            gap = top[:, 1] - top[:, 0]
            if ((gap != 0) & (gap < margin * (1 + np.abs(top[:, 1])))).any():
                return 'positions whose top two scores are within the margin'
        if (np.abs(last - THRESHOLD) < margin * (1 + THRESHOLD)).any():
            return 'positions whose last column sits at the threshold clamp'
    return None


Reference = collections.namedtuple('Reference', 'p P trans x lengths mask ref32 ref64 want64 flat64')


def _freeze(a):
    if isinstance(a, np.ndarray):
        a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=8)
def reference(c):
    """Everything the references say about a case, read-only: float32 and float64 scores [B, L, K] (compared at valid positions
    only), the float64 decode [B, L] (pads -1) and its valid entries batch-major"""
    p, P, trans = model(c)
    x, lengths = batch(c)
    ref32, ref64 = reference_pair(c, p, P, x, lengths)
    if c.tie is not None:      # the same arithmetic on equal rows, yet a BLAS may round two columns of one product apart by an ulp
        for a in (ref32, ref64):                             # (unmet() holds the pair as computed to a few ulps)
            a[..., c.tie[1]] = a[..., c.tie[0]]
    mask = np.arange(c.L)[None, :] < lengths[:, None]
    want64 = decode(c, ref64, lengths, trans)
    return Reference({n: _freeze(a) for n, a in p.items()}, _freeze(P), _freeze(trans), _freeze(x), _freeze(lengths), _freeze(mask),
                     _freeze(ref32), _freeze(ref64), _freeze(want64), _freeze(want64[mask]))


def mismatch(c, r, scores, tags=None):
    """None where scores [B, L, K] (and tags [B, L], if given) pass the case's comparator at the valid positions, else what it said"""
    try:
        assert_float_path(scores[r.mask], r.ref32[r.mask], r.ref64[r.mask], TOL)
    except AssertionError as e:
        return str(e)
    if tags is not None and not np.array_equal(tags[r.mask], r.flat64):
        return 'tags differ from the float64 decode'
    return None


def exemption_allowed(c, mu):
    return (mu == 'b' and c.L == 1) or (mu == 'a' and c.S == 1)


def applicable(c, mu):
    return mu != 'e' or c.R % 4 != 0 or c.RW % 4 != 0        # (nothing is left out where both are multiples of 4)


def unmet(c, r=None):
    """The conditions on the INPUTS of one case, from the references alone: the ones it misses (tests/test_decomp0_tag_cases_cpu.py)."""
    r = r or reference(c)
    out = []
    p, P, x, lengths = r.p, r.P, r.x, r.lengths
    if not r.mask.any():                                     # every length 0: nothing to compare; the kernel writes pads alone
        return out
    if c.semiring == SUM:
        try:
            d0r.check_gap(p, P, x, lengths, nl=c.nl, threshold=THRESHOLD, farnn=c.farnn, k=SIG_K, trans=r.trans)
        except d0r.GapError as e:
            out.append('gap rule: {}'.format(e))
        o64 = oracle_scores(c, p, P, x, lengths, wide=True)
        e = np.abs(o64 - r.ref64)[r.mask] / (1 + np.abs(r.ref64[r.mask]))
        if e.max() > 1e-9:
            out.append('the two float64 restatements are {:.2e} apart'.format(e.max()))
    else:
        why = max_gap(c, r.ref32, r.ref64, r.mask)
        if why:
            out.append('gap rule: ' + why)
    if not np.array_equal(decode(c, r.ref32, lengths, r.trans)[r.mask], r.flat64):
        out.append('the float32 and the float64 decode differ')
    e = np.abs(r.ref32.astype(np.float64) - r.ref64)[r.mask] / (1 + np.abs(r.ref64[r.mask]))
    if e.max() > TOL / 10:
        out.append('float32 reference {:.2e} from float64, bar {:.0e}'.format(e.max(), TOL / 10))
    if not (np.abs(r.ref64[r.mask]).max(-1) > 0).all():
        out.append('a valid position with an all-zero score row')
    for order in (1, -1):                                    # the create-time folds' column sums, accumulated one by one in float32
        sc = score_step(c, p, P, chains(c, p, x, lengths, colsums=_fold_order(p, order)), x, lengths)
        e = np.abs(sc.astype(np.float64) - r.ref64)[r.mask] / (1 + np.abs(r.ref64[r.mask]))
        if e.max() > TOL / 10:
            out.append('float32 with sequential column sums (order {}) {:.2e} from float64, bar {:.0e}'.format(order, e.max(), TOL / 10))
    ch = chains(c, p, x, lengths)
    own = score_step(c, p, P, ch, x, lengths)
    if not np.array_equal(own[r.mask], r.ref32[r.mask]):
        out.append('score_step restates another scoring step than the reference\'s')
    for mu in MUTANTS:
        if not applicable(c, mu) or (case_id(c), mu) in EXEMPT:
            continue
        if mu == 'f':
            bad = None if np.array_equal(decode(c, own, lengths, r.trans, mutant='f')[r.mask], r.flat64) else 'tags'
        else:
            bad = mismatch(c, r, score_step(c, p, P, ch, x, lengths, mutant=mu))
        if bad is None:
            out.append('mutant ({}) passes'.format(mu))
    if c.tie is not None:
        c1, c2 = c.tie
        raw = reference_pair(c, p, P, x, lengths)
        if not all(np.allclose(a[..., c1], a[..., c2], rtol=8 * np.finfo(a.dtype).eps, atol=0) and np.array_equal(a[..., c1], b[..., c1])
                   for a, b in zip(raw, (r.ref32, r.ref64))):
            out.append('the planted columns are not equal to a few ulps in the references as computed')
        won = tie_wins(c, r)
        d = (decode(c, r.ref64, lengths, None, last=True) != r.want64)[r.mask]
        if 2 * d.sum() < d.size or 2 * won[r.mask].sum() < d.size:
            out.append('last-index decode differs at {} of {} valid positions, the pair wins {}'.format(int(d.sum()), d.size, int(won[r.mask].sum())))
    return out


def tie_wins(c, r):
    """valid positions where the planted pair is the strict maximum of the clamped float64 scores"""
    c1, c2 = c.tie
    s = clamped(c, r.ref64)
    rest = np.delete(s, [c1, c2], axis=-1).max(-1)
    return (s[..., c1] > rest) & r.mask


# ------------------------------------------------------------------------------------------------ the grid
_SEED_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'decomp0_tag_seeds.json')
if os.path.exists(_SEED_FILE):
    with open(_SEED_FILE) as _f:
        _SEEDS = json.load(_f)
else:                                                       # (only while the file is being searched for the first time)
    _SEEDS = {'seed_bump': {}, 'exempt': []}
SEED_BUMP = _SEEDS['seed_bump']
EXEMPT = frozenset((a, b) for a, b, _ in _SEEDS['exempt'])


def _lengths(B, L, k):
    """L, 1, 0 and one length that leaves 1..3 live positions in its last workgroup, in every batch of four or more"""
    if B == 1:
        return (L,)
    i0 = (L - 1) // D0_TOK * D0_TOK
    part = min(L, i0 + 1 + k % 3)
    ls = [L, 1, 0, part]
    rng = np.random.RandomState(97 * L + B)
    while len(ls) < B:
        ls.append(int(rng.randint(1, L + 1)))
    return tuple(ls[:B])


def _mk(edge, S=5, R=6, RW=3, K=5, V=6, B=4, L=13, lengths=None, nl='tanh', farnn=0, semiring=SUM, prio=0, crf=0, mode=LOCAL, tie=None,
        seed=None):
    lengths = tuple(lengths) if lengths is not None else _lengths(B, L, S + R + RW + K)
    c = Case(S, R, RW, K, V, B, L, lengths, nl, farnn, semiring, prio, crf, mode, 0, edge, tie)
    cid = case_id(c)
    return c._replace(seed=zlib.crc32(cid.encode()) % (2 ** 30) + SEED_BUMP.get(cid, 0) if seed is None else seed)


S_EDGES = collections.OrderedDict([
    (1, 'the scalar tail alone, SP = 4'), (3, 'S < 4: the scalar tail alone'), (4, 'one step of the 4-wide loop, no tail'),
    (5, 'one step and a tail of one, SP = 8'), (64, 'SP = S'), (65, 'a tail of one behind 16 steps'), (72, 'the chain\'s last narrow size'),
    (73, 'the chain\'s first wide size, SP = 76'), (104, 'the shipped automaton size'), (128, 'the wide chain\'s last size'),
    (129, 'the generic chain\'s first size, SP = 132')])
R_EDGES = collections.OrderedDict([
    (1, 'one guarded row of CT, Rp = 4'), (3, 'R < 4: the guard on CT'), (4, 'Rp = R'), (5, 'a second step, three rows guarded'),
    (126, 'R + RW = 129: the wildcard columns fall into the second pass'), (127, 'R + RW = 130, Rp = 128'), (128, 'a whole first pass of language columns'),
    (129, 'the language columns\' second pass'), (250, 'the shipped rank: Rp = 252, two passes')])
RW_EDGES = collections.OrderedDict([
    (1, 'one guarded row of CwT, RWp = 4'), (3, 'RW < 4: the guard on CwT'), (4, 'RWp = RW'), (5, 'a second step, three rows guarded'),
    (67, 'RWp = 68')])
SUM_EDGES = collections.OrderedDict([
    ((100, 28), 'R + RW = 128: one whole pass'), ((100, 29), 'R + RW = 129: lane 0 alone in the second pass'),
    ((190, 67), 'R + RW = 257: the language / wildcard switch inside the second pass, a third pass')])
K_EDGES = collections.OrderedDict([
    (2, 'one label and the clamped column'), (3, 'three columns'), (4, 'four columns'), (5, 'five columns'),
    (63, 'decode: one pass, lane 63 idle'), (64, 'decode: one pass, every lane; Kc = K'), (65, 'decode: a second pass for lane 0, Kc 128'),
    (128, 'the label loop: one whole pass'), (129, 'the label loop\'s second pass, decode: a third pass, Kc 192'),
    (130, 'the benchmark\'s K'), (256, 'the create\'s limit (K = 257 is refused there): two label passes, four decode passes, Kc 256')])
CRF_K = (4, 5, 64, 65, 128, 129, 130)
L_EDGES = collections.OrderedDict([
    (1, 'one position: ntok = 1'), (7, 'ntok = 7 < 8 and nlive < ntok'), (8, 'one whole workgroup'), (9, 'a second workgroup of one position'),
    (16, 'two whole workgroups'), (17, 'a third workgroup of one position')])
TIE_PAIRS = ((3, 67), (0, 64), (63, 64), (1, 130))          # the same lane across passes; lane 0 / lane 0; lane 63 / lane 0; neighbours


def _grid():
    cases, n = [], [0]

    def add(edge, **kw):
        n[0] += 1
        kw.setdefault('mode', (LOCAL, FULL)[n[0] % 2])
        cases.append(_mk(edge, **kw))

    for i, (S, edge) in enumerate(S_EDGES.items()):
        add('S: ' + edge, S=S, nl=('tanh', 'relutanh')[i % 2])
    for R, edge in R_EDGES.items():
        add('R: ' + edge, R=R)
    for RW, edge in RW_EDGES.items():
        add('RW: ' + edge, R=5, RW=RW)
    for (R, RW), edge in SUM_EDGES.items():
        add('R + RW: ' + edge, R=R, RW=RW)
    for K, edge in K_EDGES.items():
        add('K: ' + edge, K=K, **(dict(R=12, RW=7) if K > 16 else {}))
    for i, K in enumerate(CRF_K):
        add('K under the CRF: {} columns, rows of stride Kp = {}'.format(K, round_up(K, 4)), K=K, crf=1, prio=i % 2, **(dict(R=12, RW=7) if K > 16 else {}))
    for K in (65, 130):
        add('priority with K > 64: sc2 across decode passes', K=K, prio=1, R=12, RW=7)
    add('the benchmark\'s shape class: S 64, R 100, RW 29, K 129', S=64, R=100, RW=29, K=129)
    add('every boundary at once: S 65, R 130, RW 67, K 130', S=65, R=130, RW=67, K=130)
    for L, edge in L_EDGES.items():
        for mode in (LOCAL, FULL):
            add('L: ' + edge, L=L, mode=mode)
    for mode in (LOCAL, FULL):
        add('every length 0: pads alone', lengths=(0, 0, 0, 0), mode=mode)
        add('B 1', B=1, mode=mode)
    add('B 9, L 17: drawn lengths behind the four fixed ones', B=9, L=17)
    for nl in ('none', 'relu', 'tanh', 'relutanh'):
        for farnn in (0, 1, 2):
            add('recurrence: {} / farnn {}'.format(nl, farnn), S=9, nl=nl, farnn=farnn)
    for farnn in (0, 1):
        for nl in ('tanh', 'relu'):
            add('max semiring: farnn {} / {}'.format(farnn, nl), S=9, nl=nl, farnn=farnn, semiring=MAX)
    for prio, crf in ((1, 0), (0, 1), (1, 1)):
        for mode in (LOCAL, FULL):
            add('priority {} / CRF {}'.format(prio, crf), K=7, prio=prio, crf=crf, mode=mode)
    for (R, RW), what in zip(lds_shapes()[:3], ('the largest shape within 48 KiB', 'the first above 48 KiB: hipFuncSetAttribute', 'the largest within 160 KiB')):
        add('LDS: {} ({} bytes)'.format(what, d0_geometry(4, R, RW, 3, 9).lds), S=4, R=R, RW=RW, K=3, V=5, L=9)
    assert len({case_id(c) for c in cases}) == len(cases)
    return tuple(cases)


CASES = _grid()
TIE_CASES = tuple(_mk('tie: columns {} and {} bit-equal'.format(c1, c2), K=c2 + 2, R=12, RW=7, tie=(c1, c2), mode=(LOCAL, FULL)[i % 2])
                  for i, (c1, c2) in enumerate(TIE_PAIRS))
# one handle, varying shapes: the same model (one seed) under four batches; the stash stride changes with L
VARYING_SHAPES = ((4, 9), (2, 3), (7, 17), (4, 9))
VARYING_CASES = tuple(_mk('one handle: B {} L {}'.format(B, L), S=17, R=9, RW=5, K=6, prio=1, B=B, L=L, seed=1717, mode=FULL,
                          lengths=(L, 1) if B == 2 else None) for B, L in VARYING_SHAPES)
ALL_CASES = CASES + TIE_CASES + VARYING_CASES[:3]
# against the training step (sum semiring, CE1 and the CRF, farnn 0 and 2, one shape with R % 4 != 0 and K > 64)
TRAIN_CASES = tuple(c for c in CASES if c.mode == LOCAL and c.semiring == SUM and any(c.lengths) and (
    (c.S == 9 and c.nl == 'tanh' and c.farnn in (0, 2)) or (c.K == 7 and c.crf) or (c.K == 65 and c.R == 12 and not c.crf)
    or (c.K == 130 and c.S == 65) or (c.crf and c.K in (5, 65))))


def refused_lds_shape():
    """(S, R, RW, K) of the first shape whose score kernel does not fit 160 KiB: refused by farnn_tag, before its launch"""
    R, RW = lds_shapes()[3]
    return 4, R, RW, 3


def search_seeds(limit=400):
    """redraw every case that misses a condition with later seeds; the recorded result"""
    global SEED_BUMP, EXEMPT
    bumps, exempt = {}, []
    SEED_BUMP, EXEMPT = {}, frozenset()
    for c in ALL_CASES:
        cid = case_id(c)
        base = c.seed - _SEEDS['seed_bump'].get(cid, 0)
        for k in range(limit):
            cc = c._replace(seed=base + k)
            miss = unmet(cc, None)
            excused = [m for m in miss if m.startswith('mutant (') and exemption_allowed(c, m[8])]
            if len(excused) == len(miss):
                if k:
                    bumps[cid] = k
                reasons = {'a': 'S = 1: a state that stays put', 'b': 'L = 1'}
                exempt += [[cid, m[8], reasons[m[8]]] for m in excused]
                break
            if c in VARYING_CASES:                          # (one model for all of them: its seed is chosen by hand)
                raise SystemExit('the shared model of the varying shapes misses: {} {}'.format(cid, miss))
        else:
            raise SystemExit('no conforming draw for {} in {} seeds: {}'.format(cid, limit, miss))
        print(cid, k, [e[1] for e in exempt if e[0] == cid], flush=True)
    with open(_SEED_FILE, 'w') as f:
        json.dump({'exempt': exempt, 'seed_bump': bumps}, f, indent=0, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    search_seeds()
