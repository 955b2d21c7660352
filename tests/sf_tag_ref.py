"""The vector-input tagger (FARNN_S_SF) restated through the existing oracle, for the CPU and GPU tests of farnn_tag_vectors.

FARNN_S_SF.forward is FARNN_S_D_W_I_S.forward_local with the looked-up row Vgen[x[b, t]] replaced by the given vector
v[b, t]: the oracle's decomposed i-FST forward, called with Vgen := v.reshape(B L, R) and the identity ids b L + t, IS that
model.  Nothing under oracle/ is edited.

Which tags are compared: a float32 evaluation may move every score by the parity bar TOL (1 + |s|) (util.assert_float_path),
so a decode is only determined where the float64 scores separate the winner from the runner-up by more than what two such
errors can close:
  argmax decode:  top1 - top2 > 2 TOL (1 + max(|top1|, |top2|))            at the position;
  CRF decode:     the best path beats every path that differs from it somewhere by more than 2 TOL sum_t (1 + max_j |s[t, j]|)
                  (a path's score sums one emission per position; the transitions are the same constants on both sides);
                  a sequence below that leaves all its positions out.
At most UNDECIDED_CAP of a config's valid positions may be left out; the fixture's inputs were drawn so that none is.
"""
import json
import os

import numpy as np

from oracle import farnn_oracle as fo
from util import GOLDEN, in_float64

TOL = 1e-4
UNDECIDED_CAP = 0.02


def fixture():
    """(configs of decomp_small.json, meta of sf_small.json, decomp_small.npz, sf_small.npz)"""
    with open(os.path.join(GOLDEN, 'decomp_small.json')) as f:
        dmeta = json.load(f)
    with open(os.path.join(GOLDEN, 'sf_small.json')) as f:
        smeta = json.load(f)
    return dmeta, smeta, np.load(os.path.join(GOLDEN, 'decomp_small.npz')), np.load(os.path.join(GOLDEN, 'sf_small.npz'))


def sf_configs():
    with open(os.path.join(GOLDEN, 'sf_small.json')) as f:
        return json.load(f)['configs']


def params_from_fixture(g, k, cfg):
    """The oracle's parameter dict (without Vgen) of config k of decomp_small."""
    pre = 'c{}.'.format(k)
    p = {'S1': g[pre + 'S1'], 'S2': g[pre + 'S2'], 'W': g[pre + 'wildcard_mat'], 'Cout': g[pre + 'C_output_mat'],
         'h0': g[pre + 'h0'], 'hT': g[pre + 'hT'], 'farnn': cfg.get('farnn', 0),
         'nl': fo.NL_CODES[cfg.get('update_nonlinear', 'none')], 'semiring': fo.SEMIRING_SUM,
         'sig_k': cfg.get('sigmoid_exponent', 5)}
    for kk in ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2'):
        if pre + kk in g.files:
            p[kk] = g[pre + kk]
    return p


def gates_of(p):
    return {k: (p[k].reshape(-1) if k.startswith('bs') else p[k]) for k in ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2') if k in p}


def restate(p, v, lengths, P=None, wide=False):
    """scores [B, lengths.max(), K] of the vector-input model: float32 like the kernels, or (wide) float64."""
    B, L, R = v.shape
    ids = np.arange(B * L, dtype=np.int64).reshape(B, L)
    q = dict(p, Vgen=np.ascontiguousarray(v).reshape(B * L, R))
    if wide:
        return in_float64(fo.decomp_ifst_scores, q, ids, lengths, P=None if P is None else P.astype(np.float64))
    return fo.decomp_ifst_scores(q, ids, lengths, P)


def _clamped(s, col, threshold):
    s = np.array(s, np.float64, copy=True)
    s[..., col] = np.minimum(s[..., col], threshold)
    return s


def decided(s64, lengths, threshold, crf_tr=None):
    """bool [B, L]: the valid positions whose tag the float64 scores decide beyond the float path's error (module docstring)."""
    B, L, K = s64.shape
    out = np.zeros((B, L), bool)
    if crf_tr is None:
        s = _clamped(s64, K - 1, threshold)
        top = np.sort(s, axis=-1)
        t1, t2 = top[..., -1], top[..., -2]
        ok = (t1 - t2) > 2 * TOL * (1 + np.maximum(np.abs(t1), np.abs(t2)))
        return ok & (np.arange(L)[None, :] < np.asarray(lengths)[:, None])
    s = _clamped(s64, K - 3, threshold)
    tr = np.asarray(crf_tr, np.float64)
    START, STOP = K - 2, K - 1
    for b in range(B):
        n = int(lengths[b])
        f = s[b, :n]
        al = np.zeros((n, K)); be = np.zeros((n, K))
        al[0] = f[0] + tr[START]
        for t in range(1, n):
            al[t] = f[t] + (al[t - 1][:, None] + tr).max(0)
        be[n - 1] = tr[:, STOP]
        for t in range(n - 2, -1, -1):
            be[t] = (tr + (f[t + 1] + be[t + 1])[None, :]).max(1)
        through = al + be                                     # best path through tag j at position t
        best = through.max(1)
        path = through.argmax(1)
        rest = through.copy()
        rest[np.arange(n), path] = -np.inf
        margin = best[0] - rest.max()
        out[b, :n] = margin > 2 * TOL * (1 + np.abs(f).max(1)).sum()
    return out


def decided_positions(g, k, cfg, meta, v, lengths):
    pre = 'c{}.'.format(k)
    P = g[pre + 'priority_mat'] if cfg.get('use_priority', 0) else None
    s64 = restate(params_from_fixture(g, k, cfg), v, lengths, P, wide=True)
    tr = g[pre + 'crf_transitions'] if cfg.get('use_crf', 0) else None
    return decided(s64, lengths, meta['threshold'], tr)


def flat_mask(mask, lengths):
    """the [B, L] mask in forward_local's flat order"""
    return fo.flatten(mask, lengths)
