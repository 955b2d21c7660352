"""A torch restatement of the decomposed independent=1 training step under --use_crf 1 (FARNN_S_D_W_I, farnn = 0, CE1; DESIGN.md,
row f9): decomp1_train_ref.forward with the CRF on top, written from the arithmetic, for the tests of
farnn_decomp_ind1_crf_train_step.  Evaluates in the dtype it is asked for (float32 or float64), differentiates with autograd.

Reference citations (src_seq/baselines/crf.py, src_seq/farnn/model_decompose.py):
  emissions f = score [. P]; C = labels + 2, START = C-2, STOP = C-1              model_decompose_independent.py:45-47, :277-278
  alpha_0[j] = trans[START, j] + f_0[j]; alpha_t[j] = logsumexp_i(alpha_{t-1}[i] + trans[i, j]) + f_t[j] over the valid
  positions; log Z = logsumexp_i(alpha_{n-1}[i] + trans[i, STOP])                 crf.py:48-99
  gold = sum_t (f_t[y_t] + trans[y_{t-1}, y_t]), y_{-1} = START, + trans[y_{n-1}, STOP]   crf.py:202-251 (no START energy beyond
                                                                                  the bigram of position 0)
  loss = sum over the sequences of log Z - gold (a sum, not a mean)               crf.py:253-260
  decode: column C-3 of the emissions clamped to threshold, Viterbi with the first index winning a tie (torch.max),
  C-3 -> o_idx                                                                    model_decompose.py:349-356, crf.py:102-195
A sequence of length 0 contributes nothing (the reference cannot run one: crf.py:232 gathers at length - 1).

The gap rule: decomp1_train_ref.check_gap's rule on the chains' pre-activations, and (viterbi(check=True), the float64 path)
every Viterbi maximisation the decoded path reads -- the last one into STOP and the one behind every back-pointer it follows
-- has its runner-up farther than min_gap + margin (1 + |top|) from the top.  That covers the decode: if another complete
path came within the margin of the best one, the maximisation at which the two merge lies on the best path and its runner-up
is at least that close.  The maximisations off the path are not held to it: into a column behind a -10000 transition
(START, or out of STOP) |top| is 1e4, where the margin is 1 and float32 resolves 1e-3 -- no case could pass.

`fault` plants one wrong statement, for the tests that show the fixtures see it: 'mean', 'no_stop', 'clamp_last', 'last_tie',
'no_gold_counts'.
"""
import numpy as np
import torch

import decomp1_max_train_ref as dmr
import decomp1_train_ref as dtr
from decomp1_train_ref import GapError, _ints, _params, _t

TRANS = 'crf.transitions'
FAULTS = ('mean', 'no_stop', 'clamp_last', 'last_tie', 'no_gold_counts')


def default_transitions(C):
    """CRF.__init__ (crf.py:39-41) for C = labels + 2 tags"""
    tr = np.zeros((C, C), np.float32)
    tr[:, C - 2] = -10000.0
    tr[C - 1, :] = -10000.0
    return tr


def crf_nll(em, trans, lens, labels, fault=None):
    """sum over the sequences of log Z - gold; em [B, L, C]"""
    B, L, C = em.shape
    START, STOP = C - 2, C - 1
    gtr = trans.detach() if fault == 'no_gold_counts' else trans
    total = em.new_zeros(())
    for b in range(B):
        n = int(lens[b])
        if n == 0:
            continue
        f, y = em[b, :n], labels[b, :n]
        a = trans[START] + f[0]
        for t in range(1, n):
            a = torch.logsumexp(a[:, None] + trans, 0) + f[t]
        logZ = torch.logsumexp(a + trans[:, STOP], 0)
        prev = torch.cat([torch.tensor([START]), y[:-1]])
        gold = f[torch.arange(n), y].sum() + gtr[prev, y].sum()
        if fault != 'no_stop':
            gold = gold + gtr[y[-1], STOP]
        total = total + (logZ - gold)
    return total / B if fault == 'mean' else total


def _argmax(v, last):
    """(index, top, runner-up) of a 1-D array: the first maximum as torch.max, the last one under the planted fault"""
    top = v.max()
    idx = np.flatnonzero(v == top)
    k = int(idx[-1] if last else idx[0])
    rest = np.delete(v, k)
    return k, top, (rest.max() if rest.size else -np.inf)


def viterbi(em, trans, lens, threshold, o_idx, fault=None, check=False, min_gap=2e-5, margin=1e-4):
    """flat predictions (the valid positions, sequence after sequence) of numpy emissions [B, L, C]; check: the gap rule"""
    em, trans = np.asarray(em), np.asarray(trans)
    B, L, C = em.shape
    START, STOP = C - 2, C - 1
    col = C - 1 if fault == 'clamp_last' else C - 3
    last = fault == 'last_tie'
    out = []
    for b in range(B):
        n = int(lens[b])
        if n == 0:
            continue
        f = em[b, :n].copy()
        f[:, col] = np.minimum(f[:, col], em.dtype.type(threshold))
        v = f[0] + trans[START]
        bp, gaps = [], []
        for t in range(1, n):
            cand = (f[t][None, :] + trans) + v[:, None]              # [from, to] (crf.py:123, :145)
            res = [_argmax(cand[:, j], last) for j in range(C)]
            bp.append([r[0] for r in res])
            gaps.append([(r[1], r[2]) for r in res])
            v = np.array([r[1] for r in res], em.dtype)
        ptr, top, second = _argmax(v + trans[:, STOP], last)
        read = [(top, second)]
        path = [ptr]
        for t in range(n - 1, 0, -1):
            read.append(gaps[t - 1][ptr])
            ptr = bp[t - 1][ptr]
            path.append(ptr)
        if check:
            for top, second in read:
                if top - second < min_gap + margin * (1 + abs(top)):
                    raise GapError('a Viterbi maximisation on the decoded path of sequence {} has its runner-up within the margin'.format(b))
        out.extend(path[::-1])
    pred = np.asarray(out, np.int64)
    pred[pred == C - 3] = o_idx
    return pred


def emissions(p, P, x, lens, nl, add_nl, semiring):
    """[B, L, C]: the scores of decomp1_train_ref.forward (sum semiring) or decomp1_max_train_ref.forward (max) -- the reference
    sends only the two recurrences through semiring_func, the CRF on top is the same"""
    return (dmr if semiring == 'max' else dtr).forward(p, P, x, lens, nl=nl, add_nl=add_nl)[0]


def check_gap(p, P, trans, x, lengths, nl='none', add_nl='none', threshold=0.5, o_idx=0, min_gap=2e-5, margin=1e-4,
              semiring='sum'):
    """Raises GapError unless the rule of the module docstring holds on these inputs: the chains in float32 and float64 (max:
    decomp1_max_train_ref.check_gap's arg-max rule), the Viterbi maximisations on the float64 path."""
    x, lengths = _ints(x), _ints(lengths)
    lens = lengths.clamp(0, x.shape[1])
    if semiring == 'max':
        dmr.check_gap(p, P, x, lens, nl=nl, add_nl=add_nl, min_gap=max(min_gap, 2e-5), relu_gap=min_gap)
    elif nl in ('relu', 'relutanh'):
        for dtype in (torch.float32, torch.float64):
            with torch.no_grad():
                _, _, pre, mag = dtr.forward(_params(p, dtype), None if P is None else _t(P, dtype), x, lens, nl=nl, add_nl=add_nl)
            live = (torch.arange(x.shape[1])[None, :] < lens[:, None] - 1)[None, :, :, None]
            bad = live & (pre != 0) & (pre.abs() < torch.clamp(8 * pre.shape[-1] * dtr.EPS32 * mag, min=min_gap))
            if bool(bad.any()):
                raise GapError('{} chain pre-activations within the gap of 0 in {}'.format(int(bad.sum()), dtype))
    with torch.no_grad():
        sc = emissions(_params(p, torch.float64), None if P is None else _t(P, torch.float64), x, lens, nl, add_nl, semiring)
    viterbi(sc.numpy(), np.asarray(trans, np.float64), lens.numpy(), threshold, o_idx, check=True, min_gap=max(min_gap, 2e-5),
            margin=margin)


def step(p, P, trans, x, lengths, labels, nl='none', add_nl='none', threshold=0.5, o_idx=0, dtype=torch.float64, fault=None,
         semiring='sum'):
    """(loss, {name: gradient} for every float tensor of p and for 'crf.transitions', flat_pred) of one training step in `dtype`"""
    x, lengths, labels = _ints(x), _ints(lengths), _ints(labels)
    lens = lengths.clamp(0, x.shape[1])
    pt = _params(dict(p, **{TRANS: trans}), dtype, grad=True)
    Pt = None if P is None else _t(P, dtype)
    sc = emissions({k: v for k, v in pt.items() if k != TRANS}, Pt, x, lens, nl, add_nl, semiring)
    loss = crf_nll(sc, pt[TRANS], lens, labels, fault)
    loss.backward()
    grads = {k: (t.grad.detach().numpy() if t.grad is not None else np.zeros(tuple(t.shape), t.detach().numpy().dtype))
             for k, t in pt.items()}
    pred = viterbi(sc.detach().numpy(), pt[TRANS].detach().numpy(), lens.numpy(), threshold, o_idx, fault)
    return float(loss.detach()), grads, pred
