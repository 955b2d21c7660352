"""A torch restatement of the onehot i-FST training step in the MAX semiring (FARNN_S_O_I_S, --train_mode max, CE1 loss),
written from the arithmetic, for the tests of farnn_onehot_ifst_train_step after farnn_onehot_train_set_semiring(MAX).
Evaluates in the dtype of its inputs (float32 or float64) and differentiates with autograd.

Reference citations (src_seq/farnn/model_onehot.py unless noted):
  semiring_func = _maxmul                          :57; utils.py:192-195 (torch.max(dim=1): ONE index per target state, the
                                                   first maximal one, and its backward sends the whole adjoint there)
  forward chain  f_t = nl(max_j(f_{t-1}[j] M_{x_t}[j,s]) * o)             :376-387
  backward chain b_t = nl(max_j((b_{t-1} * o)[j] M_{x'_t}[s,j]))          :390-401
  scores, priority, loss, decode                   as the sum step (onehot_train_ref.py)

min_gap (the rule of decomp_max_train_ref.py, extended by one case): at every step that reaches a valid score, a non-zero
maximum must beat the runner-up by at least min_gap relative, in the float32 AND the float64 evaluation, so that rounding
cannot decide which index wins -- or it may tie the runner-up EXACTLY in both evaluations (structurally identical paths of
a 0/1 automaton: both sides then take the first index).  Exact-zero maxima stay exempt: a product with a zero factor is
exactly +-0 under any rounding.  Anything else raises GapError.  The pad steps, which the reference runs too, reach no
valid score and are not held to the rule.
"""
import numpy as np
import torch

from onehot_train_ref import _nl, _t


class GapError(AssertionError):
    pass


def _reversed_tokens(x, lens):
    L = x.shape[1]
    idx = torch.arange(L)
    src = torch.where(idx[None, :] < lens[:, None], lens[:, None] - 1 - idx[None, :], idx[None, :])
    return torch.gather(x, 1, src)


def _chains(T, W, O, h0, hT, x, lens, nl, tops=None):
    """F, Bs [B, L+1, S]: the states of both chains.  tops: a list that receives, per step, the two largest candidates of
    the forward and of the backward chain ([2 chains, 2, B, S], detached) for the gap rule."""
    B, L = x.shape
    M = T + W
    o = O.sum(0)
    xr = _reversed_tokens(x, lens)
    f, b = [h0.expand(B, -1)], [hT.expand(B, -1)]
    for t in range(L):
        tf = f[-1].unsqueeze(2) * M[x[:, t]]                               # [B, j, s] = f[j] M[j, s]
        tb = (b[-1] * o).unsqueeze(2) * M[xr[:, t]].transpose(1, 2)        # [B, j, s] = c[j] M[s, j]
        if tops is not None and tf.shape[1] > 1:
            with torch.no_grad():
                tops.append(torch.stack([torch.topk(tf, 2, dim=1).values.transpose(0, 1),
                                         torch.topk(tb, 2, dim=1).values.transpose(0, 1)]))
        f.append(_nl(torch.max(tf, dim=1)[0] * o, nl))
        b.append(_nl(torch.max(tb, dim=1)[0], nl))
    return torch.stack(f, 1), torch.stack(b, 1)


def check_gap(T, W, O, h0, hT, x, lengths, nl='none', min_gap=2e-5):
    """Raises GapError unless the rule of the module docstring holds on these inputs."""
    x = torch.as_tensor(np.asarray(x))
    lens = torch.as_tensor(np.asarray(lengths)).clamp(0, x.shape[1])
    ev = {}
    for dtype in (torch.float32, torch.float64):
        tops = []
        with torch.no_grad():
            _chains(*(_t(a, dtype) for a in (T, W, O, h0, hT)), x, lens, nl, tops)
        if not tops:
            return
        ev[dtype] = torch.stack(tops)                                      # [L, 2 chains, 2, B, S]
    L = x.shape[1]
    t = torch.arange(L)[:, None]
    # steps that reach a valid score: t < len forward, t < len - 1 backward (b_len feeds no score)
    live = torch.stack([t < lens[None, :], t < lens[None, :] - 1], 1).unsqueeze(-1)      # [L, 2, B, 1]
    tie = (ev[torch.float32][:, :, 0] == ev[torch.float32][:, :, 1]) & (ev[torch.float64][:, :, 0] == ev[torch.float64][:, :, 1])
    for dtype, e in ev.items():
        top, second = e[:, :, 0], e[:, :, 1]
        ok = (top == 0) | ((top - second) >= min_gap * top.abs()) | tie
        bad = live & ~ok
        if bool(bad.any()):
            raise GapError('{} maxima are decided by less than {} relative in {} without being exact ties in both '
                           'evaluations'.format(int(bad.sum()), min_gap, dtype))


def loss_and_pred(T, W, O, h0, hT, P, x, lengths, labels, nl, threshold, o_idx):
    x = torch.as_tensor(np.asarray(x)) if not torch.is_tensor(x) else x
    lengths = torch.as_tensor(np.asarray(lengths)) if not torch.is_tensor(lengths) else lengths
    B, L = x.shape
    lens = lengths.clamp(0, L)
    F, Bs = _chains(T, W, O, h0, hT, x, lens, nl)
    i = torch.arange(L)[None, :].expand(B, L)
    bidx = (lens[:, None] - 1 - i).clamp(min=0)
    alpha = F[:, 1:]
    beta = torch.gather(Bs, 1, bidx.unsqueeze(-1).expand(B, L, Bs.shape[-1]))
    sc = torch.einsum('cs,bls->blc', O, alpha * beta)
    if P is not None:
        sc = sc @ P
    valid = i < lens[:, None]
    lab = torch.as_tensor(np.asarray(labels)) if not torch.is_tensor(labels) else labels
    flat = sc[valid]
    loss = torch.nn.functional.cross_entropy(flat, lab[valid])
    with torch.no_grad():
        d = flat.clone()
        C = d.shape[1]
        d[:, C - 1] = torch.clamp(d[:, C - 1], max=threshold)
        pred = d.argmax(1)
        pred[pred == C - 1] = o_idx
    return loss, pred.numpy()


def step(T, W, O, h0, hT, P, x, lengths, labels, nl='none', threshold=0.5, o_idx=0, dtype=torch.float64, min_gap=None):
    """(loss, dT, flat_pred) of one training step, evaluated in `dtype`; with min_gap the inputs are held to the gap rule."""
    if min_gap is not None:
        check_gap(T, W, O, h0, hT, x, lengths, nl, min_gap)
    Tt = _t(T, dtype).clone().requires_grad_(True)
    Wt, Ot, h0t, hTt = (_t(a, dtype) for a in (W, O, h0, hT))
    Pt = None if P is None else _t(P, dtype)
    loss, pred = loss_and_pred(Tt, Wt, Ot, h0t, hTt, Pt, x, lengths, labels, nl, threshold, o_idx)
    loss.backward()
    return float(loss.detach()), Tt.grad.detach().numpy(), pred


def adam_steps(T, W, O, h0, hT, P, batches, nl='none', lr=1e-3, dtype=torch.float64, min_gap=None, losses=None):
    """language_tensor after one Adam step (torch.optim.Adam, weight_decay 0) per (x, lengths, labels) of `batches`; with
    min_gap the gap rule is asserted on the weights of every step; `losses`: a list that receives every step's loss."""
    Tt = _t(T, dtype).clone().requires_grad_(True)
    Wt, Ot, h0t, hTt = (_t(a, dtype) for a in (W, O, h0, hT))
    Pt = None if P is None else _t(P, dtype)
    opt = torch.optim.Adam([Tt], lr=lr, weight_decay=0)
    for x, lengths, labels in batches:
        if min_gap is not None:
            check_gap(Tt.detach(), Wt, Ot, h0t, hTt, x, lengths, nl, min_gap)
        opt.zero_grad()
        loss, _ = loss_and_pred(Tt, Wt, Ot, h0t, hTt, Pt, x, lengths, labels, nl, 0.5, 0)
        loss.backward()
        opt.step()
        if losses is not None:
            losses.append(float(loss.detach()))
    return Tt.detach().numpy()

