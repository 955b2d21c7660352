"""The two recurrences of the FST / independent=1 models in the MAX semiring, shared by the restatements
fst4_max_train_ref.py, ind1_max_train_ref.py and decomp1_max_train_ref.py (written from the arithmetic; torch, any dtype).

Reference: semiring_func = _maxmul when --train_mode max (src_seq/farnn/model_onehot.py:57, used at :93, :100, :264, :276;
model_decompose_independent.py:177-179) and utils._maxmul (utils.py:192-195): torch.max(dim=1) over hidden[j] M[j, s], ONE
index per target state, the first maximal one, and its backward sends the whole adjoint there.  Only the recurrences go
through it; the score of a position, the priority layer, the loss and the decode stay sum-times.
  forward chain   alpha_{t+1}[s] = nl(max_j alpha_t[j] M_{x_t}[j, s]),   alpha_0 = h0
  backward chain  b_{t+1}[s]     = nl(max_j b_t[j] M_{x'_t}[s, j]),      b_0 = hT,  x' = reverse(x, len)   (b_t = beta_{len-t})

The arg-max gap rule (check_argmax_gap, the rule of onehot_train_max_ref.check_gap): at every step that reaches a valid score
a non-zero maximum beats the runner-up by min_gap relative, in float32 AND in float64, or ties it EXACTLY in both (both
sides then take the first index).  Exact-zero maxima are exempt: a product with a zero factor is +-0 under any rounding.

`fault` plants one of the faults the CPU tests show the fixtures can see:
  'sum'       sum chains in place of max chains
  'last'      the last maximal index in place of the first
  'fwd_idx'   the forward chain's index used for the backward chain (the backward chain's candidate at that index)
  'no_carry0' the first chain step carries nothing back into h0 / hT (the row-0 carry of dh0 / dhT dropped)
"""
import torch


class GapError(AssertionError):
    pass


def reversed_tokens(x, lens):
    L = x.shape[1]
    idx = torch.arange(L)
    src = torch.where(idx[None, :] < lens[:, None], lens[:, None] - 1 - idx[None, :], idx[None, :])
    return torch.gather(x, 1, src)


def _pick(cand, fault, other_idx=None):
    """cand [B, j, s] -> (value [B, s], index [B, s]) of the step"""
    if fault == 'sum':
        return cand.sum(1), None
    if fault == 'last':
        S = cand.shape[1]
        idx = S - 1 - torch.max(cand.flip(1), dim=1)[1]
        return torch.gather(cand, 1, idx.unsqueeze(1)).squeeze(1), idx
    if other_idx is not None:
        return torch.gather(cand, 1, other_idx.unsqueeze(1)).squeeze(1), other_idx
    v, idx = torch.max(cand, dim=1)              # the first maximal index (torch.max on the CPU; -0 == +0)
    return v, idx


def chains(M, h0, hT, x, lens, nl, fault=None, tops=None, pre=None):
    """F, Bs [B, L+1, S]: alpha_t and beta_{len-t}.  nl: a function.  tops: a list that receives, per step, the two largest
    candidates of both chains ([2 chains, 2, B, S], detached); pre: a list that receives the pre-activations [2, B, S]"""
    B, L = x.shape
    xr = reversed_tokens(x, lens)
    f, b = [h0.expand(B, -1)], [hT.expand(B, -1)]
    for t in range(L):
        inf, inb = (f[-1].detach(), b[-1].detach()) if fault == 'no_carry0' and t == 0 else (f[-1], b[-1])
        cf = inf.unsqueeze(2) * M[x[:, t]]                                 # [B, j, s] = alpha[j] M[j, s]
        cb = inb.unsqueeze(2) * M[xr[:, t]].transpose(1, 2)                # [B, j, s] = b[j] M[s, j]
        if tops is not None and cf.shape[1] > 1:
            with torch.no_grad():
                tops.append(torch.stack([torch.topk(cf, 2, dim=1).values.transpose(0, 1),
                                         torch.topk(cb, 2, dim=1).values.transpose(0, 1)]))
        pf, jf = _pick(cf, fault)
        pb, _ = _pick(cb, fault, other_idx=jf if fault == 'fwd_idx' else None)
        if pre is not None:
            pre.append(torch.stack([pf, pb]).detach())
        f.append(nl(pf))
        b.append(nl(pb))
    return torch.stack(f, 1), torch.stack(b, 1)


def states_at_positions(F, Bs, lens):
    """alpha_i (the state BEFORE token i) and beta_{i+1} of every position [B, L, S], valid [B, L]"""
    B, L = F.shape[0], F.shape[1] - 1
    i = torch.arange(L)[None, :].expand(B, L)
    bidx = (lens[:, None] - 1 - i).clamp(min=0)
    beta = torch.gather(Bs, 1, bidx.unsqueeze(-1).expand(B, L, Bs.shape[-1]))
    return F[:, :L], beta, i < lens[:, None]


def check_argmax_gap(run, x, lens, min_gap=2e-5, relu=True, relu_gap=None):
    """run(dtype, tops, pre) evaluates the chains in dtype and fills the two lists.  Raises GapError unless the arg-max rule
    holds and (relu) every chain pre-activation that can reach a score is exactly 0 or relu_gap (min_gap when not given) away
    from 0."""
    relu_gap = min_gap if relu_gap is None else relu_gap
    L = x.shape[1]
    t = torch.arange(L)[:, None]
    live = torch.stack([t < lens[None, :] - 1, t < lens[None, :] - 1], 1).unsqueeze(-1)      # alpha_len and beta_0 feed nothing
    ev = {}
    for dtype in (torch.float32, torch.float64):
        tops, pre = [], []
        with torch.no_grad():
            run(dtype, tops, pre)
        p = torch.stack(pre)                                                   # [L, 2, B, S]
        bad = live & (p != 0) & (p.abs() < relu_gap)
        if relu and bool(bad.any()):
            raise GapError('{} chain pre-activations within {} of 0 in {}'.format(int(bad.sum()), relu_gap, dtype))
        if tops:
            ev[dtype] = torch.stack(tops)                                      # [L, 2 chains, 2, B, S]
    if not ev:
        return
    tie = (ev[torch.float32][:, :, 0] == ev[torch.float32][:, :, 1]) & (ev[torch.float64][:, :, 0] == ev[torch.float64][:, :, 1])
    for dtype, e in ev.items():
        top, second = e[:, :, 0], e[:, :, 1]
        ok = (top == 0) | ((top - second) >= min_gap * top.abs()) | tie
        bad = live & ~ok
        if bool(bad.any()):
            raise GapError('{} maxima are decided by less than {} relative in {} without being exact ties in both '
                           'evaluations'.format(int(bad.sum()), min_gap, dtype))
