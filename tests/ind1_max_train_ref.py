"""A torch restatement of the onehot independent=1 training step in the MAX semiring (FARNN_S_O_I, --train_mode max, CE1),
written from the arithmetic, for the tests of farnn_ind1_train_step after farnn_ind1_train_set_semiring(MAX).  The chains are
max_chains_ref.chains on Mc_w = N_w (* Osum) with relu (src_seq/farnn/model_onehot.py:259-279); the score, the priority layer,
the loss and the decode are the sum step's (ind1_train_ref.py: :229-233, :293-302, :131-180), restated on the max chains'
states.  Evaluates in float32 or float64 and differentiates with autograd.  `fault`: max_chains_ref's planted faults."""
import numpy as np
import torch

import max_chains_ref as mc
from ind1_train_ref import _ints, _t, signed_base  # noqa: F401  (signed_base: the tests' and the capture script's base)
from max_chains_ref import GapError  # noqa: F401


def forward(T, W, O, h0, hT, P, x, lengths, mask=False, fault=None, tops=None, pre=None):
    """scores [B, L, C] (after the priority layer), valid [B, L]"""
    x, lengths = _ints(x), _ints(lengths)
    lens = lengths.clamp(0, x.shape[1])
    N = T + W
    M = N * O.sum(0) if mask else N
    F, Bs = mc.chains(M, h0, hT, x, lens, torch.relu, fault=fault, tops=tops, pre=pre)
    alpha, beta, valid = mc.states_at_positions(F, Bs, lens)
    ab = (alpha[:, :, :, None] * beta[:, :, None, :]) * N[x]   # [B, L, S, S]
    sc = torch.einsum('csj,blsj->blc', O, ab)
    if P is not None:
        sc = sc @ P
    return sc, valid


def check_gap(T, W, O, h0, hT, x, lengths, mask=False, min_gap=2e-5):
    """the arg-max rule and the sum fixtures' relu rule on the chain pre-activations (max_chains_ref.check_argmax_gap)"""
    x, lengths = _ints(x), _ints(lengths)
    lens = lengths.clamp(0, x.shape[1])
    mc.check_argmax_gap(lambda dtype, tops, pre: forward(*(_t(a, dtype) for a in (T, W, O, h0, hT)), None, x, lens, mask=mask,
                                                         tops=tops, pre=pre), x, lens, min_gap)


def loss_and_pred(T, W, O, h0, hT, P, x, lengths, labels, threshold, o_idx, mask=False, fault=None):
    sc, valid = forward(T, W, O, h0, hT, P, x, lengths, mask=mask, fault=fault)
    flat = sc[valid]
    loss = torch.nn.functional.cross_entropy(flat, _ints(labels)[valid])
    with torch.no_grad():
        d = flat.clone()
        C = d.shape[1]
        d[:, C - 1] = torch.clamp(d[:, C - 1], max=threshold)
        pred = d.argmax(1)
        pred[pred == C - 1] = o_idx
    return loss, pred.numpy()


def step(T, W, O, h0, hT, P, x, lengths, labels, mask=False, threshold=0.5, o_idx=0, dtype=torch.float64, fault=None):
    """(loss, dT, flat_pred) of one training step, evaluated in `dtype`."""
    Tt = _t(T, dtype).clone().requires_grad_(True)
    Wt, Ot, h0t, hTt = (_t(a, dtype) for a in (W, O, h0, hT))
    Pt = None if P is None else _t(P, dtype)
    loss, pred = loss_and_pred(Tt, Wt, Ot, h0t, hTt, Pt, x, lengths, labels, threshold, o_idx, mask=mask, fault=fault)
    loss.backward()
    return float(loss.detach()), Tt.grad.detach().numpy(), pred


def adam_steps(T, W, O, h0, hT, P, batches, mask=False, lr=1e-3, dtype=torch.float64, min_gap=None):
    """language_tensor after one Adam step (torch.optim.Adam, weight_decay 0) per (x, lengths, labels); with min_gap the gap
    rule is asserted on the weights of every step"""
    Tt = _t(T, dtype).clone().requires_grad_(True)
    Wt, Ot, h0t, hTt = (_t(a, dtype) for a in (W, O, h0, hT))
    Pt = None if P is None else _t(P, dtype)
    opt = torch.optim.Adam([Tt], lr=lr, weight_decay=0)
    for x, lengths, labels in batches:
        if min_gap is not None:
            check_gap(Tt.detach(), Wt, Ot, h0t, hTt, x, lengths, mask=mask, min_gap=min_gap)
        opt.zero_grad()
        loss, _ = loss_and_pred(Tt, Wt, Ot, h0t, hTt, Pt, x, lengths, labels, 0.5, 0, mask=mask)
        loss.backward()
        opt.step()
    return Tt.detach().numpy()
