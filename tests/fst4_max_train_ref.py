"""A torch restatement of the onehot FST training step in the MAX semiring (FARNN_S_O, --train_mode max, CE1), written from
the arithmetic, for the tests of farnn_fst4_train_step after farnn_fst4_train_set_semiring(MAX).  The chains are
max_chains_ref.chains on M_w = language_tensor.sum(1)[w] + wildcard_tensor.sum(0) with relu (src_seq/farnn/model_onehot.py:82,
:89-102); the score with its relu, the priority layer, the loss and the decode are the sum step's (fst4_train_ref.py:
:115-127, :131-180), restated on the max chains' states.  Evaluates in float32 or float64 and differentiates with autograd.
`fault`: max_chains_ref's planted faults."""
import torch

import max_chains_ref as mc
from fst4_train_ref import _ints, _t, signed_base  # noqa: F401
from max_chains_ref import GapError


def forward(T4, W4, h0, hT, P, x, lengths, fault=None, tops=None, pre=None):
    """scores [B, L, C] (after the priority layer), valid [B, L], the score products [B, L, C, S, S]"""
    x, lengths = _ints(x), _ints(lengths)
    lens = lengths.clamp(0, x.shape[1])
    M = T4.sum(1) + W4.sum(0)
    A = T4 + W4
    F, Bs = mc.chains(M, h0, hT, x, lens, torch.relu, fault=fault, tops=tops, pre=pre)
    alpha, beta, valid = mc.states_at_positions(F, Bs, lens)
    prod = (A[x] * alpha[:, :, None, :, None]) * beta[:, :, None, None, :]
    sc = torch.relu(prod).sum(dim=(3, 4))
    if P is not None:
        sc = sc @ P
    return sc, valid, prod


def check_gap(T4, W4, h0, hT, x, lengths, min_gap=2e-5):
    """the arg-max rule, and the sum fixtures' relu rule on the chain pre-activations and on the score products"""
    x, lengths = _ints(x), _ints(lengths)
    lens = lengths.clamp(0, x.shape[1])
    prods = {}

    def run(dtype, tops, pre):
        _, valid, prod = forward(*(_t(a, dtype) for a in (T4, W4, h0, hT)), None, x, lens, tops=tops, pre=pre)
        prods[dtype] = (valid, prod)
    mc.check_argmax_gap(run, x, lens, min_gap)
    for dtype, (valid, prod) in prods.items():
        bad = valid[:, :, None, None, None] & (prod != 0) & (prod.abs() < min_gap)
        if bool(bad.any()):
            raise GapError('{} score products within {} of 0 in {}'.format(int(bad.sum()), min_gap, dtype))


def loss_and_pred(T4, W4, h0, hT, P, x, lengths, labels, threshold, o_idx, fault=None):
    sc, valid, _ = forward(T4, W4, h0, hT, P, x, lengths, fault=fault)
    flat = sc[valid]
    loss = torch.nn.functional.cross_entropy(flat, _ints(labels)[valid])
    with torch.no_grad():
        d = flat.clone()
        C = d.shape[1]
        d[:, C - 1] = torch.clamp(d[:, C - 1], max=threshold)
        pred = d.argmax(1)
        pred[pred == C - 1] = o_idx
    return loss, pred.numpy()


def step(T4, W4, h0, hT, P, x, lengths, labels, threshold=0.5, o_idx=0, dtype=torch.float64, fault=None):
    """(loss, dT4, dW4, flat_pred) of one training step, evaluated in `dtype`."""
    Tt = _t(T4, dtype).clone().requires_grad_(True)
    Wt = _t(W4, dtype).clone().requires_grad_(True)
    h0t, hTt = _t(h0, dtype), _t(hT, dtype)
    Pt = None if P is None else _t(P, dtype)
    loss, pred = loss_and_pred(Tt, Wt, h0t, hTt, Pt, x, lengths, labels, threshold, o_idx, fault=fault)
    loss.backward()
    return float(loss.detach()), Tt.grad.detach().numpy(), Wt.grad.detach().numpy(), pred


def adam_steps(T4, W4, h0, hT, P, batches, train_wildcard=False, lr=1e-3, dtype=torch.float64, min_gap=None):
    """(language_tensor, wildcard_tensor) after one Adam step (torch.optim.Adam, weight_decay 0) per (x, lengths, labels)"""
    Tt = _t(T4, dtype).clone().requires_grad_(True)
    Wt = _t(W4, dtype).clone().requires_grad_(bool(train_wildcard))
    h0t, hTt = _t(h0, dtype), _t(hT, dtype)
    Pt = None if P is None else _t(P, dtype)
    opt = torch.optim.Adam([Tt] + ([Wt] if train_wildcard else []), lr=lr, weight_decay=0)
    for x, lengths, labels in batches:
        if min_gap is not None:
            check_gap(Tt.detach(), Wt.detach(), h0t, hTt, x, lengths, min_gap=min_gap)
        opt.zero_grad()
        loss, _ = loss_and_pred(Tt, Wt, h0t, hTt, Pt, x, lengths, labels, 0.5, 0)
        loss.backward()
        opt.step()
    return Tt.detach().numpy(), Wt.detach().numpy()
