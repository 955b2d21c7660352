"""A torch restatement of the decomposed independent=1 training step in the MAX semiring (FARNN_S_D_W_I, farnn = 0,
--train_mode max, CE1), written from the arithmetic, for the tests of farnn_decomp_ind1_train_step after
farnn_decomp_ind1_train_set_semiring(MAX).  The chains are max_chains_ref.chains on Mc_w = N_w * Osum with update_nonlinear
(src_seq/farnn/model_decompose_independent.py:174-188); N, Osum, br, the score, the priority layer, the loss and the decode
are the sum step's (decomp1_train_ref.py), restated on the max chains' states.  Evaluates in float32 or float64 and
differentiates with autograd.  `fault`: max_chains_ref's planted faults."""
import numpy as np
import torch

import max_chains_ref as mc
from decomp1_train_ref import FLOAT_KEYS, VGEN_KEYS, _ints, _params, _t, apply_nl, signed_base, vgen_of  # noqa: F401
from max_chains_ref import GapError  # noqa: F401


def forward(p, P, x, lengths, nl='none', add_nl='none', fault=None, tops=None, pre=None):
    """scores [B, L, C] (after the priority layer), valid [B, L]"""
    x, lengths = _ints(x), _ints(lengths)
    lens = lengths.clamp(0, x.shape[1])
    v = vgen_of(p, add_nl)
    # N and Osum as sums over the rank of elementwise products, r ascending: every entry goes through the same correctly rounded
    # operations in the same order, so two states with identical factor rows (the fixtures' planted twin) give bit-identical
    # entries of Mc in either dtype on any machine -- a blocked einsum may round the entries of one row differently, and the
    # arg-max of an exact tie must not hang on that
    N, Osum = p['wildcard_mat'].expand(v.shape[0], -1, -1), 0.0
    for r in range(v.shape[1]):
        N = N + v[:, r, None, None] * (p['S1'][:, r, None] * p['S2'][None, :, r])
    csum = p['C_output'].sum(0)
    for r in range(csum.shape[0]):
        Osum = Osum + csum[r] * (p['S1_output'][:, r, None] * p['S2_output'][None, :, r])
    M = N * Osum
    F, Bs = mc.chains(M, p['h0'], p['hT'], x, lens, lambda a: apply_nl(a, nl), fault=fault, tops=tops, pre=pre)
    alpha, beta, valid = mc.states_at_positions(F, Bs, lens)
    ab = (alpha[:, :, :, None] * beta[:, :, None, :]) * N[x]   # [B, L, S, S]
    br = torch.einsum('blij,ir,jr->blr', ab, p['S1_output'], p['S2_output'])
    sc = br @ p['C_output'].t()
    if P is not None:
        sc = sc @ P
    return sc, valid


def check_gap(p, P, x, lengths, nl='none', add_nl='none', min_gap=2e-5, relu_gap=None):
    """the arg-max rule (min_gap, relative) and, for the relu chains, the relu rule on the chain pre-activations (relu_gap,
    absolute; min_gap when not given)"""
    x, lengths = _ints(x), _ints(lengths)
    lens = lengths.clamp(0, x.shape[1])
    mc.check_argmax_gap(lambda dtype, tops, pre: forward(_params(p, dtype), None, x, lens, nl=nl, add_nl=add_nl, tops=tops,
                                                         pre=pre), x, lens, min_gap, relu=nl in ('relu', 'relutanh'),
                        relu_gap=relu_gap)


def loss_and_pred(p, P, x, lengths, labels, nl, add_nl, threshold, o_idx, fault=None):
    sc, valid = forward(p, P, x, lengths, nl=nl, add_nl=add_nl, fault=fault)
    flat = sc[valid]
    loss = torch.nn.functional.cross_entropy(flat, _ints(labels)[valid])
    with torch.no_grad():
        d = flat.clone()
        C = d.shape[1]
        d[:, C - 1] = torch.clamp(d[:, C - 1], max=threshold)
        pred = d.argmax(1)
        pred[pred == C - 1] = o_idx
    return loss, pred.numpy()


def step(p, P, x, lengths, labels, nl='none', add_nl='none', threshold=0.5, o_idx=0, dtype=torch.float64, fault=None):
    """(loss, {name: gradient} for every float tensor of p, flat_pred) of one training step, evaluated in `dtype`."""
    pt = _params(p, dtype, grad=True)
    Pt = None if P is None else _t(P, dtype)
    loss, pred = loss_and_pred(pt, Pt, x, lengths, labels, nl, add_nl, threshold, o_idx, fault=fault)
    loss.backward()
    grads = {k: (t.grad.detach().numpy() if t.grad is not None else np.zeros(tuple(t.shape), t.detach().numpy().dtype))
             for k, t in pt.items()}
    return float(loss.detach()), grads, pred


def adam_steps(p, P, batches, trainable, nl='none', add_nl='none', lr=1e-3, dtype=torch.float64, min_gap=None):
    """every tensor of p after one Adam step (torch.optim.Adam, weight_decay 0) per (x, lengths, labels)"""
    pt = {k: _t(a, dtype).clone().requires_grad_(k in trainable) for k, a in p.items()}
    Pt = None if P is None else _t(P, dtype)
    opt = torch.optim.Adam([pt[k] for k in p if k in trainable], lr=lr, weight_decay=0)
    for x, lengths, labels in batches:
        if min_gap is not None:
            check_gap({k: t.detach() for k, t in pt.items()}, None, x, lengths, nl=nl, add_nl=add_nl, min_gap=min_gap)
        opt.zero_grad()
        loss, _ = loss_and_pred(pt, Pt, x, lengths, labels, nl, add_nl, 0.5, 0)
        loss.backward()
        opt.step()
    return {k: t.detach().numpy() for k, t in pt.items()}
