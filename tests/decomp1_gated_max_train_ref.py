"""A torch restatement of the GATED decomposed independent=1 training step in the MAX semiring (FARNN_S_D_W_I, --farnn 1 | 2
--train_mode max, CE1 loss or the CRF), written from the arithmetic, for the tests of
farnn_decomp_ind1_gated_max_train_step.  Evaluates in the dtype it is asked for (float32 or float64), differentiates with
autograd, and runs Adam for the multi-step checks.  Everything the chains do not touch is decomp1_train_ref's (the scores, the
loss, the decode) and decomp1_crf_train_ref's (the CRF on top); the gate tensors are decomp1_gated_train_ref's.

Reference (src_seq/farnn/model_decompose_independent.py:148-197, utils.py:192-195): only the two block products go through
semiring_func; the gate products stay ordinary matrix products.
  z    = sigmoid(k (h Wss1 + v Wrs1 + bs1))                  farnn 1, 2    (sum-times)
  r    = sigmoid(k (h Wss2 + v Wrs2 + bs2))                  farnn 2       (sum-times)
  hbar = (1 - r) * h_init + r * h   (farnn 1: hbar = h)                    h_init = h0 (forward), hT (backward)
  q[s] = max_j hbar[j] Mc_w[j, s]   (backward chain: max_j hbar[j] Mc_w[s, j]), the FIRST maximal j (torch.max(dim=1))
  y    = nl(q);   h' = (1 - z) * h + z * y
N, Osum and the gate products are written as sums of elementwise products in a fixed order (decomp1_max_train_ref.forward says
why): two states with identical rows and columns in every tensor stay bit-identical in either dtype, and the fixtures' planted
twin ties exactly.

`fault` plants one wrong statement, for the tests that show the fixtures see it:
  'sum'            sum chains in place of max chains
  'last'           the last maximal index in place of the first
  'fwd_idx'        the forward chain's index used for the backward chain
  'gates_max'      the gate products h Wss sent through max-times as well
  'no_init_share'  the (1 - r) share of d h_init dropped (farnn 2; the values are untouched)
  'no_carry0'      the first chain step carries nothing back into h0 / hT (the values are untouched)
"""
import numpy as np
import torch

import decomp1_crf_train_ref as dcr
import max_chains_ref as mc
from decomp1_gated_train_ref import GATE_KEYS, TRANS, gate_keys, gates_for  # noqa: F401
from decomp1_train_ref import _ints, _params, _t, apply_nl, vgen_of
from max_chains_ref import GapError

FAULTS = ('sum', 'last', 'fwd_idx', 'gates_max', 'no_init_share', 'no_carry0')
FARNN2_ONLY = ('no_init_share',)


def _gate(h, W, gv, k, fault):
    cand = h.unsqueeze(2) * W                                  # [B, j, s] = h[j] Wss[j, s]
    a = cand.max(1)[0] if fault == 'gates_max' else cand.sum(1)
    return torch.sigmoid(k * (a + gv))


def _chain_step(h, h_init, Mw, gv1, gv2, p, farnn, k, nl, backward, fault, other_idx=None):
    """h', the block product's candidates [B, j, s], its value and its index"""
    hbar = h
    if farnn == 2:
        r = _gate(h, p['Wss2'], gv2, k, fault)
        hi = h_init.detach() if fault == 'no_init_share' else h_init
        hbar = (1 - r) * hi + r * h
    z = _gate(h, p['Wss1'], gv1, k, fault)
    cand = hbar.unsqueeze(2) * (Mw.transpose(1, 2) if backward else Mw)
    q, idx = mc._pick(cand, fault if fault in ('sum', 'last') else None, other_idx=other_idx)
    return (1 - z) * h + z * apply_nl(q, nl), cand, q, idx


def forward(p, P, x, lengths, nl='none', add_nl='none', farnn=1, k=5.0, fault=None, tops=None, pre=None):
    """scores [B, L, C] (after the priority layer), valid [B, L].  tops / pre: max_chains_ref.chains' lists"""
    x, lengths = _ints(x), _ints(lengths)
    B, L = x.shape
    lens = lengths.clamp(0, L)
    v = vgen_of(p, add_nl)
    N, Osum = p['wildcard_mat'].expand(v.shape[0], -1, -1), 0.0
    for r in range(v.shape[1]):
        N = N + v[:, r, None, None] * (p['S1'][:, r, None] * p['S2'][None, :, r])
    csum = p['C_output'].sum(0)
    for r in range(csum.shape[0]):
        Osum = Osum + csum[r] * (p['S1_output'][:, r, None] * p['S2_output'][None, :, r])
    M = N * Osum
    GV1 = (v.unsqueeze(2) * p['Wrs1']).sum(1) + p['bs1'].reshape(1, -1)
    GV2 = (v.unsqueeze(2) * p['Wrs2']).sum(1) + p['bs2'].reshape(1, -1) if farnn == 2 else None
    xr = mc.reversed_tokens(x, lens)
    h0, hT = p['h0'].expand(B, -1), p['hT'].expand(B, -1)
    f, b = [h0], [hT]
    for t in range(L):
        wf, wb = x[:, t], xr[:, t]
        inf, inb = (f[-1].detach(), b[-1].detach()) if fault == 'no_carry0' and t == 0 else (f[-1], b[-1])
        nf, cf, pf, jf = _chain_step(inf, h0, M[wf], GV1[wf], None if GV2 is None else GV2[wf], p, farnn, k, nl, False, fault)
        nb, cb, pb, _ = _chain_step(inb, hT, M[wb], GV1[wb], None if GV2 is None else GV2[wb], p, farnn, k, nl, True, fault,
                                    other_idx=jf if fault == 'fwd_idx' else None)
        if tops is not None and cf.shape[1] > 1:
            with torch.no_grad():
                tops.append(torch.stack([torch.topk(cf, 2, dim=1).values.transpose(0, 1),
                                         torch.topk(cb, 2, dim=1).values.transpose(0, 1)]))
        if pre is not None:
            pre.append(torch.stack([pf, pb]).detach())
        f.append(nf)
        b.append(nb)
    alpha, beta, valid = mc.states_at_positions(torch.stack(f, 1), torch.stack(b, 1), lens)
    ab = (alpha[:, :, :, None] * beta[:, :, None, :]) * N[x]
    br = torch.einsum('blij,ir,jr->blr', ab, p['S1_output'], p['S2_output'])
    sc = br @ p['C_output'].t()
    if P is not None:
        sc = sc @ P
    return sc, valid


def check_gap(p, P, x, lengths, nl='none', add_nl='none', farnn=1, k=5.0, threshold=0.5, o_idx=0, min_gap=2e-5, relu_gap=None,
              margin=1e-4, trans=None):
    """max_chains_ref's arg-max rule on the gated chains at every step, in float32 and float64 (relu / relutanh: with the relu
    rule on the block products' values), then the decode rule of decomp1_gated_train_ref.check_gap: the margins of the arg-max
    decode, or with trans decomp1_crf_train_ref's rule on the Viterbi path."""
    x, lengths = _ints(x), _ints(lengths)
    lens = lengths.clamp(0, x.shape[1])
    Pt = {dt: None if P is None else _t(P, dt) for dt in (torch.float32, torch.float64)}
    out = {}

    def run(dtype, tops, pre):
        out[dtype] = forward(_params(p, dtype), Pt[dtype], x, lens, nl=nl, add_nl=add_nl, farnn=farnn, k=k, tops=tops, pre=pre)
    mc.check_argmax_gap(run, x, lens, min_gap, relu=nl in ('relu', 'relutanh'), relu_gap=relu_gap)
    for dtype, (sc, valid) in out.items():
        if trans is not None:
            if dtype == torch.float64:
                dcr.viterbi(sc.numpy(), np.asarray(trans, np.float64), lens.numpy(), threshold, o_idx, check=True,
                            min_gap=max(min_gap, 2e-5), margin=margin)
            continue
        flat = sc[valid]
        if flat.numel():
            C = flat.shape[1]
            last = flat[:, C - 1]
            d = flat.clone()
            d[:, C - 1] = torch.clamp(last, max=threshold)
            if C > 1:
                top = d.topk(2, dim=1).values
                gap = top[:, 0] - top[:, 1]
                if bool(((gap != 0) & (gap < margin * (1 + top[:, 0].abs()))).any()):
                    raise GapError('positions whose top two scores are within the margin in {}'.format(dtype))
            if bool(((last - threshold).abs() < margin * (1 + abs(threshold))).any()):
                raise GapError('positions whose last column sits at the threshold clamp in {}'.format(dtype))


def _loss_and_pred(pt, Pt, x, lens, labels, nl, add_nl, farnn, k, threshold, o_idx, fault):
    sc, valid = forward({q: v for q, v in pt.items() if q != TRANS}, Pt, x, lens, nl=nl, add_nl=add_nl, farnn=farnn, k=k,
                        fault=fault)
    if TRANS in pt:
        loss = dcr.crf_nll(sc, pt[TRANS], lens, labels)
        return loss, dcr.viterbi(sc.detach().numpy(), pt[TRANS].detach().numpy(), lens.numpy(), threshold, o_idx)
    flat = sc[valid]
    loss = torch.nn.functional.cross_entropy(flat, labels[valid])
    with torch.no_grad():
        d = flat.clone()
        C = d.shape[1]
        d[:, C - 1] = torch.clamp(d[:, C - 1], max=threshold)
        pred = d.argmax(1)
        pred[pred == C - 1] = o_idx
    return loss, pred.numpy()


def step(p, P, x, lengths, labels, nl='none', add_nl='none', farnn=1, k=5.0, threshold=0.5, o_idx=0, dtype=torch.float64,
         trans=None, fault=None):
    """(loss, {name: gradient} for every float tensor of p (and 'crf.transitions' with trans), flat_pred) of one training step
    in `dtype`.  p: 'Vgen' or decomp1_train_ref.VGEN_KEYS, decomp1_train_ref.FLOAT_KEYS and gate_keys(farnn)."""
    x, lengths, labels = _ints(x), _ints(lengths), _ints(labels)
    lens = lengths.clamp(0, x.shape[1])
    pt = _params(p if trans is None else dict(p, **{TRANS: trans}), dtype, grad=True)
    Pt = None if P is None else _t(P, dtype)
    loss, pred = _loss_and_pred(pt, Pt, x, lens, labels, nl, add_nl, farnn, k, threshold, o_idx, fault)
    loss.backward()
    grads = {q: (t.grad.detach().numpy() if t.grad is not None else np.zeros(tuple(t.shape), t.detach().numpy().dtype))
             for q, t in pt.items()}
    return float(loss.detach()), grads, pred


def adam_steps(p, P, batches, trainable, nl='none', add_nl='none', farnn=1, k=5.0, lr=1e-3, dtype=torch.float64, min_gap=None):
    """every tensor of p after one Adam step (torch.optim.Adam, weight_decay 0) per (x, lengths, labels); only the names in
    `trainable` move.  min_gap: the arg-max rule is checked before every step."""
    pt = {q: _t(a, dtype).clone().requires_grad_(q in trainable) for q, a in p.items()}
    Pt = None if P is None else _t(P, dtype)
    opt = torch.optim.Adam([pt[q] for q in p if q in trainable], lr=lr, weight_decay=0)
    for x, lengths, labels in batches:
        x, lengths, labels = _ints(x), _ints(lengths), _ints(labels)
        if min_gap is not None:
            check_gap({q: t.detach().numpy() for q, t in pt.items()}, None, x, lengths, nl=nl, add_nl=add_nl, farnn=farnn, k=k,
                      min_gap=min_gap, margin=0.0)
        opt.zero_grad()
        loss, _ = _loss_and_pred(pt, Pt, x, lengths.clamp(0, x.shape[1]), labels, nl, add_nl, farnn, k, 0.5, 0, None)
        loss.backward()
        opt.step()
    return {q: t.detach().numpy() for q, t in pt.items()}
