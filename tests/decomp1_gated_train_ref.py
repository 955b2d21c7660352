"""A torch restatement of the GATED decomposed independent=1 training step (FARNN_S_D_W_I, --farnn 1 | 2, sum semiring, CE1
loss or the CRF), written from the arithmetic, for the tests of farnn_decomp_ind1_gated_train_step.
Evaluates in the dtype it is asked for (float32 or float64), differentiates with autograd, and runs Adam for the multi-step
checks.  Everything the gates do not touch is decomp1_train_ref's (N, Osum, Mc, the scores, the loss, the decode) and
decomp1_crf_train_ref's (the CRF on top).

Reference citations (src_seq/farnn/model_decompose_independent.py):
  z    = sigmoid(k (h Wss1 + v Wrs1 + bs1))                  farnn 1, 2    :162, :164 (Sigmoidal: model_decompose.py:97-102)
  r    = sigmoid(k (h Wss2 + v Wrs2 + bs2))                  farnn 2       :165
  hbar = (1 - r) * h_init + r * h   (farnn 1: hbar = h)                    :161, :166     h_init = h0 (forward), hT (backward)
  y    = nl(hbar Mc_w)   (backward chain: hbar Mc_w^T; Wss untransposed in both chains)   :171-188
  h'   = (1 - z) * h + z * y                                               :193
The stash rows the scores read are the gated h'.

`fault` plants one wrong statement, for the tests that show the fixtures see it:
  'gates_on_hbar'   z's gate reads hbar instead of the raw h (farnn 2)
  'wss_transposed'  the backward chain reads Wss^T
  'no_k'            k dropped from the gates' derivative (the values are untouched)
  'dmc_with_h'      dMc takes h, not hbar, as its row factor (farnn 2; the values are untouched)
  'no_init_share'   the (1 - r) share of d h_init dropped (farnn 2; the values are untouched)
"""
import numpy as np
import torch

import decomp1_crf_train_ref as dcr
import decomp1_train_ref as dtr
from decomp1_train_ref import GapError, _ints, _params, _t, apply_nl, vgen_of

GATE_KEYS = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')
FAULTS = ('gates_on_hbar', 'wss_transposed', 'no_k', 'dmc_with_h', 'no_init_share')
FARNN2_ONLY = ('gates_on_hbar', 'dmc_with_h', 'no_init_share')
TRANS = dcr.TRANS


def gate_keys(farnn):
    return GATE_KEYS[:3 * farnn]


def _sig(a, k, fault):
    if fault == 'no_k':                                        # the value of sigmoid(k a), the derivative of sigmoid(k a0 + a)
        a0 = a.detach()
        return torch.sigmoid(k * a0 + (a - a0))
    return torch.sigmoid(k * a)


def _chain_step(h, h_init, Mw, gv1, gv2, p, farnn, k, nl, backward, fault):
    """h' and (pre-activation of the block product, the sum of its terms' magnitudes)"""
    W1 = p['Wss1'].t() if backward and fault == 'wss_transposed' else p['Wss1']
    hbar = h
    if farnn == 2:
        W2 = p['Wss2'].t() if backward and fault == 'wss_transposed' else p['Wss2']
        r = _sig(h @ W2 + gv2, k, fault)
        hi = h_init.detach() if fault == 'no_init_share' else h_init
        hbar = (1 - r) * hi + r * h
    z = _sig((hbar if fault == 'gates_on_hbar' else h) @ W1 + gv1, k, fault)
    if backward:
        Mw = Mw.transpose(1, 2)
    pre = torch.bmm(hbar.unsqueeze(1), Mw).squeeze(1)
    if fault == 'dmc_with_h':                                  # the value from hbar, d / d Mc from h
        wrong = torch.bmm(h.detach().unsqueeze(1), Mw).squeeze(1)
        pre = torch.bmm(hbar.unsqueeze(1), Mw.detach()).squeeze(1) + (wrong - wrong.detach())
    with torch.no_grad():
        mag = torch.bmm(hbar.abs().unsqueeze(1), Mw.abs()).squeeze(1)
    y = apply_nl(pre, nl)
    return (1 - z) * h + z * y, pre, mag


def forward(p, P, x, lengths, nl='none', add_nl='none', farnn=1, k=5.0, fault=None):
    """scores [B, L, C] (after the priority layer), valid [B, L], the block products' pre-activations [2, B, L, S] and the sums
    of their terms' magnitudes"""
    x, lengths = _ints(x), _ints(lengths)
    B, L = x.shape
    lens = lengths.clamp(0, L)
    v = vgen_of(p, add_nl)
    N = torch.einsum('wr,ir,jr->wij', v, p['S1'], p['S2']) + p['wildcard_mat']
    Osum = torch.einsum('r,ir,jr->ij', p['C_output'].sum(0), p['S1_output'], p['S2_output'])
    M = N * Osum
    GV1 = v @ p['Wrs1'] + p['bs1'].reshape(1, -1)
    GV2 = v @ p['Wrs2'] + p['bs2'].reshape(1, -1) if farnn == 2 else None
    idx = torch.arange(L)
    src = torch.where(idx[None, :] < lens[:, None], lens[:, None] - 1 - idx[None, :], idx[None, :])
    xr = torch.gather(x, 1, src)                               # reverse(x, len)
    h0, hT = p['h0'].expand(B, -1), p['hT'].expand(B, -1)
    f, b, pre, mag = [h0], [hT], [], []
    for t in range(L):
        wf, wb = x[:, t], xr[:, t]
        nf, pf, mf = _chain_step(f[-1], h0, M[wf], GV1[wf], None if GV2 is None else GV2[wf], p, farnn, k, nl, False, fault)
        nb, pb, mb = _chain_step(b[-1], hT, M[wb], GV1[wb], None if GV2 is None else GV2[wb], p, farnn, k, nl, True, fault)
        f.append(nf)
        b.append(nb)
        pre.append(torch.stack([pf, pb]))
        mag.append(torch.stack([mf, mb]))
    F, Bs = torch.stack(f, 1), torch.stack(b, 1)               # [B, L+1, S]: alpha_t, beta_{len-t}
    i = idx[None, :].expand(B, L)
    bidx = (lens[:, None] - 1 - i).clamp(min=0)
    alpha = F[:, :L]
    beta = torch.gather(Bs, 1, bidx.unsqueeze(-1).expand(B, L, Bs.shape[-1]))
    ab = (alpha[:, :, :, None] * beta[:, :, None, :]) * N[x]
    br = torch.einsum('blij,ir,jr->blr', ab, p['S1_output'], p['S2_output'])
    sc = br @ p['C_output'].t()
    if P is not None:
        sc = sc @ P
    return sc, i < lens[:, None], torch.stack(pre, 2), torch.stack(mag, 2)


def check_gap(p, P, x, lengths, nl='none', add_nl='none', farnn=1, k=5.0, threshold=0.5, o_idx=0, min_gap=2e-5, margin=1e-4,
              trans=None):
    """decomp1_train_ref.check_gap's rule on the gated chains (the block products' pre-activations of a relu / relutanh chain,
    the decode margins); with trans, decomp1_crf_train_ref's rule on the Viterbi path in their place"""
    x, lengths = _ints(x), _ints(lengths)
    L = x.shape[1]
    lens = lengths.clamp(0, L)
    t = torch.arange(L)[None, :]
    for dtype in (torch.float32, torch.float64):
        with torch.no_grad():
            sc, valid, pre, mag = forward(_params(p, dtype), None if P is None else _t(P, dtype), x, lens, nl=nl, add_nl=add_nl,
                                          farnn=farnn, k=k)
        if nl in ('relu', 'relutanh'):
            live = (t < lens[:, None] - 1)[None, :, :, None]
            bad = live & (pre != 0) & (pre.abs() < torch.clamp(8 * pre.shape[-1] * dtr.EPS32 * mag, min=min_gap))
            if bool(bad.any()):
                raise GapError('{} chain pre-activations within the gap of 0 in {}'.format(int(bad.sum()), dtype))
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
    sc, valid, _, _ = forward({q: v for q, v in pt.items() if q != TRANS}, Pt, x, lens, nl=nl, add_nl=add_nl, farnn=farnn, k=k,
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


def adam_steps(p, P, batches, trainable, nl='none', add_nl='none', farnn=1, k=5.0, lr=1e-3, dtype=torch.float64):
    """every tensor of p after one Adam step (torch.optim.Adam, weight_decay 0) per (x, lengths, labels); only the names in
    `trainable` move"""
    pt = {q: _t(a, dtype).clone().requires_grad_(q in trainable) for q, a in p.items()}
    Pt = None if P is None else _t(P, dtype)
    opt = torch.optim.Adam([pt[q] for q in p if q in trainable], lr=lr, weight_decay=0)
    for x, lengths, labels in batches:
        x, lengths, labels = _ints(x), _ints(lengths), _ints(labels)
        opt.zero_grad()
        loss, _ = _loss_and_pred(pt, Pt, x, lengths.clamp(0, x.shape[1]), labels, nl, add_nl, farnn, k, 0.5, 0, None)
        loss.backward()
        opt.step()
    return {q: t.detach().numpy() for q, t in pt.items()}


def gates_for(S, R, farnn, rng, scale=0.3, bias=0.2):
    """seeded gate tensors for the C-ABI cases: small enough (with k = 5) that the sigmoids stay away from saturation"""
    g = {}
    for n in range(1, farnn + 1):
        g['Wss%d' % n] = (rng.randn(S, S) * scale / np.sqrt(S)).astype(np.float32)
        g['Wrs%d' % n] = (rng.randn(R, S) * scale / np.sqrt(R)).astype(np.float32)
        g['bs%d' % n] = (rng.randn(S) * bias).astype(np.float32)
    return g
