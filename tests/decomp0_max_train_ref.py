"""A torch restatement of the decomposed FST's training step (FARNN_S_D_W) in the MAX semiring (--train_mode max), for the tests of
farnn_decomp_fst_train_step on a context switched by farnn_decomp_fst_train_set_semiring.  It is decomp0_train_ref.py's forward
with the two recurrences through first-index torch.max; the score head, the priority layer, the CE1 / CRF loss and the decode are
that module's, unchanged (the reference sends nothing else through _maxmul: model_decompose.py:269-276, utils.py:192-195).

  Rtab[w] = Vgen[w] * C_embed.sum(0);  W = S1w diag(C_wildcard.sum(0)) S2w^T + WW
  Tr_w[j, s] = sum_r S2[s, r] Rtab[w, r] S1[j, r] + W[j, s]
  forward chain   n[s] = max_j hbar[j] Tr_w[j, s]        backward chain  n[s] = max_j hbar[j] Tr_w[s, j]
  the gates read Rtab[w] (the reference's _R), as in the sum step

The gap rule (check_gap): max_chains_ref.check_argmax_gap on both chains with the project's MIN_GAP = 2e-5, in float32 and
float64 (a non-zero maximum beats the runner-up by MIN_GAP relative or ties it exactly in both; relu pre-activations are 0 or
MIN_GAP away from 0), and decomp0_train_ref's decode margin on the scores.

`fault` plants one of the faults the CPU tests show the captures can see:
  'sum'        sum chains in place of max chains
  'last'       the last maximal index in place of the first
  'no_transpose'  Tr not transposed in the backward chain
  'no_W'       W dropped from Tr
  'gates_v'    the gates fed V_vec in place of _R
"""
import numpy as np
import torch

import decomp0_train_ref as d0r
from decomp0_train_ref import (FLOAT_KEYS, GATE_KEYS, TRANS, VGEN_KEYS, GapError, _ints, _params, _t, apply_nl,  # noqa: F401
                               badly_drawn, crf_decode, crf_nll, gate_keys, signed_base, vgen_of)
from max_chains_ref import GapError as ChainGapError, _pick, check_argmax_gap, reversed_tokens

MIN_GAP = 2e-5
FAULTS = ('sum', 'last', 'no_transpose', 'no_W', 'gates_v')


def forward(p, P, x, lengths, nl='none', add_nl='none', farnn=0, k=5.0, fault=None, tops=None, pre=None):
    """scores [B, L, K] after the priority layer and valid [B, L]; tops / pre: lists filled as max_chains_ref.chains fills them"""
    x, lengths = _ints(x), _ints(lengths)
    B, L = x.shape
    lens = lengths.clamp(0, L)
    v = vgen_of(p, add_nl)
    rtab = v * p['C_embed'].sum(0)
    gin = v if fault == 'gates_v' else rtab
    W = (p['S1_wildcard'] * p['C_wildcard'].sum(0)) @ p['S2_wildcard'].t() + p['wildcard_wildcard']
    xr = reversed_tokens(x, lens)

    def step(h, hin, w, fwd):
        r = rtab[w]
        z = None
        if farnn >= 1:
            z = torch.sigmoid(k * (h @ p['Wss1'] + gin[w] @ p['Wrs1'] + p['bs1'].reshape(1, -1)))
        hbar = h
        if farnn == 2:
            g = torch.sigmoid(k * (h @ p['Wss2'] + gin[w] @ p['Wrs2'] + p['bs2'].reshape(1, -1)))
            hbar = (1 - g) * hin + g * h
        Tr = torch.einsum('sr,bjr->bjs', p['S2'], r[:, None, :] * p['S1'][None])       # [B, j, s]
        if fault != 'no_W':
            Tr = Tr + W
        if not fwd and fault != 'no_transpose':
            Tr = Tr.transpose(1, 2)
        cand = hbar.unsqueeze(2) * Tr
        if tops is not None and cand.shape[1] > 1:
            with torch.no_grad():
                top2.append(torch.topk(cand, 2, dim=1).values.transpose(0, 1))
        val, _ = _pick(cand, fault if fault in ('sum', 'last') else None)
        n = apply_nl(val, nl)
        return (n if z is None else (1 - z) * h + z * n), val

    h0, hT = p['h0'].expand(B, -1), p['hT'].expand(B, -1)
    f, b = [h0], [hT]
    for t in range(L):
        top2 = []
        nf, pf = step(f[-1], h0, x[:, t], True)
        nb, pb = step(b[-1], hT, xr[:, t], False)
        f.append(nf); b.append(nb)
        if tops is not None and top2:
            tops.append(torch.stack(top2))
        if pre is not None:
            pre.append(torch.stack([pf, pb]).detach())
    F, Bs = torch.stack(f, 1), torch.stack(b, 1)
    i = torch.arange(L)[None, :].expand(B, L)
    bidx = (lens[:, None] - 1 - i).clamp(min=0)
    alpha = F[:, :L]
    beta = torch.gather(Bs, 1, bidx.unsqueeze(-1).expand(B, L, Bs.shape[-1]))
    u = v[x] * (alpha @ p['S1']) * (beta @ p['S2'])
    uw = (alpha @ p['S1_wildcard']) * (beta @ p['S2_wildcard'])
    sc = u @ p['C_embed'].t() + uw @ p['C_wildcard'].t()
    if P is not None:
        sc = sc @ P
    return sc, i < lens[:, None]


def loss_and_pred(p, P, x, lengths, labels, nl, add_nl, threshold, o_idx, farnn=0, k=5.0, trans=None, fault=None):
    sc, valid = forward(p, P, x, lengths, nl=nl, add_nl=add_nl, farnn=farnn, k=k, fault=fault)
    lab = _ints(labels)
    lens = _ints(lengths).clamp(0, sc.shape[1])
    if trans is not None:
        loss = crf_nll(sc, lens, lab, trans)
        with torch.no_grad():
            pred = crf_decode(sc.detach(), lens, trans.detach(), threshold, o_idx)
        return loss, pred
    flat = sc[valid]
    loss = torch.nn.functional.cross_entropy(flat, lab[valid]) if flat.numel() else sc.sum() * 0
    with torch.no_grad():
        d = flat.clone()
        C = d.shape[1]
        d[:, C - 1] = torch.clamp(d[:, C - 1], max=threshold)
        pred = d.argmax(1)
        pred[pred == C - 1] = o_idx
    return loss, pred.numpy()


def step(p, P, x, lengths, labels, nl='none', add_nl='none', threshold=0.5, o_idx=0, dtype=torch.float64, farnn=0, k=5.0,
         trans=None, fault=None):
    """(loss, {name: gradient} for every float tensor of p and 'crf.transitions', flat_pred), evaluated in `dtype`"""
    pt = _params(p, dtype, grad=True)
    Pt = None if P is None else _t(P, dtype)
    tr = None if trans is None else _t(trans, dtype).clone().requires_grad_(True)
    loss, pred = loss_and_pred(pt, Pt, x, lengths, labels, nl, add_nl, threshold, o_idx, farnn=farnn, k=k, trans=tr, fault=fault)
    loss.backward()
    grads = {q: (t.grad.detach().numpy() if t.grad is not None else np.zeros(tuple(t.shape), t.detach().numpy().dtype))
             for q, t in pt.items()}
    if tr is not None:
        grads[TRANS] = tr.grad.detach().numpy() if tr.grad is not None else np.zeros(tuple(tr.shape), tr.detach().numpy().dtype)
    return float(loss.detach()), grads, pred


def check_gap(p, P, x, lengths, nl='none', add_nl='none', threshold=0.5, farnn=0, k=5.0, trans=None, min_gap=MIN_GAP, margin=1e-4):
    """Raises GapError unless the module docstring's rule holds"""
    x, lengths = _ints(x), _ints(lengths)
    L = x.shape[1]
    lens = lengths.clamp(0, L)
    scores = {}

    def run(dtype, tops, pre):
        scores[dtype] = forward(_params(p, dtype), None if P is None else _t(P, dtype), x, lens, nl=nl, add_nl=add_nl, farnn=farnn,
                                k=k, tops=tops, pre=pre)
    try:
        check_argmax_gap(run, x, lens, min_gap=min_gap, relu=nl in ('relu', 'relutanh'))
    except ChainGapError as e:
        raise GapError(str(e))
    paths = []
    for dtype in (torch.float32, torch.float64):
        sc, valid = scores[dtype]
        if trans is not None:
            paths.append(crf_decode(sc, lens, _t(trans, dtype), threshold, 0))
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
    if trans is not None and not np.array_equal(paths[0], paths[1]):
        raise GapError('the float32 and float64 Viterbi paths differ')
