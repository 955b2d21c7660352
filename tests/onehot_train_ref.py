"""A torch restatement of the onehot i-FST training step (FARNN_S_O_I_S, sum semiring, CE1 loss), written from the
arithmetic, for the tests of farnn_onehot_ifst_train_step.  Evaluates in the dtype of its inputs (float32 or float64),
differentiates with autograd, and runs Adam for the multi-step checks.

Reference citations (src_seq/farnn/model_onehot.py unless noted):
  M_w = T[w] + W                                   :370
  o = output_mat.sum(0)                            :372 (CE1)
  forward chain  f_t = nl((f_{t-1} M_{x_t}) * o)   :376-387, f_0 = h0 :358
  backward chain b_t = nl((b_{t-1} * o) M_{x'_t}^T), x' = reverse(x, len)  :390-401, b_0 = hT :359
  score_i = output_mat (f_{i+1} * b_{len-1-i})     :339-342, :404-424 (beta = reverse([hT, b_1..], len+1)[i+1])
  priority: score @ P                              :425-426, priority.py
  loss = CrossEntropyLoss(mean) over valid tokens  :131-146, :61-64
  decode: column C-1 clamped to threshold, argmax, C-1 -> o_idx   :162-180
"""
import numpy as np
import torch


def _nl(v, nl):
    if nl == 'relu':
        return torch.relu(v)
    if nl == 'tanh':
        return torch.tanh(v)
    if nl == 'relutanh':
        return torch.tanh(torch.relu(v))
    return v


def _t(a, dtype):
    return a.to(dtype) if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)).to(dtype)


def scores_and_pre(T, W, O, h0, hT, P, x, lengths, nl):
    """scores [B, L, C] (rows past a sequence's length are zero) and the pre-activations of both chains [2, B, L, S]."""
    x = torch.as_tensor(np.asarray(x)) if not torch.is_tensor(x) else x
    lengths = torch.as_tensor(np.asarray(lengths)) if not torch.is_tensor(lengths) else lengths
    B, L = x.shape
    lens = lengths.clamp(0, L)
    M = T + W
    o = O.sum(0)
    idx = torch.arange(L)
    # reverse(x, len): the first len tokens of a row reversed, the pads where they were
    src = torch.where(idx[None, :] < lens[:, None], lens[:, None] - 1 - idx[None, :], idx[None, :])
    xr = torch.gather(x, 1, src)
    f, b = [h0.expand(B, -1)], [hT.expand(B, -1)]
    pre = []
    for t in range(L):
        pf = torch.bmm(f[-1].unsqueeze(1), M[x[:, t]]).squeeze(1) * o
        pb = torch.bmm((b[-1] * o).unsqueeze(1), M[xr[:, t]].transpose(1, 2)).squeeze(1)
        pre.append(torch.stack([pf, pb]))
        f.append(_nl(pf, nl))
        b.append(_nl(pb, nl))
    F, Bs = torch.stack(f, 1), torch.stack(b, 1)           # [B, L+1, S]
    i = idx[None, :].expand(B, L)
    bidx = (lens[:, None] - 1 - i).clamp(min=0)
    alpha = F[:, 1:]
    beta = torch.gather(Bs, 1, bidx.unsqueeze(-1).expand(B, L, Bs.shape[-1]))
    sc = torch.einsum('cs,bls->blc', O, alpha * beta)
    if P is not None:
        sc = sc @ P
    valid = i < lens[:, None]
    sc = sc * valid.unsqueeze(-1).to(sc.dtype)
    return sc, valid, torch.stack(pre, 2)


def step(T, W, O, h0, hT, P, x, lengths, labels, nl='none', threshold=0.5, o_idx=0, dtype=torch.float64):
    """(loss, dT, flat_pred) of one training step, evaluated in `dtype`."""
    Tt = _t(T, dtype).clone().requires_grad_(True)
    Wt, Ot, h0t, hTt = (_t(a, dtype) for a in (W, O, h0, hT))
    Pt = None if P is None else _t(P, dtype)
    loss, pred = loss_and_pred(Tt, Wt, Ot, h0t, hTt, Pt, x, lengths, labels, nl, threshold, o_idx)
    loss.backward()
    return float(loss.detach()), Tt.grad.detach().numpy(), pred


def loss_and_pred(T, W, O, h0, hT, P, x, lengths, labels, nl, threshold, o_idx):
    sc, valid, _ = scores_and_pre(T, W, O, h0, hT, P, x, lengths, nl)
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


def adam_steps(T, W, O, h0, hT, P, batches, nl='none', lr=1e-3, dtype=torch.float64):
    """language_tensor after one Adam step (torch.optim.Adam, weight_decay 0) per (x, lengths, labels) of `batches`."""
    Tt = _t(T, dtype).clone().requires_grad_(True)
    Wt, Ot, h0t, hTt = (_t(a, dtype) for a in (W, O, h0, hT))
    Pt = None if P is None else _t(P, dtype)
    opt = torch.optim.Adam([Tt], lr=lr, weight_decay=0)
    for x, lengths, labels in batches:
        opt.zero_grad()
        loss, _ = loss_and_pred(Tt, Wt, Ot, h0t, hTt, Pt, x, lengths, labels, nl, 0.5, 0)
        loss.backward()
        opt.step()
    return Tt.detach().numpy()
