"""A torch restatement of the onehot independent=1 training step (FARNN_S_O_I, sum semiring, CE1 loss), written from the
arithmetic, for the tests of farnn_ind1_train_step.  Evaluates in the dtype it is asked for (float32 or float64),
differentiates with autograd, and runs Adam for the multi-step checks.

Reference citations (src_seq/farnn/model_onehot.py):
  N_w = language_tensor[w] + wildcard_mat                           :250
  Osum = output_tensor.sum(0)                                       :252 (CE1: output_wildcard_mat is not read)
  Mc_w = N_w * Osum if args.independent == 2 else N_w               :259-262, :271-274
  forward chain  alpha_{i+1} = relu(alpha_i Mc_{x_i}), alpha_0 = h0 :264-267 (always relu)
  backward chain beta_i = relu(Mc_{x_i} beta_{i+1}), beta_n = hT    :276-279
  score_i[c] = sum_{s,j} O[c,s,j] alpha_i[s] beta_{i+1}[j] N_{x_i}[s,j]   :229-233, :293-299 (alpha_i: the state BEFORE
                                                                    token i; N, not Mc; no relu)
  priority: score @ P                                               :301-302
  loss = CrossEntropyLoss(mean) over valid tokens                   :131-146, :59-60
  decode: column C-1 clamped to threshold, argmax, C-1 -> o_idx     :162-180

The gap rule (check_gap): every chain pre-activation that can reach a score is exactly 0 or at least min_gap away from 0,
in float32 and in float64, so that no relu decision of the step can be reversed by float32 rounding (the gradient is
discontinuous there: a reversed decision is a different function).  The score has no relu: only the chains need the gap.
"""
import numpy as np
import torch


class GapError(AssertionError):
    pass


def _t(a, dtype):
    return a.to(dtype) if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)).to(dtype)


def _ints(a):
    return a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))


def forward(T, W, O, h0, hT, P, x, lengths, mask=False):
    """scores [B, L, C] (after the priority layer), valid [B, L], chain pre-activations [2, B, L, S]"""
    x, lengths = _ints(x), _ints(lengths)
    B, L = x.shape
    lens = lengths.clamp(0, L)
    N = T + W
    M = N * O.sum(0) if mask else N
    idx = torch.arange(L)
    src = torch.where(idx[None, :] < lens[:, None], lens[:, None] - 1 - idx[None, :], idx[None, :])
    xr = torch.gather(x, 1, src)                               # reverse(x, len)
    f, b, pre = [h0.expand(B, -1)], [hT.expand(B, -1)], []
    for t in range(L):
        pf = torch.bmm(f[-1].unsqueeze(1), M[x[:, t]]).squeeze(1)
        pb = torch.bmm(b[-1].unsqueeze(1), M[xr[:, t]].transpose(1, 2)).squeeze(1)
        pre.append(torch.stack([pf, pb]))
        f.append(torch.relu(pf))
        b.append(torch.relu(pb))
    F, Bs = torch.stack(f, 1), torch.stack(b, 1)               # [B, L+1, S]: alpha_t, beta_{len-t}
    i = idx[None, :].expand(B, L)
    bidx = (lens[:, None] - 1 - i).clamp(min=0)
    alpha = F[:, :L]
    beta = torch.gather(Bs, 1, bidx.unsqueeze(-1).expand(B, L, Bs.shape[-1]))
    ab = (alpha[:, :, :, None] * beta[:, :, None, :]) * N[x]   # [B, L, S, S]
    sc = torch.einsum('csj,blsj->blc', O, ab)
    if P is not None:
        sc = sc @ P
    valid = i < lens[:, None]
    return sc, valid, torch.stack(pre, 2)


def check_gap(T, W, O, h0, hT, x, lengths, mask=False, min_gap=2e-5):
    """Raises GapError unless the rule of the module docstring holds on these inputs."""
    x, lengths = _ints(x), _ints(lengths)
    L = x.shape[1]
    lens = lengths.clamp(0, L)
    t = torch.arange(L)[None, :]
    for dtype in (torch.float32, torch.float64):
        with torch.no_grad():
            _, _, pre = forward(*(_t(a, dtype) for a in (T, W, O, h0, hT)), None, x, lens, mask=mask)
        live = (t < lens[:, None] - 1)[None, :, :, None]          # alpha_len and beta_0 feed nothing
        bad = live & (pre != 0) & (pre.abs() < min_gap)
        if bool(bad.any()):
            raise GapError('{} chain pre-activations within {} of 0 in {}'.format(int(bad.sum()), min_gap, dtype))


def loss_and_pred(T, W, O, h0, hT, P, x, lengths, labels, threshold, o_idx, mask=False):
    sc, valid, _ = forward(T, W, O, h0, hT, P, x, lengths, mask=mask)
    lab = _ints(labels)
    flat = sc[valid]
    loss = torch.nn.functional.cross_entropy(flat, lab[valid])
    with torch.no_grad():
        d = flat.clone()
        C = d.shape[1]
        d[:, C - 1] = torch.clamp(d[:, C - 1], max=threshold)
        pred = d.argmax(1)
        pred[pred == C - 1] = o_idx
    return loss, pred.numpy()


def step(T, W, O, h0, hT, P, x, lengths, labels, mask=False, threshold=0.5, o_idx=0, dtype=torch.float64):
    """(loss, dT, flat_pred) of one training step, evaluated in `dtype`."""
    Tt = _t(T, dtype).clone().requires_grad_(True)
    Wt, Ot, h0t, hTt = (_t(a, dtype) for a in (W, O, h0, hT))
    Pt = None if P is None else _t(P, dtype)
    loss, pred = loss_and_pred(Tt, Wt, Ot, h0t, hTt, Pt, x, lengths, labels, threshold, o_idx, mask=mask)
    loss.backward()
    return float(loss.detach()), Tt.grad.detach().numpy(), pred


def adam_steps(T, W, O, h0, hT, P, batches, mask=False, lr=1e-3, dtype=torch.float64):
    """language_tensor after one Adam step (torch.optim.Adam, weight_decay 0) per (x, lengths, labels)"""
    Tt = _t(T, dtype).clone().requires_grad_(True)
    Wt, Ot, h0t, hTt = (_t(a, dtype) for a in (W, O, h0, hT))
    Pt = None if P is None else _t(P, dtype)
    opt = torch.optim.Adam([Tt], lr=lr, weight_decay=0)
    for x, lengths, labels in batches:
        opt.zero_grad()
        loss, _ = loss_and_pred(Tt, Wt, Ot, h0t, hTt, Pt, x, lengths, labels, 0.5, 0, mask=mask)
        loss.backward()
        opt.step()
    return Tt.detach().numpy()


def signed_base(V, S, C, rng, density=None):
    """Signed real-valued tensors on which the gap rule holds by construction for short sequences: sparse blocks whose
    entries are multiples of 1/4 in [-1, 1.25] (every chain value is then a small dyadic rational, exact in float32 and in
    float64, as long as the sequences stay a few tokens long).  output_tensor is signed as well: about two labels per
    (s, j) entry, so that the masked chains (N * Osum) stay alive."""
    density = density if density is not None else min(0.5, 3.0 / S)            # |N| rows sum to about 2
    vals = np.array([-1.0, -0.5, -0.25, 0.25, 0.5, 0.75, 1.0, 1.25], np.float32)
    T = rng.choice(vals, size=(V, S, S)) * (rng.rand(V, S, S) < density)
    W = rng.choice(vals, size=(S, S)) * (rng.rand(S, S) < density / 2)
    O = rng.choice(np.array([-0.5, 0.5, 1.0, 1.0], np.float32), size=(C, S, S)) * (rng.rand(C, S, S) < min(1.0, 2.0 / C))
    h0 = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=S); h0[0] = 1.0
    hT = (rng.rand(S) < 0.5).astype(np.float32); hT[S - 1] = 1.0
    return T.astype(np.float32), W.astype(np.float32), O.astype(np.float32), h0, hT
