"""A torch restatement of the onehot FST training step (FARNN_S_O, sum semiring, CE1 loss), written from the arithmetic,
for the tests of farnn_fst4_train_step.  Evaluates in the dtype it is asked for (float32 or float64), differentiates with
autograd, and runs Adam for the multi-step checks.

Reference citations (src_seq/farnn/model_onehot.py):
  M_w = language_tensor.sum(1)[w] + wildcard_tensor.sum(0)          :82 (CE1)
  A = language_tensor + wildcard_tensor                             :87
  forward chain  alpha_{i+1} = relu(alpha_i M_{x_i}), alpha_0 = h0  :89-95 (always relu, no mask)
  backward chain beta_i = relu(M_{x_i} beta_{i+1}), beta_n = hT     :97-102
  score_i[c] = sum_{s,j} relu(A[x_i,c,s,j] alpha_i[s] beta_{i+1}[j])  :115-122 (alpha_i: the state BEFORE token i)
  priority: score @ P                                               :124-125
  loss = CrossEntropyLoss(mean) over valid tokens                   :131-146, :59-60
  decode: column C-1 clamped to threshold, argmax, C-1 -> o_idx     :162-180

The gap rule (check_gap): every chain pre-activation that can reach a score and every score product A alpha beta at a valid
position is exactly 0 or at least min_gap away from 0, in float32 and in float64, so that no relu decision of the step can
be reversed by float32 rounding (the gradient is discontinuous there: a reversed decision is a different function).
"""
import numpy as np
import torch


class GapError(AssertionError):
    pass


def _t(a, dtype):
    return a.to(dtype) if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)).to(dtype)


def _ints(a):
    return a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))


def forward(T4, W4, h0, hT, P, x, lengths):
    """scores [B, L, C] (after the priority layer), valid [B, L], chain pre-activations [2, B, L, S], products [B, L, C, S, S]"""
    x, lengths = _ints(x), _ints(lengths)
    B, L = x.shape
    lens = lengths.clamp(0, L)
    M = T4.sum(1) + W4.sum(0)
    A = T4 + W4
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
    prod = (A[x] * alpha[:, :, None, :, None]) * beta[:, :, None, None, :]
    sc = torch.relu(prod).sum(dim=(3, 4))
    if P is not None:
        sc = sc @ P
    valid = i < lens[:, None]
    return sc, valid, torch.stack(pre, 2), prod


def check_gap(T4, W4, h0, hT, x, lengths, min_gap=2e-5):
    """Raises GapError unless the rule of the module docstring holds on these inputs."""
    x, lengths = _ints(x), _ints(lengths)
    L = x.shape[1]
    lens = lengths.clamp(0, L)
    t = torch.arange(L)[None, :]
    for dtype in (torch.float32, torch.float64):
        with torch.no_grad():
            _, valid, pre, prod = forward(*(_t(a, dtype) for a in (T4, W4, h0, hT)), None, x, lens)
        live = (t < lens[:, None] - 1)[None, :, :, None]          # alpha_len and beta_0 feed nothing
        bad = live & (pre != 0) & (pre.abs() < min_gap)
        if bool(bad.any()):
            raise GapError('{} chain pre-activations within {} of 0 in {}'.format(int(bad.sum()), min_gap, dtype))
        bad = valid[:, :, None, None, None] & (prod != 0) & (prod.abs() < min_gap)
        if bool(bad.any()):
            raise GapError('{} score products within {} of 0 in {}'.format(int(bad.sum()), min_gap, dtype))


def loss_and_pred(T4, W4, h0, hT, P, x, lengths, labels, threshold, o_idx):
    sc, valid, _, _ = forward(T4, W4, h0, hT, P, x, lengths)
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


def step(T4, W4, h0, hT, P, x, lengths, labels, threshold=0.5, o_idx=0, dtype=torch.float64):
    """(loss, dT4, dW4, flat_pred) of one training step, evaluated in `dtype`."""
    Tt = _t(T4, dtype).clone().requires_grad_(True)
    Wt = _t(W4, dtype).clone().requires_grad_(True)
    h0t, hTt = _t(h0, dtype), _t(hT, dtype)
    Pt = None if P is None else _t(P, dtype)
    loss, pred = loss_and_pred(Tt, Wt, h0t, hTt, Pt, x, lengths, labels, threshold, o_idx)
    loss.backward()
    return float(loss.detach()), Tt.grad.detach().numpy(), Wt.grad.detach().numpy(), pred


def adam_steps(T4, W4, h0, hT, P, batches, train_wildcard=False, lr=1e-3, dtype=torch.float64):
    """(language_tensor, wildcard_tensor) after one Adam step (torch.optim.Adam, weight_decay 0) per (x, lengths, labels)"""
    Tt = _t(T4, dtype).clone().requires_grad_(True)
    Wt = _t(W4, dtype).clone().requires_grad_(bool(train_wildcard))
    h0t, hTt = _t(h0, dtype), _t(hT, dtype)
    Pt = None if P is None else _t(P, dtype)
    opt = torch.optim.Adam([Tt] + ([Wt] if train_wildcard else []), lr=lr, weight_decay=0)
    for x, lengths, labels in batches:
        opt.zero_grad()
        loss, _ = loss_and_pred(Tt, Wt, h0t, hTt, Pt, x, lengths, labels, 0.5, 0)
        loss.backward()
        opt.step()
    return Tt.detach().numpy(), Wt.detach().numpy()


def signed_base(V, S, C, rng, density=None):
    """Signed real-valued tensors on which the gap rule holds by construction for short sequences: sparse blocks whose
    entries are multiples of 1/4 in [-1, 1.25] (every chain value and score product is then a small dyadic rational,
    exact in float32 and in float64, as long as the sequences stay a few tokens long)."""
    density = density if density is not None else min(0.5, 3.0 / (S * C))      # |M| rows sum to about 2
    vals = np.array([-1.0, -0.5, -0.25, 0.25, 0.5, 0.75, 1.0, 1.25], np.float32)
    T4 = rng.choice(vals, size=(V, C, S, S)) * (rng.rand(V, C, S, S) < density)
    W4 = rng.choice(vals, size=(C, S, S)) * (rng.rand(C, S, S) < density / 2)
    h0 = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=S); h0[0] = 1.0
    hT = (rng.rand(S) < 0.5).astype(np.float32); hT[S - 1] = 1.0
    return T4.astype(np.float32), W4.astype(np.float32), h0, hT
