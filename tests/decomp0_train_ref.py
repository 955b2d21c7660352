"""A torch restatement of the decomposed FST's training step (FARNN_S_D_W, sum semiring, farnn 0 / 1 / 2, CE1 or the CRF's
negative log-likelihood), written from the arithmetic, for the tests of farnn_decomp_fst_train_step.  Evaluates in the dtype
it is asked for (float32 or float64) and differentiates with autograd.

  csum = C_embed.sum(0); cwsum = C_wildcard.sum(0)
  Rtab[w] = Vgen[w] * csum;  W = S1w diag(cwsum) S2w^T + WW
  forward chain   a_{t+1} = step(a_t, Rtab[x_t], S1, S2, W),   a_0 = h0
  backward chain  b_{t+1} = step(b_t, Rtab[x_{n-1-t}], S2, S1, W^T), b_0 = hT
  step(h, r, M1, M2, W): z = sig(k (h Wss1 + r Wrs1 + bs1)) [farnn >= 1]; g = sig(k (h Wss2 + r Wrs2 + bs2)) [farnn 2];
                         hbar = (1 - g) h_init + g h [farnn 2] else h; n = nl(((hbar M1) * r) M2^T + hbar W);
                         h' = (1 - z) h + z n [farnn >= 1] else n
  score_i[c] = sum_r Vgen[x_i, r] C_embed[c, r] (a_i S1)_r (b_{n-1-i} S2)_r + sum_q C_wildcard[c, q] (a_i S1w)_q (b_{n-1-i} S2w)_q
  then score @ P; CE1: mean cross-entropy over the valid tokens, decode = argmax with the last column clamped to the threshold;
  CRF: sum over the sequences of log Z - gold path score with START = K-2, STOP = K-1, decode = Viterbi with column K-3 clamped.

The gap rule (check_gap) is decomp1_train_ref's: relu pre-activations away from 0 and the decoded column a margin ahead, in
float32 and float64, so that both decode alike.
"""
import numpy as np
import torch

from decomp1_train_ref import EPS32, GapError, WORD_KEYS, _ints, _params, _t, apply_nl, badly_drawn, vgen_of  # noqa: F401

FLOAT_KEYS = ('S1', 'S2', 'C_embed', 'C_wildcard', 'S1_wildcard', 'S2_wildcard', 'wildcard_wildcard', 'h0', 'hT')
VGEN_KEYS = ('V_embed', 'embedding.weight', 'embed_r_generalized', 'beta_vec')
GATE_KEYS = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')
TRANS = 'crf.transitions'


def gate_keys(farnn):
    return GATE_KEYS[:3 * int(farnn)]


def forward(p, P, x, lengths, nl='none', add_nl='none', farnn=0, k=5.0):
    """scores [B, L, K] after the priority layer, valid [B, L], chain pre-activations [2, B, L, S] and their terms' magnitudes"""
    x, lengths = _ints(x), _ints(lengths)
    B, L = x.shape
    lens = lengths.clamp(0, L)
    v = vgen_of(p, add_nl)
    rtab = v * p['C_embed'].sum(0)
    W = (p['S1_wildcard'] * p['C_wildcard'].sum(0)) @ p['S2_wildcard'].t() + p['wildcard_wildcard']
    idx = torch.arange(L)
    src = torch.where(idx[None, :] < lens[:, None], lens[:, None] - 1 - idx[None, :], idx[None, :])
    xr = torch.gather(x, 1, src)

    def step(h, hin, r, M1, M2, Wm):
        z = g = None
        if farnn >= 1:
            z = torch.sigmoid(k * (h @ p['Wss1'] + r @ p['Wrs1'] + p['bs1'].reshape(1, -1)))
        hbar = h
        if farnn == 2:
            g = torch.sigmoid(k * (h @ p['Wss2'] + r @ p['Wrs2'] + p['bs2'].reshape(1, -1)))
            hbar = (1 - g) * hin + g * h
        pre = ((hbar @ M1) * r) @ M2.t() + hbar @ Wm
        with torch.no_grad():
            mag = ((hbar.abs() @ M1.abs()) * r.abs()) @ M2.abs().t() + hbar.abs() @ Wm.abs()
        n = apply_nl(pre, nl)
        return (n if z is None else (1 - z) * h + z * n), pre, mag

    h0, hT = p['h0'].expand(B, -1), p['hT'].expand(B, -1)
    f, b, pre, mag = [h0], [hT], [], []
    for t in range(L):
        nf, pf, mf = step(f[-1], h0, rtab[x[:, t]], p['S1'], p['S2'], W)
        nb, pb, mb = step(b[-1], hT, rtab[xr[:, t]], p['S2'], p['S1'], W.t())
        f.append(nf); b.append(nb); pre.append(torch.stack([pf, pb])); mag.append(torch.stack([mf, mb]))
    F, Bs = torch.stack(f, 1), torch.stack(b, 1)
    i = idx[None, :].expand(B, L)
    bidx = (lens[:, None] - 1 - i).clamp(min=0)
    alpha = F[:, :L]
    beta = torch.gather(Bs, 1, bidx.unsqueeze(-1).expand(B, L, Bs.shape[-1]))
    u = v[x] * (alpha @ p['S1']) * (beta @ p['S2'])
    uw = (alpha @ p['S1_wildcard']) * (beta @ p['S2_wildcard'])
    sc = u @ p['C_embed'].t() + uw @ p['C_wildcard'].t()
    if P is not None:
        sc = sc @ P
    return sc, i < lens[:, None], torch.stack(pre, 2), torch.stack(mag, 2)


def crf_nll(sc, lens, labels, tr):
    """sum over the sequences of log Z - score(gold path); tr[i, j]: from i to j; START = K - 2, STOP = K - 1"""
    B, L, K = sc.shape
    total = sc.new_zeros(())
    for b in range(B):
        n = int(lens[b])
        if n == 0:
            continue
        a = sc[b, 0] + tr[K - 2]
        gold = sc[b, 0, labels[b, 0]] + tr[K - 2, labels[b, 0]]
        for t in range(1, n):
            a = torch.logsumexp(a[:, None] + tr, 0) + sc[b, t]
            gold = gold + sc[b, t, labels[b, t]] + tr[labels[b, t - 1], labels[b, t]]
        total = total + torch.logsumexp(a + tr[:, K - 1], 0) - (gold + tr[labels[b, n - 1], K - 1])
    return total


def crf_decode(sc, lens, tr, threshold, o_idx):
    B, L, K = sc.shape
    sc = sc.clone()
    sc[:, :, K - 3] = torch.clamp(sc[:, :, K - 3], max=threshold)
    out = []
    for b in range(B):
        n = int(lens[b])
        if n == 0:
            continue
        vit, bp = sc[b, 0] + tr[K - 2], []
        for t in range(1, n):
            cand = (sc[b, t][None, :] + tr) + vit[:, None]
            vit, arg = cand.max(0)
            bp.append(arg)
        ptr = int((vit + tr[:, K - 1]).argmax())
        path = [ptr]
        for arg in reversed(bp):
            ptr = int(arg[ptr])
            path.append(ptr)
        out += [o_idx if c == K - 3 else c for c in reversed(path)]
    return np.asarray(out, np.int64)


def loss_and_pred(p, P, x, lengths, labels, nl, add_nl, threshold, o_idx, farnn=0, k=5.0, trans=None):
    sc, valid, _, _ = forward(p, P, x, lengths, nl=nl, add_nl=add_nl, farnn=farnn, k=k)
    lab = _ints(labels)
    lens = _ints(lengths).clamp(0, sc.shape[1])
    if trans is not None:
        loss = crf_nll(sc, lens, lab, trans)
        with torch.no_grad():
            pred = crf_decode(sc.detach(), lens, trans.detach(), threshold, o_idx)
        return loss, pred
    flat = sc[valid]
    loss = torch.nn.functional.cross_entropy(flat, lab[valid])
    with torch.no_grad():
        d = flat.clone()
        C = d.shape[1]
        d[:, C - 1] = torch.clamp(d[:, C - 1], max=threshold)
        pred = d.argmax(1)
        pred[pred == C - 1] = o_idx
    return loss, pred.numpy()


def step(p, P, x, lengths, labels, nl='none', add_nl='none', threshold=0.5, o_idx=0, dtype=torch.float64, farnn=0, k=5.0,
         trans=None):
    """(loss, {name: gradient} for every float tensor of p and 'crf.transitions', flat_pred), evaluated in `dtype`"""
    pt = _params(p, dtype, grad=True)
    Pt = None if P is None else _t(P, dtype)
    tr = None if trans is None else _t(trans, dtype).clone().requires_grad_(True)
    loss, pred = loss_and_pred(pt, Pt, x, lengths, labels, nl, add_nl, threshold, o_idx, farnn=farnn, k=k, trans=tr)
    loss.backward()
    grads = {q: (t.grad.detach().numpy() if t.grad is not None else np.zeros(tuple(t.shape), t.detach().numpy().dtype))
             for q, t in pt.items()}
    if tr is not None:
        grads[TRANS] = tr.grad.detach().numpy()
    return float(loss.detach()), grads, pred


def adam_steps(p, P, batches, nl='none', add_nl='none', farnn=0, k=5.0, lr=1e-3, dtype=torch.float64):
    """every tensor of p after one Adam step (torch.optim.Adam, weight_decay 0) per (x, lengths, labels); CE1 loss"""
    pt = {q: _t(a, dtype).clone().requires_grad_(True) for q, a in p.items()}
    Pt = None if P is None else _t(P, dtype)
    opt = torch.optim.Adam(list(pt.values()), lr=lr, weight_decay=0)
    for x, lengths, labels in batches:
        opt.zero_grad()
        loss, _ = loss_and_pred(pt, Pt, x, lengths, labels, nl, add_nl, 0.5, 0, farnn=farnn, k=k)
        loss.backward()
        opt.step()
    return {q: t.detach().numpy() for q, t in pt.items()}


def check_gap(p, P, x, lengths, nl='none', add_nl='none', threshold=0.5, farnn=0, k=5.0, trans=None, min_gap=2e-5, margin=1e-4):
    """Raises GapError unless the module docstring's rule holds.  Under the CRF the margin is asked of the sequence: the
    float32 and the float64 Viterbi paths must agree."""
    x, lengths = _ints(x), _ints(lengths)
    L = x.shape[1]
    lens = lengths.clamp(0, L)
    t = torch.arange(L)[None, :]
    paths = []
    for dtype in (torch.float32, torch.float64):
        with torch.no_grad():
            sc, valid, pre, mag = forward(_params(p, dtype), None if P is None else _t(P, dtype), x, lens, nl=nl, add_nl=add_nl,
                                          farnn=farnn, k=k)
        if nl in ('relu', 'relutanh'):
            live = (t < lens[:, None] - 1)[None, :, :, None]
            bound = torch.clamp(8 * pre.shape[-1] * EPS32 * mag, min=min_gap)
            bad = live & (pre != 0) & (pre.abs() < bound)
            if bool(bad.any()):
                raise GapError('{} chain pre-activations within the gap of 0 in {}'.format(int(bad.sum()), dtype))
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


def signed_base(V, S, R, Q, K, rng, farnn=0):
    """Signed real-valued factors, small multiples of 1/4, scaled by powers of two so that the chains neither die nor blow up"""
    vals = np.array([-1.0, -0.5, -0.25, 0.25, 0.5, 0.75, 1.0, 1.25], np.float32)
    dens = min(0.6, 2.0 / max(1.0, np.sqrt(S)))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    Vgen = rng.choice(vals, size=(V, R)) * (rng.rand(V, R) < min(1.0, 3.0 / R + 0.3))
    S1 = rng.choice(vals, size=(S, R)) * (rng.rand(S, R) < dens)
    S2 = rng.choice(vals, size=(S, R)) * (rng.rand(S, R) < dens)
    S1w = rng.choice(vals, size=(S, Q)) * (rng.rand(S, Q) < dens)
    S2w = rng.choice(vals, size=(S, Q)) * (rng.rand(S, Q) < dens)
    WW = rng.choice(vals, size=(S, S)) * (rng.rand(S, S) < min(0.5, 1.5 / S))
    Ce = rng.choice(np.array([-0.5, 0.5, 1.0, 1.0], np.float32), size=(K, R)) * (rng.rand(K, R) < min(1.0, 2.0 / R + 0.4))
    Cw = rng.choice(np.array([-0.5, 0.5, 1.0, 1.0], np.float32), size=(K, Q)) * (rng.rand(K, Q) < min(1.0, 2.0 / Q + 0.4))
    h0 = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=S); h0[0] = 1.0
    hT = (rng.rand(S) < 0.5).astype(np.float32); hT[S - 1] = 1.0
    cs, cw = Ce.sum(0), Cw.sum(0)
    for _ in range(2):                        # the mean absolute row sum of a word's transition matrix into [1, 2)
        M = np.einsum('wr,ir,jr->wij', Vgen * cs, S1, S2) + (S1w * cw) @ S2w.T + WW
        rows = np.abs(M).sum(2).mean()
        if rows > 0:
            s = 2.0 ** -np.floor(np.log2(rows))
            Vgen, S1w, WW = Vgen * s, S1w * s, WW * s
    p = {'Vgen': f(Vgen), 'S1': f(S1), 'S2': f(S2), 'C_embed': f(Ce), 'C_wildcard': f(Cw), 'S1_wildcard': f(S1w),
         'S2_wildcard': f(S2w), 'wildcard_wildcard': f(WW), 'h0': f(h0), 'hT': f(hT)}
    for g in range(int(farnn)):
        p['Wss%d' % (g + 1)] = f(rng.choice(vals, size=(S, S)) * (rng.rand(S, S) < min(0.5, 2.0 / S)) * 0.25)
        p['Wrs%d' % (g + 1)] = f(rng.choice(vals, size=(R, S)) * (rng.rand(R, S) < min(0.5, 2.0 / R)) * 0.25)
        p['bs%d' % (g + 1)] = f(rng.choice(np.array([-0.25, 0.0, 0.25], np.float32), size=S))
    return p
