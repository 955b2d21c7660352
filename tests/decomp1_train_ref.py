"""A torch restatement of the decomposed independent=1 training step (FARNN_S_D_W_I, farnn = 0, sum semiring, CE1 loss),
written from the arithmetic, for the tests of farnn_decomp_ind1_train_step.  Evaluates in the dtype it is asked for
(float32 or float64), differentiates with autograd, and runs Adam for the multi-step checks.

Reference citations (src_seq/farnn/model_decompose_independent.py; model_decompose.py for the word table):
  Vgen = V_embed * beta + act(E G) * (1 - beta)                       model_decompose.py:222-241
  N_w[i,j] = sum_r Vgen[w,r] S1[i,r] S2[j,r] + wildcard_mat[i,j]      :171-173
  Osum[i,j] = sum_r (sum_c C_output[c,r]) S1_output[i,r] S2_output[j,r]   :210-214 (einsum 'sr,jr->js' of S2_output[s,r]
                                                                      and csum_r S1_output[j,r]; CE1: no wildcard_output)
  Mc_w = N_w * Osum                                                   :174
  forward chain  alpha_{t+1} = nl(alpha_t Mc_{x_t}), alpha_0 = h0     :176-188, :239-245
  backward chain beta_t = nl(Mc_{x_t} beta_{t+1}), beta_n = hT        :179, :247-252
  br_i[r] = sum_ij alpha_i[i] beta_{i+1}[j] N_{x_i}[i,j] S1_output[i,r] S2_output[j,r]     :199-205 (alpha_i: the state BEFORE
                                                                      token i; N, not Mc)
  score_i = br_i C_output^T, then score @ P                           :206, :277-278
  loss = CrossEntropyLoss(mean) over valid tokens                     :295
  decode: column C-1 clamped to threshold, argmax, C-1 -> o_idx       :298

The gap rule (check_gap): every pre-activation of a relu / relutanh chain that can reach a score is exactly 0 or away from 0
by min_gap and by 8 S eps32 times the sum of its terms' magnitudes (eight times the rounding bound of a float32 dot product
of S terms: what a float32 evaluation in another order can move it by), in float32 and in float64 (a reversed relu decision
is a different function; min_gap = 0 leaves the rounding bound alone, for inputs with noise in them), and at every valid
position the decoded column wins by a margin -- top two clamped scores apart, the last column not within the margin of the
threshold clamp -- so that float32 and float64 decode alike.
"""
import numpy as np
import torch

FLOAT_KEYS = ('S1', 'S2', 'wildcard_mat', 'C_output', 'S1_output', 'S2_output', 'h0', 'hT')
VGEN_KEYS = ('V_embed', 'embedding.weight', 'embed_r_generalized', 'beta_vec')
EPS32 = 2.0 ** -24


class GapError(AssertionError):
    pass


def _t(a, dtype):
    return a.to(dtype) if torch.is_tensor(a) else torch.from_numpy(np.asarray(a)).to(dtype)


def _ints(a):
    return a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))


def apply_nl(v, nl):
    if nl == 'relu':
        return torch.relu(v)
    if nl == 'tanh':
        return torch.tanh(v)
    if nl == 'relutanh':
        return torch.tanh(torch.relu(v))
    if nl == 'sigmoid':
        return torch.sigmoid(v)
    return v


def vgen_of(p, add_nl='none'):
    """the word table [V, R]: p['Vgen'] when the case gives it, else built from the model's four tensors"""
    if 'Vgen' in p:
        return p['Vgen']
    gen = apply_nl(p['embedding.weight'] @ p['embed_r_generalized'], add_nl)
    return p['V_embed'] * p['beta_vec'] + gen * (1 - p['beta_vec'])


def forward(p, P, x, lengths, nl='none', add_nl='none', detach_chains=False):
    """scores [B, L, C] (after the priority layer), valid [B, L], chain pre-activations [2, B, L, S] and the sums of their
    terms' magnitudes (|state| |Mc|), same shape"""
    x, lengths = _ints(x), _ints(lengths)
    B, L = x.shape
    lens = lengths.clamp(0, L)
    v = vgen_of(p, add_nl)
    N = torch.einsum('wr,ir,jr->wij', v, p['S1'], p['S2']) + p['wildcard_mat']
    csum = p['C_output'].sum(0)
    Osum = torch.einsum('r,ir,jr->ij', csum, p['S1_output'], p['S2_output'])
    M = N * Osum
    if detach_chains:                                          # no gradient through the chains: dMc = 0
        M = M.detach()
    idx = torch.arange(L)
    src = torch.where(idx[None, :] < lens[:, None], lens[:, None] - 1 - idx[None, :], idx[None, :])
    xr = torch.gather(x, 1, src)                               # reverse(x, len)
    f, b, pre, mag = [p['h0'].expand(B, -1)], [p['hT'].expand(B, -1)], [], []
    for t in range(L):
        pf = torch.bmm(f[-1].unsqueeze(1), M[x[:, t]]).squeeze(1)
        pb = torch.bmm(b[-1].unsqueeze(1), M[xr[:, t]].transpose(1, 2)).squeeze(1)
        pre.append(torch.stack([pf, pb]))
        with torch.no_grad():
            mag.append(torch.stack([torch.bmm(f[-1].abs().unsqueeze(1), M[x[:, t]].abs()).squeeze(1),
                                    torch.bmm(b[-1].abs().unsqueeze(1), M[xr[:, t]].abs().transpose(1, 2)).squeeze(1)]))
        f.append(apply_nl(pf, nl))
        b.append(apply_nl(pb, nl))
    F, Bs = torch.stack(f, 1), torch.stack(b, 1)               # [B, L+1, S]: alpha_t, beta_{len-t}
    i = idx[None, :].expand(B, L)
    bidx = (lens[:, None] - 1 - i).clamp(min=0)
    alpha = F[:, :L]
    beta = torch.gather(Bs, 1, bidx.unsqueeze(-1).expand(B, L, Bs.shape[-1]))
    ab = (alpha[:, :, :, None] * beta[:, :, None, :]) * N[x]   # [B, L, S, S]
    br = torch.einsum('blij,ir,jr->blr', ab, p['S1_output'], p['S2_output'])
    sc = br @ p['C_output'].t()
    if P is not None:
        sc = sc @ P
    valid = i < lens[:, None]
    return sc, valid, torch.stack(pre, 2), torch.stack(mag, 2)


def _params(p, dtype, grad=False):
    return {k: (_t(a, dtype).clone().requires_grad_(True) if grad else _t(a, dtype)) for k, a in p.items()}


def check_gap(p, P, x, lengths, nl='none', add_nl='none', threshold=0.5, min_gap=2e-5, margin=1e-4):
    """Raises GapError unless the rule of the module docstring holds on these inputs."""
    x, lengths = _ints(x), _ints(lengths)
    L = x.shape[1]
    lens = lengths.clamp(0, L)
    t = torch.arange(L)[None, :]
    for dtype in (torch.float32, torch.float64):
        with torch.no_grad():
            sc, valid, pre, mag = forward(_params(p, dtype), None if P is None else _t(P, dtype), x, lens, nl=nl, add_nl=add_nl)
        if nl in ('relu', 'relutanh'):
            live = (t < lens[:, None] - 1)[None, :, :, None]      # alpha_len and beta_0 feed nothing
            bound = torch.clamp(8 * pre.shape[-1] * EPS32 * mag, min=min_gap)
            bad = live & (pre != 0) & (pre.abs() < bound)
            if bool(bad.any()):
                raise GapError('{} chain pre-activations within the gap of 0 in {}'.format(int(bad.sum()), dtype))
        flat = sc[valid]
        if flat.numel():
            C = flat.shape[1]
            last = flat[:, C - 1]
            d = flat.clone()
            d[:, C - 1] = torch.clamp(last, max=threshold)
            if C > 1:
                top = d.topk(2, dim=1).values
                gap = top[:, 0] - top[:, 1]                           # (an exact tie decodes to the first index in both)
                tie = (gap != 0) & (gap < margin * (1 + top[:, 0].abs()))
                if bool(tie.any()):
                    raise GapError('{} positions whose top two scores are within the margin in {}'.format(int(tie.sum()), dtype))
            near = (last - threshold).abs() < margin * (1 + abs(threshold))
            if bool(near.any()):
                raise GapError('{} positions whose last column sits at the threshold clamp in {}'.format(int(near.sum()), dtype))


def loss_and_pred(p, P, x, lengths, labels, nl, add_nl, threshold, o_idx, detach_chains=False):
    sc, valid, _, _ = forward(p, P, x, lengths, nl=nl, add_nl=add_nl, detach_chains=detach_chains)
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


def step(p, P, x, lengths, labels, nl='none', add_nl='none', threshold=0.5, o_idx=0, dtype=torch.float64, detach_chains=False):
    """(loss, {name: gradient} for every float tensor of p, flat_pred) of one training step, evaluated in `dtype`.
    p: 'Vgen' or the four tensors of VGEN_KEYS, plus FLOAT_KEYS."""
    pt = _params(p, dtype, grad=True)
    Pt = None if P is None else _t(P, dtype)
    loss, pred = loss_and_pred(pt, Pt, x, lengths, labels, nl, add_nl, threshold, o_idx, detach_chains=detach_chains)
    loss.backward()
    grads = {k: (t.grad.detach().numpy() if t.grad is not None else np.zeros(tuple(t.shape), t.detach().numpy().dtype))
             for k, t in pt.items()}
    return float(loss.detach()), grads, pred


def adam_steps(p, P, batches, trainable, nl='none', add_nl='none', lr=1e-3, dtype=torch.float64):
    """every tensor of p after one Adam step (torch.optim.Adam, weight_decay 0) per (x, lengths, labels); only the names in
    `trainable` move"""
    pt = {k: _t(a, dtype).clone().requires_grad_(k in trainable) for k, a in p.items()}
    Pt = None if P is None else _t(P, dtype)
    opt = torch.optim.Adam([pt[k] for k in p if k in trainable], lr=lr, weight_decay=0)
    for x, lengths, labels in batches:
        opt.zero_grad()
        loss, _ = loss_and_pred(pt, Pt, x, lengths, labels, nl, add_nl, 0.5, 0)
        loss.backward()
        opt.step()
    return {k: t.detach().numpy() for k, t in pt.items()}


def signed_base(V, S, R, RO, C, rng):
    """Signed real-valued factors: entries are small multiples of 1/4 (sparse for the state factors, so that a block N_w has
    a few entries per row), h0 / hT as in ind1_train_ref.signed_base.  Dense products of them are not dyadic-exact for long
    sequences: the cases are drawn again until check_gap holds."""
    vals = np.array([-1.0, -0.5, -0.25, 0.25, 0.5, 0.75, 1.0, 1.25], np.float32)
    dens = min(0.6, 2.0 / max(1.0, np.sqrt(S)))
    Vgen = rng.choice(vals, size=(V, R)) * (rng.rand(V, R) < min(1.0, 3.0 / R + 0.3))
    S1 = rng.choice(vals, size=(S, R)) * (rng.rand(S, R) < dens)
    S2 = rng.choice(vals, size=(S, R)) * (rng.rand(S, R) < dens)
    W = rng.choice(vals, size=(S, S)) * (rng.rand(S, S) < min(0.5, 1.5 / S))
    Cout = rng.choice(np.array([-0.5, 0.5, 1.0, 1.0], np.float32), size=(C, RO)) * (rng.rand(C, RO) < min(1.0, 2.0 / RO + 0.4))
    S1o = rng.choice(np.array([-0.5, 0.5, 1.0, 1.0], np.float32), size=(S, RO)) * (rng.rand(S, RO) < max(dens, min(1.0, 2.0 / RO)))
    S2o = rng.choice(np.array([-0.5, 0.5, 1.0, 1.0], np.float32), size=(S, RO)) * (rng.rand(S, RO) < max(dens, min(1.0, 2.0 / RO)))
    h0 = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=S); h0[0] = 1.0
    hT = (rng.rand(S) < 0.5).astype(np.float32); hT[S - 1] = 1.0
    # powers of two (exact) bring max |Osum| into [1, 2) and the mean absolute row sum of Mc = N * Osum into [1, 2): the chains
    # neither die out nor blow up over a few tokens, whatever R and R_O are
    Osum = np.einsum('r,ir,jr->ij', Cout.sum(0), S1o, S2o)
    if np.abs(Osum).max() > 0:
        k = 2.0 ** -np.floor(np.log2(np.abs(Osum).max()))
        Cout, Osum = Cout * k, Osum * k
    rows = np.abs(np.einsum('wr,ir,jr->wij', Vgen, S1, S2) * Osum).sum(2).mean()
    if rows > 0:
        Vgen = Vgen * 2.0 ** -np.floor(np.log2(rows))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    return {'Vgen': f(Vgen), 'S1': f(S1), 'S2': f(S2), 'wildcard_mat': f(W), 'C_output': f(Cout), 'S1_output': f(S1o),
            'S2_output': f(S2o), 'h0': f(h0), 'hT': f(hT)}


WORD_KEYS = ('Vgen', 'V_embed', 'embedding.weight')


def badly_drawn(g32, g64, present, tol=1e-4):
    """Why tests/util.py's gradient rule would call these inputs badly drawn, read off the restatement alone, or None: a
    tensor without a live float64 gradient, a tensor on which float32 is beyond a tenth of the bar from float64, or (word
    tensors) a present word whose slice is"""
    for n in sorted(g64):
        a, b = np.asarray(g32[n], np.float64), np.asarray(g64[n], np.float64)
        s = np.abs(b).max()
        if not s > 0:
            return n + ': no gradient'
        if np.abs(a - b).max() > tol / 10 * s:
            return n + ': float32 beyond a tenth of the bar'
        if n in WORD_KEYS:
            a, b = a.reshape(a.shape[0], -1)[present], b.reshape(b.shape[0], -1)[present]
            if (np.abs(a - b).max(1) > tol / 10 * np.abs(b).max(1)).any():
                return n + ': a present word is ill-conditioned in float32'
    return None
