"""Test infrastructure: one training step of the decomposed i-FST in the max semiring (--train_mode max), restated in plain
torch with autograd on the CPU, in float64 or float32.

    get_forward_score, train_mode = 'max'   reference model_decompose_single.py:156-166
    _maxmul                                 reference utils.py:192-195

torch.max over the source state returns ONE index per target state, the first maximal one, and its backward sends the
whole adjoint there; this restatement uses torch.max too.  Everything else (the gates, Osum, the scores, CE1 or the CRF,
the priority layer, the word table) is oracle/farnn_train_oracle.py's sum-semiring restatement, unchanged.

min_gap: every non-zero maximum must beat every other candidate by at least min_gap relative (GapError otherwise), so
that rounding cannot decide which index wins and a float32 kernel must pick the same one.  Exact-zero maxima are exempt:
a product with a zero factor is exactly +-0 under any rounding, and both sides then take the first of the tied indices.
"""
import numpy as np
import torch

from oracle import farnn_train_oracle as to


class GapError(AssertionError):
    pass


def maxmul(h, Tr, min_gap=None):
    """n[s] = max_j h[j] Tr[j, s] (torch.max: the first maximal j)."""
    temp = h[:, None] * Tr
    val, _ = torch.max(temp, dim=0)
    if min_gap is not None and temp.shape[0] > 1:
        with torch.no_grad():
            top = torch.topk(temp, 2, dim=0).values
            bad = (top[0] != 0) & ((top[0] - top[1]) < min_gap * top[0].abs())
            if bool(bad.any()):
                raise GapError('a maximum is decided by less than {} relative'.format(min_gap))
    return val


def chain_scores(Vgen, S1, S2, W, C, h0, hT, x, lengths, nl='none', P=None, gates=None, farnn=0, sig_k=5.0, min_gap=None):
    """Scores of the valid positions, flattened batch-major ([sum(len), K])."""
    osum = C.sum(0)

    def step(h, v, h_init, fwd):
        if farnn >= 1:
            z = torch.sigmoid(sig_k * (h @ gates['Wss1'] + v @ gates['Wrs1'] + gates['bs1'].reshape(-1)))
        hbar = h
        if farnn == 2:
            r = torch.sigmoid(sig_k * (h @ gates['Wss2'] + v @ gates['Wrs2'] + gates['bs2'].reshape(-1)))
            hbar = (1 - r) * h_init + r * h
        Tr = (v * S1) @ S2.T + W                                      # Tr[j, s] = sum_r S2[s, r] v[r] S1[j, r] + W[j, s]
        if fwd:
            nxt = to._nl(maxmul(hbar, Tr, min_gap) * osum, nl)
        else:
            nxt = to._nl(maxmul(hbar * osum, Tr.T, min_gap), nl)
        return nxt if farnn == 0 else (1 - z) * h + z * nxt

    flat = []
    for b in range(x.shape[0]):
        n = int(lengths[b])
        if n == 0:
            continue
        toks = [int(t) for t in x[b, :n]]
        f = [h0]
        for t in toks:
            f.append(step(f[-1], Vgen[t], h0, True))
        bk = [hT]
        for t in reversed(toks):
            bk.append(step(bk[-1], Vgen[t], hT, False))
        for i in range(n):
            flat.append((f[i + 1] * bk[n - 1 - i]) @ C.T)
    s = torch.stack(flat)
    return s @ P if P is not None else s


def _loss(s, lengths, labels, trans):
    if trans is not None:
        return to.crf_nll(s, lengths, labels, trans)
    flat_labels = torch.cat([torch.as_tensor(labels[b, :int(lengths[b])]) for b in range(len(lengths))])
    return torch.nn.functional.cross_entropy(s, flat_labels)


def train_step(p, x, lengths, labels, nl='none', additional_nonlinear='none', use_priority=False, farnn=0, sig_k=5.0,
               dtype=torch.float32, min_gap=None):
    """p: the reference's parameters by name (+ 'priority_mat', 'crf.transitions', gates).  Returns (loss, {name: grad})."""
    q = {k: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(k != 'priority_mat') for k, v in p.items()}
    Vgen = to.generalized_table(q, additional_nonlinear)
    s = chain_scores(Vgen, q['S1'], q['S2'], q['wildcard_mat'], q['C_output_mat'], q['h0'], q['hT'], x, lengths, nl,
                     q['priority_mat'] if use_priority else None, gates=q, farnn=farnn, sig_k=sig_k, min_gap=min_gap)
    loss = _loss(s, lengths, labels, q.get('crf.transitions'))
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in q.items() if v.grad is not None}


def step_on_table(w, x, lengths, labels, nl='none', farnn=0, sig_k=5.0, dtype=torch.float64, min_gap=None):
    """The step on the library's inputs: w holds Vgen, S1, S2, W, C, h0, hT, optionally P, trans and the gates (numpy).
    Returns (loss, {name: grad}, scores)."""
    q = {k: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(k != 'P') for k, v in w.items() if v is not None}
    s = chain_scores(q['Vgen'], q['S1'], q['S2'], q['W'], q['C'], q['h0'], q['hT'], x, lengths, nl, q.get('P'),
                     gates=q, farnn=farnn, sig_k=sig_k, min_gap=min_gap)
    loss = _loss(s, lengths, labels, q.get('trans'))
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in q.items() if v.grad is not None}, s.detach().numpy()
