"""Test infrastructure: one training step of the decomposed i-FST with the KD / PR teacher term (--marryup_type kd | pr),
restated in plain torch with autograd on the CPU, in float64 or float32.

    forward_local(train=True, re_tags=...)   reference model_decompose_single.py:207-304
    KD_loss, PR_loss                         reference baselines/KD.py:3-18

What differs from the plain step (oracle/farnn_train_oracle.py): the KL term is KLDivLoss()'s default 'mean' over ALL
B * Lmax * K elements, so it reads the scores of the pad positions.  A pad position i >= len scores C (f_{i+1} * b_{i+1}):
the forward chain continued through the pad tokens x[b, len:], and the backward chain continued past its len reversed tokens
through the SAME raw tokens x[b, len:] (reverse() flips only the first len entries, :222; reverse(.., lengths + 1) only the
first len + 1 stash rows, :261).  The cross-entropy / CRF term stays on the valid positions.

`fault` plants one deliberate mistake (the CPU tests show that the fixtures and the drawn cases see each of them):
    'mask_pads'      the KL sums the valid positions only
    'divisor_valid'  the KL is divided by valid * K instead of B * Lmax * K
    'tail_reversed'  the backward chain reads its tail tokens x[b, len:] reversed
    'detach_pr'      the PR teacher q is detached
    'no_T2'          KD without the factor T^2
    'pi_c2'          PR's weight taken as c2 instead of max(c2, c3 ** t)
"""
import numpy as np
import torch

from oracle import farnn_train_oracle as to

FAULTS = ('mask_pads', 'divisor_valid', 'tail_reversed', 'detach_pr', 'no_T2', 'pi_c2')


def _step(S1, S2, W, osum, nl, gates, farnn, sig_k):
    """get_forward_score in the sum semiring (:138-200), as oracle/farnn_train_oracle.chain_scores states it"""
    def step(h, v, h_init, fwd):
        if farnn >= 1:
            z = torch.sigmoid(sig_k * (h @ gates['Wss1'] + v @ gates['Wrs1'] + gates['bs1'].reshape(-1)))
        hbar = h
        if farnn == 2:
            r = torch.sigmoid(sig_k * (h @ gates['Wss2'] + v @ gates['Wrs2'] + gates['bs2'].reshape(-1)))
            hbar = (1 - r) * h_init + r * h
        if fwd:
            nxt = to._nl((((hbar @ S1) * v) @ S2.T + hbar @ W) * osum, nl)
        else:
            bb = hbar * osum
            nxt = to._nl(((bb @ S2) * v) @ S1.T + bb @ W.T, nl)
        return nxt if farnn == 0 else (1 - z) * h + z * nxt
    return step


def all_scores(Vgen, S1, S2, W, C, h0, hT, x, lengths, nl='none', P=None, gates=None, farnn=0, sig_k=5.0, fault=None):
    """[B, L, K] with L = x.shape[1]: every position's scores, pads included, after the priority layer."""
    step = _step(S1, S2, W, C.sum(0), nl, gates, farnn, sig_k)
    B, L = x.shape
    rows = []
    for b in range(B):
        n = int(lengths[b])
        toks = [int(t) for t in x[b]]
        tail = toks[n:][::-1] if fault == 'tail_reversed' else toks[n:]
        f = [h0]
        for t in toks:
            f.append(step(f[-1], Vgen[t], h0, True))
        bk = [hT]
        for t in toks[:n][::-1] + tail:
            bk.append(step(bk[-1], Vgen[t], hT, False))
        # valid: alpha row i+1 and backward row n-1-i; pad: row i+1 of both; backward row n is read by nobody
        rows.append(torch.stack([(f[i + 1] * bk[n - 1 - i if i < n else i + 1]) @ C.T for i in range(L)]))
    s = torch.stack(rows)
    return s @ P if P is not None else s


def _kl_sum(log_input, target):
    """the pointwise terms of torch's kl_div: xlogy(target, target) - target * input, per position ([B, L])"""
    return (torch.xlogy(target, target) - target * log_input).sum(2)


def kl_term(scores, re, mode, c1, lengths, fault=None):
    """KD_loss / PR_loss (KD.py:3-18) on scores, re [B, L, K]"""
    B, L, K = scores.shape
    if mode == 'kd':
        per_pos = _kl_sum(torch.log_softmax(scores / c1, 2), torch.softmax(re / c1, 2))
        factor = 1.0 if fault == 'no_T2' else c1 * c1
    else:
        q = torch.softmax(torch.softmax(scores, 2) * (torch.exp(re - 1) * c1), 2)          # NOT detached (KD.py:15-17)
        if fault == 'detach_pr':
            q = q.detach()
        per_pos = _kl_sum(torch.log_softmax(scores, 2), q)
        factor = 1.0
    valid = torch.arange(L)[None, :] < torch.as_tensor(np.asarray(lengths))[:, None]
    if fault == 'mask_pads':
        per_pos = per_pos * valid.to(per_pos.dtype)
    div = float(valid.sum()) * K if fault == 'divisor_valid' else float(B * L * K)
    return per_pos.sum() / div * factor


def original_loss(scores, lengths, labels, trans):
    """cross-entropy, mean over the valid tokens, or the CRF's sum over the batch -- on the valid positions only"""
    B = scores.shape[0]
    flat = torch.cat([scores[b, :int(lengths[b])] for b in range(B)])
    if trans is not None:
        return to.crf_nll(flat, lengths, labels, trans)
    flat_labels = torch.cat([torch.as_tensor(np.asarray(labels[b, :int(lengths[b])])) for b in range(B)])
    return torch.nn.functional.cross_entropy(flat, flat_labels)


def pad_and_cut(re_tags, use_crf, L):
    """the zero columns of :213-218 (one without the CRF, three with it) and the cut to Lmax of :292-298"""
    B, Lp, _ = re_tags.shape
    return np.concatenate([re_tags, np.zeros((B, Lp, 3 if use_crf else 1), re_tags.dtype)], 2)[:, :L]


def weight_of_original(mode, c2, c3, fault=None, t=1):
    """c2 for KD; max(c2, c3 ** t) for PR with t = 1, which the decomposed model never advances (:299, model_decompose.py:42)"""
    return c2 if mode == 'kd' or fault == 'pi_c2' else max(c2, c3 ** t)


def step_on_table(w, x, lengths, labels, re, mode, c1, pi, nl='none', farnn=0, sig_k=5.0, dtype=torch.float64, fault=None):
    """The step on the library's inputs: w holds Vgen, S1, S2, W, C, h0, hT, optionally P, trans and the gates (numpy); re is
    [B, L, K].  Returns (loss, {name: grad}, scores [B, L, K])."""
    q = {k: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(k != 'P') for k, v in w.items() if v is not None}
    x = np.asarray(x)
    s = all_scores(q['Vgen'], q['S1'], q['S2'], q['W'], q['C'], q['h0'], q['hT'], x, lengths, nl, q.get('P'), gates=q,
                   farnn=farnn, sig_k=sig_k, fault=fault)
    ret = torch.as_tensor(np.asarray(re)).to(dtype)
    loss = pi * original_loss(s, lengths, labels, q.get('trans')) + (1 - pi) * kl_term(s, ret, mode, c1, lengths, fault)
    loss.backward()
    return float(loss.detach()), {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in q.items()
                                  if v.requires_grad}, s.detach().numpy()


def train_step(p, x, lengths, labels, re_tags, mode, c1, c2, c3, nl='none', additional_nonlinear='none', use_priority=False,
               farnn=0, sig_k=5.0, dtype=torch.float64, fault=None):
    """p: the reference's parameters by name (+ 'priority_mat', 'crf.transitions', gates); re_tags: the raw [B, L_pad, C]
    teacher scores.  Returns (loss, {name: grad})."""
    q = {k: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(k != 'priority_mat') for k, v in p.items()}
    Lmax = int(np.asarray(lengths).max())
    x = np.asarray(x)[:, :Lmax]
    labels = np.asarray(labels)[:, :Lmax]
    trans = q.get('crf.transitions')
    Vgen = to.generalized_table(q, additional_nonlinear)
    s = all_scores(Vgen, q['S1'], q['S2'], q['wildcard_mat'], q['C_output_mat'], q['h0'], q['hT'], x, lengths, nl,
                   q['priority_mat'] if use_priority else None, gates=q, farnn=farnn, sig_k=sig_k, fault=fault)
    ret = torch.as_tensor(pad_and_cut(np.asarray(re_tags), trans is not None, Lmax)).to(dtype)
    pi = weight_of_original(mode, c2, c3, fault)
    loss = pi * original_loss(s, lengths, labels, trans) + (1 - pi) * kl_term(s, ret, mode, c1, lengths, fault)
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in q.items() if v.grad is not None}
