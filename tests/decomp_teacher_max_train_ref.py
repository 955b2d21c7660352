"""Test infrastructure: one training step of the decomposed i-FST with the KD / PR teacher term in the MAX semiring
(--train_mode max --marryup_type kd | pr), restated in plain torch with autograd on the CPU, in float64 or float32.

    forward_local(train=True, re_tags=...)   reference model_decompose_single.py:207-304
    get_forward_score, train_mode = 'max'    reference model_decompose_single.py:156-166, utils._maxmul (utils.py:192-195)
    KD_loss, PR_loss                         reference baselines/KD.py:3-18

The pieces are the two restatements this one joins: all the loss side -- kl_term, original_loss, pad_and_cut,
weight_of_original, and which stash row a position reads -- is decomp_teacher_train_ref.py's; the chain step is the sum
step's with its product replaced by decomp_max_train_ref.maxmul (torch.max: ONE source state per target state, the first
maximal one), its min_gap check included.  Both chains of every sequence run L = x.shape[1] steps: the forward chain over
x[b, :], the backward chain over the len reversed tokens and then the raw pad tokens x[b, len:].

The arg-max gap rule (check_gap; the rule of max_chains_ref.check_argmax_gap) over ALL L steps of every sequence, since with
a teacher every step reaches a score: a non-zero maximum beats the runner-up by min_gap relative, in float32 AND in float64,
or ties it EXACTLY in both.  Exact-zero maxima are exempt.

`fault` plants one deliberate mistake (the CPU tests show that the fixtures and the drawn cases see each of them):
    'stop_at_len'    both chains stop at len, as the plain max step's kernels do: the rows past len stay zero
    'tail_reversed'  the backward chain reads its tail tokens x[b, len:] reversed
    'pad_row'        the backward chain's dTr entry of a pad position i is looked up at row len - i instead of i + 1: rows <= 0
                     hold no entry of that sequence (row 0 is never written), so the word loses what its pad steps send to Tr
    'sum'            sum-times chains
    'last'           the last maximal index instead of the first
"""
import numpy as np
import torch

import decomp_max_train_ref as dmr
import decomp_teacher_train_ref as dtr
from oracle import farnn_train_oracle as to

FAULTS = ('stop_at_len', 'tail_reversed', 'pad_row', 'sum', 'last')
GapError = dmr.GapError


def _maxmul(h, Tr, min_gap, fault, tops):
    temp = h[:, None] * Tr
    if tops is not None and temp.shape[0] > 1:
        tops.append(torch.topk(temp.detach(), 2, dim=0).values)
    if fault == 'last':
        S = temp.shape[0]
        idx = S - 1 - torch.max(temp.flip(0), dim=0)[1]
        return torch.gather(temp, 0, idx[None, :])[0]
    return dmr.maxmul(h, Tr, min_gap)


def _step(S1, S2, W, osum, nl, gates, farnn, sig_k, min_gap=None, fault=None, tops=None):
    """get_forward_score with train_mode = 'max' (:138-200); `pad`: a backward step over a pad token (fault 'pad_row')"""
    if fault == 'sum':
        return lambda h, v, h_init, fwd, pad=False: dtr._step(S1, S2, W, osum, nl, gates, farnn, sig_k)(h, v, h_init, fwd)

    def step(h, v, h_init, fwd, pad=False):
        if farnn >= 1:
            z = torch.sigmoid(sig_k * (h @ gates['Wss1'] + v @ gates['Wrs1'] + gates['bs1'].reshape(-1)))
        hbar = h
        if farnn == 2:
            r = torch.sigmoid(sig_k * (h @ gates['Wss2'] + v @ gates['Wrs2'] + gates['bs2'].reshape(-1)))
            hbar = (1 - r) * h_init + r * h
        Tr = (v * S1) @ S2.T + W                                      # Tr[j, s] = sum_r S2[s, r] v[r] S1[j, r] + W[j, s]
        if fwd:
            nxt = to._nl(_maxmul(hbar, Tr, min_gap, fault, tops) * osum, nl)
        else:
            if pad and fault == 'pad_row':
                Tr = Tr.detach()
            nxt = to._nl(_maxmul(hbar * osum, Tr.T, min_gap, fault, tops), nl)
        return nxt if farnn == 0 else (1 - z) * h + z * nxt
    return step


def all_scores(Vgen, S1, S2, W, C, h0, hT, x, lengths, nl='none', P=None, gates=None, farnn=0, sig_k=5.0, fault=None,
               min_gap=None, tops=None):
    """[B, L, K] with L = x.shape[1]: every position's scores, pads included, after the priority layer."""
    step = _step(S1, S2, W, C.sum(0), nl, gates, farnn, sig_k, min_gap, fault, tops)
    B, L = x.shape
    rows = []
    for b in range(B):
        n = int(lengths[b])
        toks = [int(t) for t in x[b]]
        tail = toks[n:][::-1] if fault == 'tail_reversed' else toks[n:]
        steps = n if fault == 'stop_at_len' else L
        f = [h0]
        for t in toks[:steps]:
            f.append(step(f[-1], Vgen[t], h0, True))
        bk = [hT]
        for i, t in enumerate((toks[:n][::-1] + tail)[:steps]):
            bk.append(step(bk[-1], Vgen[t], hT, False, pad=i >= n))
        zero = torch.zeros_like(h0)
        f += [zero] * (L - steps)
        bk += [zero] * (L - steps)
        # valid: alpha row i+1 and backward row n-1-i; pad: row i+1 of both; backward row n is read by nobody
        rows.append(torch.stack([(f[i + 1] * bk[n - 1 - i if i < n else i + 1]) @ C.T for i in range(L)]))
    s = torch.stack(rows)
    return s @ P if P is not None else s


def check_gap(w, x, lengths, nl='none', farnn=0, sig_k=5.0, min_gap=2e-5):
    """The arg-max gap rule over all L steps of both chains of every sequence, on the library's inputs (w as step_on_table
    takes it).  Raises GapError."""
    ev = {}
    for dtype in (torch.float32, torch.float64):
        q = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in w.items() if v is not None}
        tops = []
        with torch.no_grad():
            all_scores(q['Vgen'], q['S1'], q['S2'], q['W'], q['C'], q['h0'], q['hT'], np.asarray(x), lengths, nl, q.get('P'),
                       gates=q, farnn=farnn, sig_k=sig_k, tops=tops)
        if not tops:
            return
        ev[dtype] = torch.stack(tops).to(torch.float64)                    # [steps, 2, S]
    tie = (ev[torch.float32][:, 0] == ev[torch.float32][:, 1]) & (ev[torch.float64][:, 0] == ev[torch.float64][:, 1])
    for dtype, e in ev.items():
        top, second = e[:, 0], e[:, 1]
        bad = ~((top == 0) | ((top - second) >= min_gap * top.abs()) | tie)
        if bool(bad.any()):
            raise GapError('{} maxima are decided by less than {} relative in {} without being exact ties in both '
                           'evaluations'.format(int(bad.sum()), min_gap, dtype))


def step_on_table(w, x, lengths, labels, re, mode, c1, pi, nl='none', farnn=0, sig_k=5.0, dtype=torch.float64, fault=None,
                  min_gap=None):
    """The step on the library's inputs: w holds Vgen, S1, S2, W, C, h0, hT, optionally P, trans and the gates (numpy); re is
    [B, L, K].  Returns (loss, {name: grad}, scores [B, L, K])."""
    q = {k: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(k != 'P') for k, v in w.items() if v is not None}
    x = np.asarray(x)
    s = all_scores(q['Vgen'], q['S1'], q['S2'], q['W'], q['C'], q['h0'], q['hT'], x, lengths, nl, q.get('P'), gates=q,
                   farnn=farnn, sig_k=sig_k, fault=fault, min_gap=min_gap)
    ret = torch.as_tensor(np.asarray(re)).to(dtype)
    loss = pi * dtr.original_loss(s, lengths, labels, q.get('trans')) + (1 - pi) * dtr.kl_term(s, ret, mode, c1, lengths)
    loss.backward()
    return float(loss.detach()), {k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in q.items()
                                  if v.requires_grad}, s.detach().numpy()


def table_of(p, additional_nonlinear='none', use_priority=False, dtype=torch.float64):
    """the library's inputs of the reference's parameters p (the word table folded), for check_gap"""
    q = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in p.items()}
    w = {'Vgen': to.generalized_table(q, additional_nonlinear), 'S1': q['S1'], 'S2': q['S2'], 'W': q['wildcard_mat'],
         'C': q['C_output_mat'], 'h0': q['h0'], 'hT': q['hT'], 'P': q['priority_mat'] if use_priority else None}
    w.update({k: q[k] for k in ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2') if k in q})
    return {k: (None if v is None else v.numpy()) for k, v in w.items()}


def train_step(p, x, lengths, labels, re_tags, mode, c1, c2, c3, nl='none', additional_nonlinear='none', use_priority=False,
               farnn=0, sig_k=5.0, dtype=torch.float64, fault=None, min_gap=None):
    """p: the reference's parameters by name (+ 'priority_mat', 'crf.transitions', gates); re_tags: the raw [B, L_pad, C]
    teacher scores.  Returns (loss, {name: grad}, scores [B, Lmax, K])."""
    q = {k: torch.as_tensor(np.asarray(v)).to(dtype).clone().requires_grad_(k != 'priority_mat') for k, v in p.items()}
    Lmax = int(np.asarray(lengths).max())
    x = np.asarray(x)[:, :Lmax]
    labels = np.asarray(labels)[:, :Lmax]
    trans = q.get('crf.transitions')
    Vgen = to.generalized_table(q, additional_nonlinear)
    s = all_scores(Vgen, q['S1'], q['S2'], q['wildcard_mat'], q['C_output_mat'], q['h0'], q['hT'], x, lengths, nl,
                   q['priority_mat'] if use_priority else None, gates=q, farnn=farnn, sig_k=sig_k, fault=fault, min_gap=min_gap)
    ret = torch.as_tensor(dtr.pad_and_cut(np.asarray(re_tags), trans is not None, Lmax)).to(dtype)
    pi = dtr.weight_of_original(mode, c2, c3)
    loss = pi * dtr.original_loss(s, lengths, labels, trans) + (1 - pi) * dtr.kl_term(s, ret, mode, c1, lengths)
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in q.items() if v.grad is not None}, s.detach().numpy()
