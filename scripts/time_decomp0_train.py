"""Timing of the decomposed FST's training step (farnn_decomp_fst_train_step) at the shape of bench.py's
`decomp0` workload: V = 11 000, S = 104, 73 labels, rank 50, wildcard rank 70, tanh, B = 256, L = 64 with ragged lengths,
rotating through four batches of the same lengths.  Prints one JSON line:

  lib_us_per_step     HIP-event time of the library step (farnn_decomp_fst_train_time): median of the per-step times, with
  lib_us_min / _max   their spread
  stage_us            (--stages 1) torch.profiler's device time per kernel name over the timed steps, divided by the steps,
                      largest first, and `dominant` the first of them; a run of its own, after the event-timed steps
  result_sha          sha256 over the loss and every gradient of the last timed step (bytes)
  torch_us_per_step   the float32 torch restatement of the same step (forward + backward, batched over the sequences, on the
                      same device), wall time per step between two synchronizes, median; torch_loss its loss

    python scripts/time_decomp0_train.py [--steps 10] [--warmup 2] [--stages 1] [--use_crf 0|1] [--farnn 0|1|2] [--semiring sum|max]

--semiring max times the max-semiring step (farnn_decomp_fst_train_set_semiring) against the same restatement with the two
recurrences through torch.max.

The line carries no rate: none was measured.  Each GPU step of a job script runs it under its own time limit
(timeout -k 10 ...)."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_step(torch, w, gates, trans, x, lens, labels, farnn, k=5.0, mx=False):
    """the step restated in torch on the device, float32: loss (backward is the caller's)"""
    Vgen, Ce, S1, S2, Cw, S1w, S2w, WW, h0, hT = w
    B, L = x.shape
    rtab = Vgen * Ce.sum(0)
    W = (S1w * Cw.sum(0)) @ S2w.t() + WW
    idx = torch.arange(L, device=x.device)
    src = torch.where(idx[None, :] < lens[:, None], lens[:, None] - 1 - idx[None, :], idx[None, :])
    xr = torch.gather(x, 1, src)

    def step(h, hin, r, M1, M2, Wm):
        hbar, z = h, None
        if farnn >= 1:
            z = torch.sigmoid(k * (h @ gates[0] + r @ gates[1] + gates[2]))
        if farnn == 2:
            g = torch.sigmoid(k * (h @ gates[3] + r @ gates[4] + gates[5]))
            hbar = (1 - g) * hin + g * h
        if mx:          # Tr[b, j, s] = sum_r M2[s, r] r[b, r] M1[j, r] + Wm[j, s];  n[s] = max_j hbar[j] Tr[j, s]
            Tr = torch.einsum('sr,bjr->bjs', M2, r[:, None, :] * M1[None]) + Wm
            n = torch.tanh((hbar.unsqueeze(2) * Tr).max(1).values)
        else:
            n = torch.tanh(((hbar @ M1) * r) @ M2.t() + hbar @ Wm)
        return n if z is None else (1 - z) * h + z * n

    a0, b0 = h0.expand(B, -1), hT.expand(B, -1)
    f, b = [a0], [b0]
    for t in range(L):
        f.append(step(f[-1], a0, rtab[x[:, t]], S1, S2, W))
        b.append(step(b[-1], b0, rtab[xr[:, t]], S2, S1, W.t()))
    F, Bs = torch.stack(f, 1), torch.stack(b, 1)
    bidx = (lens[:, None] - 1 - idx[None, :]).clamp(min=0)
    alpha, beta = F[:, :L], torch.gather(Bs, 1, bidx.unsqueeze(-1).expand(B, L, Bs.shape[-1]))
    sc = (Vgen[x] * (alpha @ S1) * (beta @ S2)) @ Ce.t() + ((alpha @ S1w) * (beta @ S2w)) @ Cw.t()
    valid = idx[None, :] < lens[:, None]
    if trans is None:
        return torch.nn.functional.cross_entropy(sc[valid], labels[valid])
    K = sc.shape[2]
    al = sc[:, 0] + trans[K - 2]
    gold = sc[:, 0].gather(1, labels[:, :1]).squeeze(1) + trans[K - 2, labels[:, 0]]
    for t in range(1, L):
        live = valid[:, t]
        nxt = torch.logsumexp(al[:, :, None] + trans[None], 1) + sc[:, t]
        al = torch.where(live[:, None], nxt, al)
        gold = gold + torch.where(live, sc[:, t].gather(1, labels[:, t:t + 1]).squeeze(1) + trans[labels[:, t - 1], labels[:, t]],
                                  torch.zeros_like(gold))
    last = labels.gather(1, (lens - 1).clamp(min=0)[:, None]).squeeze(1)
    return (torch.logsumexp(al + trans[:, K - 1], 1) - (gold + trans[last, K - 1])).sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--stages', type=int, default=1)
    ap.add_argument('--use_crf', type=int, default=0)
    ap.add_argument('--farnn', type=int, choices=(0, 1, 2), default=0)
    ap.add_argument('--semiring', choices=('sum', 'max'), default='sum')
    a = ap.parse_args()
    import torch
    from re2nn_seq_amd import _lib, synth
    from re2nn_seq_amd.farnn.train_step import decomp_fst_train_step
    V, S, C, R, Q, B, L = 11000, 104, 73, 50, 70, 256, 64
    rng = np.random.RandomState(1234)
    p = synth.random_decomposed_params(V, S, C, R, 100, rng, contractive=True)
    f = lambda *shape, sc=0.2: (rng.randn(*shape) * sc).astype(np.float32)      # noqa: E731
    x0, lengths = synth.random_batch(V, B, L, rng, min_len=1)
    xs = [x0]
    for k in range(1, 4):                         # same lengths, tokens drawn afresh (bench.py batch_variants)
        r = np.random.RandomState(4321 + 7919 * k)
        xk, _ = synth.random_batch(V, B, L, r, min_len=L, full_length_rows=B)
        xk[np.arange(L)[None, :] >= lengths[:, None]] = V - 1
        xs.append(xk)
    labels = [rng.randint(0, C, size=(B, L)).astype(np.int64) for _ in xs]
    K = C + 2 * a.use_crf
    Cm = rng.randn(K, R) * 0.5                    # bench.py's decomp0 label factors: every column of C_embed sums to 1
    Cm = Cm - Cm.mean(0) + 1.0 / K
    trans = None
    if a.use_crf:
        trans = np.zeros((K, K), np.float32)
        trans[:, K - 2] = -10000.0
        trans[K - 1, :] = -10000.0
        trans += np.where(trans > -5000.0, np.random.RandomState(99).uniform(-0.5, 0.5, size=(K, K)), 0.0).astype(np.float32)
    ntok = int(lengths.sum())
    dev = torch.device('cuda', 0)
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev).requires_grad_(True)      # noqa: E731
    ws = [d(p['V_embed']), d(Cm), d(p['S1']), d(p['S2']), d(f(K, Q, sc=0.3 / np.sqrt(K))), d(f(S, Q, sc=0.2 / np.sqrt(Q))),
          d(f(S, Q, sc=0.2 / np.sqrt(Q))), d(p['wildcard_mat']), d(p['start_vector']), d(p['final_vector'])]
    xd = [torch.from_numpy(v).to(dev) for v in xs]
    ld = torch.from_numpy(lengths).to(dev)
    labd = [torch.from_numpy(v).to(dev) for v in labels]
    tc = _lib.DecompFstTrainContext(V, S, R, Q, K, nl='tanh', device=0, use_crf=bool(a.use_crf), farnn=a.farnn, sigmoid_exponent=5.0)
    if a.semiring == 'max':
        tc.set_semiring('max')
    td = None if trans is None else d(trans)
    gr = np.random.RandomState(77)
    gates = []
    for _ in range(a.farnn):
        gates += [d(gr.randn(S, S) * 0.3 / np.sqrt(S)), d(gr.randn(R, S) * 0.3 / np.sqrt(R)), d(gr.randn(S) * 0.2)]
    leaves = ws + gates + ([td] if td is not None else [])

    def one(i):
        for t in leaves:
            t.grad = None
        loss, _ = decomp_fst_train_step(tc, *ws, None, xd[i % 4], ld, labd[i % 4], crf_trans=td, gates=tuple(gates), valid_tokens=ntok)
        loss.backward()
        return loss

    def one_torch(i):
        for t in leaves:
            t.grad = None
        loss = torch_step(torch, ws, gates, td, xd[i % 4], ld, labd[i % 4], a.farnn, mx=a.semiring == 'max')
        loss.backward()
        return loss

    for i in range(a.warmup):
        one(i)
    torch.cuda.synchronize()
    tc.time()
    tc.set_profiling(1)
    per = []
    for i in range(a.steps):
        loss = one(i)
        ms, n = tc.time()
        per.append(1e3 * ms / max(n, 1))
    tc.set_profiling(0)
    sha = hashlib.sha256(loss.detach().cpu().numpy().tobytes())
    for t in leaves:
        sha.update(t.grad.cpu().numpy().tobytes())
    out = {'shape': {'V': V, 'S': S, 'K': K, 'R': R, 'Q': Q, 'B': B, 'L': L, 'nl': 'tanh'}, 'valid_tokens': ntok, 'steps': a.steps,
           'use_crf': a.use_crf, 'farnn': a.farnn, 'semiring': a.semiring, 'result_sha': sha.hexdigest()[:16], 'lib_us_per_step': float(np.median(per)),
           'lib_us_min': float(min(per)), 'lib_us_max': float(max(per)), 'loss': float(loss.detach())}
    if a.stages:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for i in range(a.steps):
                one(i)
            torch.cuda.synchronize()
        rows = sorted(((getattr(e, 'device_time_total', 0) or getattr(e, 'cuda_time_total', 0)) / a.steps, e.key)
                      for e in prof.key_averages())[::-1][:8]
        out['stage_us'] = [[k.split('(')[0][-60:], round(t, 1)] for t, k in rows if t > 0]
        out['dominant'] = out['stage_us'][0][0] if out['stage_us'] else None
    tper = []
    for i in range(2 + 3):                          # two warm-up steps, then three timed ones
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tl = one_torch(a.steps - 1)                 # the batch the library's last timed step read: torch_loss stands beside loss
        torch.cuda.synchronize()
        if i >= 2:
            tper.append(1e6 * (time.perf_counter() - t0))
    out.update(torch_us_per_step=float(np.median(tper)), torch_loss=float(tl.detach()))
    print(json.dumps(out, sort_keys=True))


if __name__ == '__main__':
    main()
