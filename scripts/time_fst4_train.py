"""Timing of the onehot FST training step (farnn_fst4_train_step) at the shape of bench.py's `fst4` workload:
V = 950, S = 71, C = 128, B = 256, L = 64 with ragged lengths, rotating through four batches of the same lengths.  Prints one
JSON line:

  lib_us_per_step     HIP-event time of the library step (farnn_fst4_train_time): median of the per-step times, with
  lib_us_min / _max   their spread
  block_gb            the bytes of the blocks one pass of a score kernel streams (T4 rows of the batch's words + W4)
  kernels             (--kernel-stats FILE: the kernel_stats csv of a `rocprofv3 --kernel-trace --stats` run of this script made
                      on its own) calls and average microseconds per kernel name; score_forward / score_adjoints / score_dT4: the
                      three passes of fst4_train_kernel with block_gb over their time in TB/s (score_dT4 also writes dT4: twice
                      the bytes), beside yardstick_tb_s, the tagging fst4_score_kernel's measured rate (DESIGN.md section 6:
                      22.2 GB in 3.03 ms).  Without the option the line carries no rate: none was measured
  cpu_ms_per_step     (--cpu-steps > 0) the float32 torch restatement (tests/fst4_train_ref.py) forward + backward on 16 CPU
                      threads, on the first --cpu-seqs sequences of a batch (the products of a whole batch do not fit a host)

    python scripts/time_fst4_train.py [--steps 20] [--warmup 3] [--cpu-steps 0] [--cpu-seqs 4] [--wildcard 1] [--kernel-stats FILE]

The tensors are generated on the device (T4 alone is 2.45 GB).  Each GPU step of a job script runs it under its own time
limit (timeout -k 10 ...)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


YARDSTICK_TB_S = 22.2 / 3.03          # fst4_score_kernel, DESIGN.md section 6


def kernel_stats(path, block_gb):
    """per-kernel calls / average us of a rocprofv3 kernel_stats csv; the score passes' rates"""
    import csv
    import re
    out = {'kernels': {}, 'yardstick_tb_s': YARDSTICK_TB_S}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get('Name') or row.get('KernelName') or ''
            short = re.sub(r'\(.*$', '', name).replace('void ', '').replace('farnn::', '')
            out['kernels'][short] = {'calls': int(row['Calls']), 'avg_us': float(row['AverageNs']) / 1e3}
            m = re.search(r'fst4_train_kernel<\d+, (\d)>', name)
            if m:
                key = ('score_forward', 'score_adjoints', 'score_dT4')[int(m.group(1))]
                gb = block_gb * (2 if key == 'score_dT4' else 1)
                out[key] = {'us': float(row['AverageNs']) / 1e3, 'gb': gb, 'tb_s': gb / (float(row['AverageNs']) / 1e9) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--train_mode', choices=('sum', 'max'), default='sum')       # the semiring of the chains
    ap.add_argument('--cpu-steps', type=int, default=0)
    ap.add_argument('--cpu-seqs', type=int, default=4)
    ap.add_argument('--wildcard', type=int, default=1)
    ap.add_argument('--kernel-stats', default=None)
    a = ap.parse_args()
    import torch
    from re2nn_seq_amd import _lib, synth
    from re2nn_seq_amd.farnn.train_step import onehot_fst4_train_step
    V, S, C, B, L = 950, 71, 128, 256, 64
    rng = np.random.RandomState(1234)
    T, W, O, h0, hT = synth.random_ifst_tensors(V, S, C, rng)
    x0, lengths = synth.random_batch(V, B, L, rng)
    xs = [x0]
    for k in range(1, 4):                         # same lengths, tokens drawn afresh (bench.py batch_variants)
        r = np.random.RandomState(4321 + 7919 * k)
        xk, _ = synth.random_batch(V, B, L, r, min_len=L, full_length_rows=B)
        xk[np.arange(L)[None, :] >= lengths[:, None]] = V - 1
        xs.append(xk)
    labels = [rng.randint(0, C, size=(B, L)).astype(np.int64) for _ in xs]
    ntok = int(lengths.sum())
    dev = torch.device('cuda', 0)
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)      # noqa: E731
    # the 4-D layout of the automaton, as bench.py builds it: label c on the edges into the states with O[c, j] = 1
    Td, Wd, Od = d(T), d(W), d(O)
    T4 = torch.einsum('vsj,cj->vcsj', Td, Od).contiguous().requires_grad_(True)
    W4 = torch.einsum('sj,cj->csj', Wd, Od).contiguous().requires_grad_(bool(a.wildcard))
    h0d, hTd = d(h0), d(hT)
    xd = [torch.from_numpy(v).to(dev) for v in xs]
    ld = torch.from_numpy(lengths).to(dev)
    labd = [torch.from_numpy(v).to(dev) for v in labels]
    tc = _lib.Fst4TrainContext(V, S, C, device=0, semiring=a.train_mode)

    def one(i):
        T4.grad = None
        W4.grad = None
        loss, _ = onehot_fst4_train_step(tc, T4, W4, h0d, hTd, None, xd[i % 4], ld, labd[i % 4], valid_tokens=ntok)
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
    words = [int(len(np.unique(v[np.arange(L)[None, :] < lengths[:, None]]))) for v in xs]
    out = {'shape': {'V': V, 'S': S, 'C': C, 'B': B, 'L': L}, 'valid_tokens': ntok, 'steps': a.steps, 'train_wildcard': a.wildcard, 'train_mode': a.train_mode,
           'lib_us_per_step': float(np.median(per)), 'lib_us_min': float(min(per)), 'lib_us_max': float(max(per)),
           'distinct_words': words, 'block_gb': (float(np.mean(words)) + 1) * C * S * S * 4 / 1e9, 'loss': float(loss.detach())}
    if a.kernel_stats:
        out.update(kernel_stats(a.kernel_stats, out['block_gb']))
    if a.cpu_steps > 0:
        import fst4_train_ref as ftr
        torch.set_num_threads(16)
        n = a.cpu_seqs
        kw = dict(T4=T4.detach().cpu().numpy(), W4=W4.detach().cpu().numpy(), h0=h0, hT=hT, P=None, x=xs[0][:n], lengths=lengths[:n],
                  labels=labels[0][:n], dtype=torch.float32)
        ftr.step(**kw)
        t0 = time.perf_counter()
        for _ in range(a.cpu_steps):
            ftr.step(**kw)
        out['cpu_ms_per_step'] = 1e3 * (time.perf_counter() - t0) / a.cpu_steps
        out['cpu_tokens'] = int(lengths[:n].sum())
    print(json.dumps(out, sort_keys=True))


if __name__ == '__main__':
    main()
