"""Timing of the onehot independent=1 training step (farnn_ind1_train_step) at the shape of bench.py's
`fst4` workload: V = 950, S = 71, C = 128, B = 256, L = 64 with ragged lengths, rotating through four batches of the same
lengths.  Prints one JSON line:

  lib_us_per_step     HIP-event time of the library step (farnn_ind1_train_time): median of the per-step times, with
  lib_us_min / _max   their spread
  o_mb                the bytes of output_tensor a workgroup of a score pass streams (C S S 4; shared by every workgroup)
  cpu_ms_per_step     (--cpu-steps > 0) the float32 torch restatement (tests/ind1_train_ref.py) forward + backward on 16 CPU
                      threads, on the first --cpu-seqs sequences of a batch

    python scripts/time_ind1_train.py [--steps 20] [--warmup 3] [--mask 0] [--cpu-steps 0] [--cpu-seqs 4]

The line carries no rate: none was measured.  Each GPU step of a job script runs it under its own time limit
(timeout -k 10 ...)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--train_mode', choices=('sum', 'max'), default='sum')       # the semiring of the chains
    ap.add_argument('--mask', type=int, default=0)
    ap.add_argument('--cpu-steps', type=int, default=0)
    ap.add_argument('--cpu-seqs', type=int, default=4)
    a = ap.parse_args()
    import torch
    from re2nn_seq_amd import _lib, synth
    from re2nn_seq_amd.farnn.train_step import onehot_ind1_train_step
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
    # the independent=1 layout of the automaton: label c on the edges into the states with O[c, j] = 1
    Td, Wd = d(T).requires_grad_(True), d(W)
    Oten = d(np.broadcast_to(O[:, None, :], (C, S, S)))
    h0d, hTd = d(h0), d(hT)
    xd = [torch.from_numpy(v).to(dev) for v in xs]
    ld = torch.from_numpy(lengths).to(dev)
    labd = [torch.from_numpy(v).to(dev) for v in labels]
    tc = _lib.Ind1TrainContext(V, S, C, mask_by_output=bool(a.mask), device=0, semiring=a.train_mode)

    def one(i):
        Td.grad = None
        loss, _ = onehot_ind1_train_step(tc, Td, Wd, Oten, h0d, hTd, None, xd[i % 4], ld, labd[i % 4], valid_tokens=ntok)
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
    out = {'shape': {'V': V, 'S': S, 'C': C, 'B': B, 'L': L}, 'valid_tokens': ntok, 'steps': a.steps, 'mask_by_output': a.mask, 'train_mode': a.train_mode,
           'lib_us_per_step': float(np.median(per)), 'lib_us_min': float(min(per)), 'lib_us_max': float(max(per)),
           'distinct_words': words, 'o_mb': C * S * S * 4 / 1e6, 'loss': float(loss.detach())}
    if a.cpu_steps > 0:
        import ind1_train_ref as itr
        torch.set_num_threads(16)
        n = a.cpu_seqs
        kw = dict(T=T, W=W, O=Oten.cpu().numpy(), h0=h0, hT=hT, P=None, x=xs[0][:n], lengths=lengths[:n], labels=labels[0][:n],
                  mask=bool(a.mask), dtype=torch.float32)
        itr.step(**kw)
        t0 = time.perf_counter()
        for _ in range(a.cpu_steps):
            itr.step(**kw)
        out['cpu_ms_per_step'] = 1e3 * (time.perf_counter() - t0) / a.cpu_steps
        out['cpu_tokens'] = int(lengths[:n].sum())
    print(json.dumps(out, sort_keys=True))


if __name__ == '__main__':
    main()
