"""Timing of the onehot i-FST training step (farnn_onehot_ifst_train_step) at the headline shape:
V = 950, S = 71, C = 128, B = 256, L = 64 with ragged lengths, rotating through four batches of the same lengths (as
bench.py's `ifst` workload does).  Prints one JSON line:

  lib_us_per_step     HIP-event time of the library step (farnn_onehot_train_time)
  step_us_per_step    the whole step as a training loop runs it: zero_grad, forward_local(train=True), backward, Adam
                      (torch events around the loop); `optimizer` says which Adam: torch's, or with RE2NN_NATIVE_OPTIM=1
                      the library's one-launch step
  tokens_per_s        valid trained tokens per second of the whole step
  cpu_ms_per_step     the float32 torch restatement (tests/onehot_train_ref.py) forward + backward on 16 CPU threads:
                      the reference trains this model on the CPU (train_onehot.py:75-76)

    python scripts/time_onehot_train.py [--steps 50] [--warmup 5] [--cpu-steps 3] [--states 71] [--semiring max]

--semiring max times the max-semiring step (farnn_onehot_train_set_semiring; the CPU figure is then tests/onehot_train_max_ref.py)
and adds "semiring": "max" to the line; the default line is unchanged.

Each GPU step of a job script runs it under its own time limit (timeout -k 10 ...)."""
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
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--cpu-steps', type=int, default=3)
    ap.add_argument('--states', type=int, default=71)
    ap.add_argument('--semiring', choices=('sum', 'max'), default='sum')
    a = ap.parse_args()
    import torch
    from re2nn_seq_amd import _lib, synth
    from re2nn_seq_amd.farnn._native import opted_in
    from re2nn_seq_amd.farnn.train_step import onehot_ifst_train_step
    V, S, C, B, L = 950, a.states, 128, 256, 64
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
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev)
    Tt = d(T).requires_grad_(True)
    Wd, Od, h0d, hTd = d(W), d(O), d(h0), d(hT)
    xd = [torch.from_numpy(v).to(dev) for v in xs]
    ld = torch.from_numpy(lengths).to(dev)
    labd = [torch.from_numpy(v).to(dev) for v in labels]
    tc = _lib.OnehotTrainContext(V, S, C, nl='none', device=0)
    if a.semiring != 'sum':
        tc.set_semiring(a.semiring)
    native = opted_in('NATIVE_OPTIM')      # as train_onehot.train_epochs picks its optimizer
    if native:
        from re2nn_seq_amd.farnn import optim
    else:
        optim = torch.optim
    opt = optim.Adam([Tt], lr=1e-3, weight_decay=0)

    def one(i):
        opt.zero_grad()
        loss, _ = onehot_ifst_train_step(tc, Tt, Wd, Od, h0d, hTd, None, xd[i % 4], ld, labd[i % 4], valid_tokens=ntok)
        loss.backward()
        opt.step()
        return loss

    for i in range(a.warmup):
        one(i)
    torch.cuda.synchronize()
    tc.time()                                     # discard the warm-up's events
    tc.set_profiling(1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(a.steps):
        loss = one(i)
    e1.record()
    torch.cuda.synchronize()
    step_ms = e0.elapsed_time(e1) / a.steps
    lib_ms, n = tc.time()
    out = dict(workload='onehot_train', V=V, S=S, C=C, B=B, L=L, valid_tokens=ntok, steps=a.steps,
               optimizer='farnn.optim.Adam' if native else 'torch.optim.Adam',
               lib_us_per_step=round(1e3 * lib_ms / max(n, 1), 2), step_us_per_step=round(1e3 * step_ms, 2),
               tokens_per_s=round(ntok / (step_ms * 1e-3), 1), final_loss=float(loss.detach()))
    if a.semiring != 'sum':
        out['semiring'] = a.semiring
    if a.cpu_steps > 0:
        if a.semiring == 'max':
            import onehot_train_max_ref as otr
        else:
            import onehot_train_ref as otr
        torch.set_num_threads(16)
        otr.step(T, W, O, h0, hT, None, xs[0], lengths, labels[0], dtype=torch.float32)
        t0 = time.perf_counter()
        for i in range(a.cpu_steps):
            otr.step(T, W, O, h0, hT, None, xs[i % 4], lengths, labels[i % 4], dtype=torch.float32)
        cpu_ms = 1e3 * (time.perf_counter() - t0) / a.cpu_steps
        out.update(cpu_ms_per_step=round(cpu_ms, 2), cpu_threads=16, cpu_tokens_per_s=round(ntok / (cpu_ms * 1e-3), 1),
                   speedup_vs_cpu=round(cpu_ms / step_ms, 1))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
