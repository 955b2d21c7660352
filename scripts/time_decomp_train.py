"""Timing of the decomposed i-FST training step (farnn_decomp_ifst_train_step) in both semirings at the
same shape: bench.py's `train` workload (SNIPS-sized V = 11000, S = 104, K = 73) with rank 250, farnn 2 and the CRF loss,
batch 256 x seqlen 64.  Prints one JSON line with, per semiring,

  lib_us_per_step     HIP-event time of the library step (farnn_train_time)
  step_us_per_step    the whole step as a training loop runs it: zero_grad, word table, the step, backward, Adam
  max_over_sum        the ratio of the library times

    python scripts/time_decomp_train.py [--steps 20] [--warmup 3] [--states 104] [--rank 250] [--farnn 2] [--crf 1]

Each GPU step of a job script runs it under its own time limit (timeout -k 10 ...)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(a, semiring):
    import torch
    from re2nn_seq_amd import _lib, synth
    from re2nn_seq_amd.farnn.train_step import decomp_ifst_train_step
    V, S, K, R, B, L = 11000, a.states, 73 + (2 if a.crf else 0), a.rank, 256, 64
    wrng, brng = np.random.RandomState(1234), np.random.RandomState(4321)
    dev = torch.device('cuda', 0)

    def f(*shape, sc=0.3):
        return torch.from_numpy((wrng.randn(*shape) * sc).astype(np.float32)).to(dev).requires_grad_(True)
    Cm = np.zeros((K, S), np.float32)
    Cm[wrng.randint(0, K - (2 if a.crf else 0), size=S), np.arange(S)] = 1
    p = dict(S1=f(S, R, sc=0.1), S2=f(S, R, sc=0.1), Vgen=f(V, R, sc=0.8),
             C=torch.from_numpy(Cm).to(dev).requires_grad_(True),
             W=torch.from_numpy(((wrng.rand(S, S) < 1.0 / S) * 0.5).astype(np.float32)).to(dev).requires_grad_(True),
             h0=f(S, sc=0.5), hT=f(S, sc=0.5))
    gate_names = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')[:3 * a.farnn]
    for n in gate_names:
        p[n] = f(S, sc=0.5) if n.startswith('bs') else (f(S, S, sc=1.0 / np.sqrt(S)) if n.startswith('Wss') else f(R, S, sc=1.0 / np.sqrt(R)))
    if a.crf:
        tr = np.zeros((K, K), np.float32)
        tr[:, K - 2] = -10000.0
        tr[K - 1, :] = -10000.0
        p['trans'] = torch.from_numpy(tr).to(dev).requires_grad_(True)
    x, lengths = synth.random_batch(V, B, L, brng)
    labels = brng.randint(0, K - (2 if a.crf else 0), size=(B, L)).astype(np.int64)
    xd, ld, lab = torch.from_numpy(x).to(dev), torch.from_numpy(lengths).to(dev), torch.from_numpy(labels).to(dev)
    tc = _lib.TrainContext(V, S, R, K, nl='tanh', threshold=0.5, o_idx=0, use_crf=a.crf, farnn=a.farnn, sigmoid_exponent=5.0,
                           semiring=semiring)
    ntok = int(lengths.sum())
    opt = torch.optim.Adam(list(p.values()), lr=1e-4)

    def one():
        opt.zero_grad(set_to_none=True)
        loss, _ = decomp_ifst_train_step(tc, p['Vgen'], p['S1'], p['S2'], p['W'], p['C'], p['h0'], p['hT'], None, xd, ld, lab,
                                         crf_trans=p.get('trans'), gates=tuple(p[n] for n in gate_names), valid_tokens=ntok)
        loss.backward()
        opt.step()
        return loss

    for _ in range(a.warmup):
        one()
    torch.cuda.synchronize()
    tc.set_profiling(1)
    tc.time()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        loss = one()
    e1.record()
    torch.cuda.synchronize()
    lib_ms, n = tc.time()
    tc.close()
    return dict(lib_us_per_step=round(1e3 * lib_ms / max(n, 1), 1), step_us_per_step=round(1e3 * e0.elapsed_time(e1) / a.steps, 1),
                final_loss=float(loss.detach())), ntok, (V, S, R, K, B, L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--states', type=int, default=104)
    ap.add_argument('--rank', type=int, default=250)
    ap.add_argument('--farnn', type=int, default=2)
    ap.add_argument('--crf', type=int, default=1)
    a = ap.parse_args()
    out = {}
    for semiring in ('sum', 'max'):
        out[semiring], ntok, shape = run(a, semiring)
    V, S, R, K, B, L = shape
    print(json.dumps(dict(workload='decomp_train', V=V, S=S, R=R, K=K, B=B, L=L, farnn=a.farnn, crf=bool(a.crf),
                          valid_tokens=ntok, steps=a.steps, sum=out['sum'], max=out['max'],
                          max_over_sum=round(out['max']['lib_us_per_step'] / out['sum']['lib_us_per_step'], 2))))


if __name__ == '__main__':
    main()
