"""Timing of the optimizer step alone: torch.optim.Adam against the library's one-launch step
(re2nn_seq_amd.farnn.optim.Adam) and a plain device copy as the floor, in one process, at

  onehot   the onehot i-FST's only trained tensor at the headline shape: language_tensor [950, 71, 71] (19 MB)
  decomp   every tensor the decomposed i-FST can train at the shipped shape (V = 11000, S = 104, R = 250, K = 75 score
           columns, embedding width 100, farnn 2, CRF): 17 tensors from 104 floats to [11000, 250]

Prints one JSON line.  Per shape and per contender (`torch`, `native`, `copy`):

  us            median over --reps repetitions of the HIP-event time of one repetition / --inner back-to-back steps
  iqr_us        the interquartile range of those repetitions (the spread), min_us / max_us beside it
  cold_us ...   the same with ONE step per event pair and a 512 MiB buffer rewritten in front of every timed step (the
                parameters, gradients and moments of either shape fit the 256 MiB Infinity Cache: back-to-back steps find
                them there, a step behind a training step's traffic finds less)

The three contenders alternate inside every repetition.  An Adam step reads 4 arrays and writes 3; `copy` is one
dst.copy_(src) of 3.5 x the parameter bytes, so it moves the same 7 x bytes (`bytes_moved`).  `bar` (shape onehot): the
library's median must beat torch's by more than the larger of the two spreads; the script exits 1 if it does not.

    python scripts/time_native_optim.py [--reps 15] [--inner 20] [--warmup 3]

Each GPU step of a job script runs it under its own time limit (timeout -k 10 ...)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes():
    V, S, R, K, D = 11000, 104, 250, 75, 100
    decomp = [(S, R), (S, R), (D, R), (V, R), (K, S), (S, S), (S,), (S,), (R,), (V, D),      # _TRAIN_FLAGS of FARNN_S_D_W_I_S
              (S, S), (R, S), (S,), (S, S), (R, S), (S,),                                    # the gates of farnn 2
              (K, K)]                                                                        # crf.transitions
    return {'onehot': [(950, 71, 71)], 'decomp': decomp}


def _stats(us):
    q1, med, q3 = np.percentile(us, [25, 50, 75])
    return dict(us=round(float(med), 2), iqr_us=round(float(q3 - q1), 2), min_us=round(float(min(us)), 2), max_us=round(float(max(us)), 2))


def measure(shape_list, a):
    import torch
    from re2nn_seq_amd.farnn import optim
    dev = torch.device('cuda', 0)
    rng = np.random.RandomState(99)

    def make():
        ps = [torch.from_numpy(rng.randn(*s).astype(np.float32)).to(dev).requires_grad_(True) for s in shape_list]
        for p in ps:
            p.grad = torch.from_numpy((rng.randn(*p.shape) * 0.1).astype(np.float32)).to(dev)
        return ps
    pt, pn = make(), make()
    ot, on = torch.optim.Adam(pt, lr=1e-3, weight_decay=0), optim.Adam(pn, lr=1e-3, weight_decay=0)
    nbytes = 4 * sum(p.numel() for p in pt)
    ncopy = (7 * nbytes // 2 + 3) // 4
    src, dst = torch.zeros(ncopy, device=dev), torch.empty(ncopy, device=dev)
    flush = torch.empty(128 * 1024 * 1024, dtype=torch.float32, device=dev)            # 512 MiB
    fns = {'torch': ot.step, 'native': on.step, 'copy': lambda: dst.copy_(src)}
    for _ in range(a.warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()

    def timed(f, inner, cold):
        if cold:
            flush.fill_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            f()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / inner
    warm = {k: [] for k in fns}
    cold = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, f in fns.items():
            warm[k].append(timed(f, a.inner, False))
        for k, f in fns.items():
            cold[k].append(timed(f, 1, True))
    out = dict(tensors=len(shape_list), param_bytes=nbytes, bytes_moved=7 * nbytes)
    for k in fns:
        out[k] = dict(_stats(warm[k]), **{'cold_' + n: v for n, v in _stats(cold[k]).items()})
    out['native_over_torch'] = round(out['native']['us'] / out['torch']['us'], 3)
    out['native_over_copy'] = round(out['native']['us'] / out['copy']['us'], 3)
    out['native_GBps'] = round(7 * nbytes / out['native']['us'] / 1e3, 1)
    out['native_cold_GBps'] = round(7 * nbytes / out['native']['cold_us'] / 1e3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('time_native_optim.py needs the GPU: a timing taken anywhere else says nothing')
    out = dict(workload='native_optim', reps=a.reps, inner=a.inner, device=torch.cuda.get_device_name(0))
    for name, sl in shapes().items():
        out[name] = measure(sl, a)
    o = out['onehot']
    gain, spread = o['torch']['us'] - o['native']['us'], max(o['torch']['iqr_us'], o['native']['iqr_us'])
    out['bar'] = dict(shape='onehot', gain_us=round(gain, 2), spread_us=round(spread, 2), passed=bool(gain > spread))
    print(json.dumps(out))
    sys.exit(0 if out['bar']['passed'] else 1)


if __name__ == '__main__':
    main()
