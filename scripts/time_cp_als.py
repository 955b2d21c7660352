"""Time the library's CP-ALS sweep (farnn_cp_run) and, beside it, the dense-unfolding numpy sweep on the same machine.

    python scripts/time_cp_als.py [--out profiles/cp_als_timing.json] [--sweeps 8] [--repeats 5] [--numpy_budget_s 240]

Two shapes: synth.planted_rule_ifst() at its default (SNIPS) size squashed to the words that occur, R = 250; and an ATIS-sized
automaton (V = 950, S = 71), R = 150.  Per shape: the milliseconds per sweep of un-profiled runs (wall clock around the call,
the factors' two bus crossings included; median and min .. max over the repeats, after a warm-up run) and the milliseconds per
sweep of each stage from HIP events (a profiled run waits after every stage, so the stages do not add up to the first figure).
The numpy sweep (float64, the machine's BLAS threads as configured) is timed on the larger shape only if one sweep of it fits
the budget.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from re2nn_seq_amd import _lib, synth  # noqa: E402


def squash(word, frm, to):
    """coordinates with the word axis squashed to the words that occur (decompose_tensor_split_slot_3d_language)"""
    words, w = np.unique(word, return_inverse=True)
    return (len(words), int(max(frm.max(), to.max())) + 1), w.astype(np.int32)


def numpy_sweep(X, f):
    normx2 = float(np.sum(X * X))
    other = {0: (1, 2), 1: (0, 2), 2: (0, 1)}
    for n in range(3):
        a, b = other[n]
        R = f[a].shape[1]
        H = (f[a].T @ f[a]) * (f[b].T @ f[b])
        kr = (f[a][:, None, :] * f[b][None, :, :]).reshape(-1, R)
        M = np.moveaxis(X, n, 0).reshape(X.shape[n], -1) @ kr
        f[n] = np.linalg.solve(H.T, M.T).T
    n2 = np.sum((f[0].T @ f[0]) * (f[1].T @ f[1]) * (f[2].T @ f[2]))
    return float(np.sqrt(abs(normx2 + n2 - 2.0 * np.sum(M * f[2])) / normx2))


def time_shape(name, dims, idx, val, R, sweeps, repeats, numpy_budget_s):
    rng = np.random.RandomState(0)
    init = [rng.random_sample((d, R)) for d in dims]
    ctx = _lib.CpContext(dims, idx[0], idx[1], idx[2], val, R)
    ctx.run(R, 2, 0.0, init)                                        # warm-up: code objects, LDS limits, first touches
    wall = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        _, errs = ctx.run(R, sweeps, 0.0, init)
        wall.append((time.perf_counter() - t0) * 1e3 / len(errs))
    ctx.set_profiling(True)
    for _ in range(repeats):
        ctx.run(R, sweeps, 0.0, init)
    stage_ms, n = ctx.time()
    ctx.close()
    out = {'shape': name, 'dims': list(dims), 'nnz': int(len(val)), 'rank': R, 'sweeps_per_run': sweeps, 'repeats': repeats,
           'ms_per_sweep': {'median': float(np.median(wall)), 'min': float(min(wall)), 'max': float(max(wall))},
           'stage_ms_per_sweep': {k: v / n for k, v in stage_ms.items()}, 'timed_sweeps': n, 'last_rec_error': errs[-1]}
    dense_bytes = 8.0 * dims[0] * dims[1] * dims[2]
    if numpy_budget_s > 0 and dense_bytes < 4e9:
        X = np.zeros(dims)
        X[tuple(idx)] = val
        f = [a.copy() for a in init]
        t0 = time.perf_counter()
        numpy_sweep(X, f)                                           # warm-up sweep; also the budget probe
        first = time.perf_counter() - t0
        if first <= numpy_budget_s / 4:
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                numpy_sweep(X, f)
                ts.append((time.perf_counter() - t0) * 1e3)
            out['numpy_dense_ms_per_sweep'] = {'median': float(np.median(ts)), 'min': float(min(ts)), 'max': float(max(ts)),
                                               'threads': int(os.environ.get('OMP_NUM_THREADS', 0)) or None}
        else:
            out['numpy_dense_ms_per_sweep'] = {'skipped': 'one sweep took {:.1f} s'.format(first)}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cp_als_timing.json'))
    p.add_argument('--sweeps', type=int, default=8)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--numpy_budget_s', type=float, default=240.0)
    args = p.parse_args()
    results = []
    T, _, _, _, _ = synth.random_ifst_tensors(950, 71, 128, np.random.RandomState(1234))
    w, a, b = np.nonzero(T)
    dims, w = squash(w, a, b)
    results.append(time_shape('atis_sized V=950 S=71', (dims[0], 71, 71), [w, a.astype(np.int32), b.astype(np.int32)],
                              T[np.nonzero(T)].astype(np.float64), 150, args.sweeps, args.repeats, args.numpy_budget_s))
    A = synth.planted_rule_ifst()
    m = A['word'] >= 0
    dims, w = squash(A['word'][m], A['frm'][m], A['to'][m])
    results.append(time_shape('planted_rule_ifst default (SNIPS size)', (dims[0], A['S'], A['S']), [w, A['frm'][m], A['to'][m]],
                              np.ones(int(m.sum())), 250, args.sweeps, args.repeats, args.numpy_budget_s))
    import torch
    line = {'device': torch.cuda.get_device_name(0), 'shapes': results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(line, f, indent=1)
    print(json.dumps(line))


if __name__ == '__main__':
    main()
