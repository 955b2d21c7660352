"""Time the library's order-4 CP-ALS sweep (farnn_cp_run_n) and, beside it, the coordinate-list numpy sweep on the same machine.

    python scripts/time_cp4_als.py [--out profiles/cp4_als_timing.json] [--sweeps 8] [--repeats 5] [--numpy_sweeps 3]

Two shapes, each the nonzeros of a case of scripts/time_cp_als.py with a label drawn for every nonzero from a fixed seed: the
ATIS-sized automaton (V' = 819, C = 127, S = 71), R = 150; and synth.planted_rule_ifst() at its default (SNIPS) size
(V' = 3 621, C = 127, S = 104), R = 250.  Per shape: the milliseconds per sweep of un-profiled runs (wall clock around the call,
the factors' two bus crossings included; median and min .. max over the repeats, after a warm-up run) and the milliseconds per
sweep of each stage from HIP events (a profiled run waits after every stage, so the stages do not add up to the first figure).
The numpy sweep is the order-4 restatement on the coordinates (np.add.at in list order, float64, the machine's BLAS threads as
configured -- 16 where the figures in profiles/ were taken); the dense [V', C, S, S] tensor is never built.  Prints one JSON line
per shape and writes them all to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from re2nn_seq_amd import _lib, synth  # noqa: E402

N_LABELS = 127
LABEL_SEED = 4321


def squash(word):
    words, w = np.unique(word, return_inverse=True)
    return len(words), np.asarray(w).reshape(-1).astype(np.int32)


def numpy_sweep(dims, idx, val, normx2, f):
    """one order-4 sweep on the coordinates; returns the rec_error"""
    N = len(dims)
    for n in range(N):
        oth = [m for m in range(N) if m != n]
        H = f[oth[0]].T @ f[oth[0]]
        terms = val[:, None] * f[oth[0]][idx[oth[0]]]
        for m in oth[1:]:
            H = H * (f[m].T @ f[m])
            terms = terms * f[m][idx[m]]
        M = np.zeros((dims[n], H.shape[0]))
        np.add.at(M, idx[n], terms)
        f[n] = np.linalg.solve(H.T, M.T).T
    g = f[0].T @ f[0]
    for m in range(1, N):
        g = g * (f[m].T @ f[m])
    return float(np.sqrt(abs(normx2 + np.sum(g) - 2.0 * np.sum(M * f[N - 1])) / normx2))


def time_shape(name, dims, idx, val, R, sweeps, repeats, numpy_sweeps):
    rng = np.random.RandomState(0)
    init = [rng.random_sample((d, R)) for d in dims]
    ctx = _lib.CpContext.from_coo(dims, idx, val, R)
    normx2, nnz = ctx.norm2()
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
    out = {'shape': name, 'order': 4, 'dims': list(dims), 'nnz': int(nnz), 'rank': R, 'sweeps_per_run': sweeps, 'repeats': repeats,
           'ms_per_sweep': {'median': float(np.median(wall)), 'min': float(min(wall)), 'max': float(max(wall))},
           'stage_ms_per_sweep': {k: v / n for k, v in stage_ms.items()}, 'timed_sweeps': n, 'last_rec_error': errs[-1]}
    if numpy_sweeps > 0:
        f = [a.copy() for a in init]
        numpy_sweep(dims, idx, val, normx2, f)                      # warm-up sweep
        ts = []
        for _ in range(numpy_sweeps):
            t0 = time.perf_counter()
            numpy_sweep(dims, idx, val, normx2, f)
            ts.append((time.perf_counter() - t0) * 1e3)
        out['numpy_coo_ms_per_sweep'] = {'median': float(np.median(ts)), 'min': float(min(ts)), 'max': float(max(ts)),
                                         'threads': int(os.environ.get('OMP_NUM_THREADS', 0)) or None}
    return out


def with_labels(w, a, b, val):
    """a label for every nonzero from a fixed seed; coordinates that collide are merged (the library would add them)"""
    lab = np.random.RandomState(LABEL_SEED).randint(0, N_LABELS, size=len(w)).astype(np.int32)
    coords = np.unique(np.stack([w, lab, a, b], axis=1), axis=0).astype(np.int32)
    return [coords[:, k].copy() for k in range(4)], np.ones(len(coords)) if val is None else val


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cp4_als_timing.json'))
    p.add_argument('--sweeps', type=int, default=8)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--numpy_sweeps', type=int, default=3)
    args = p.parse_args()
    results = []
    T, _, _, _, _ = synth.random_ifst_tensors(950, 71, 128, np.random.RandomState(1234))
    w, a, b = np.nonzero(T)
    V, w = squash(w)
    idx, val = with_labels(w, a.astype(np.int32), b.astype(np.int32), None)
    results.append(time_shape('atis_sized V={} C={} S=71'.format(V, N_LABELS), (V, N_LABELS, 71, 71), idx, val, 150, args.sweeps,
                              args.repeats, args.numpy_sweeps))
    print(json.dumps(results[-1]), flush=True)
    A = synth.planted_rule_ifst()
    m = A['word'] >= 0
    V, w = squash(A['word'][m])
    idx, val = with_labels(w, A['frm'][m].astype(np.int32), A['to'][m].astype(np.int32), None)
    results.append(time_shape('planted_rule_ifst default (SNIPS size) C={}'.format(N_LABELS), (V, N_LABELS, A['S'], A['S']), idx, val,
                              250, args.sweeps, args.repeats, args.numpy_sweeps))
    print(json.dumps(results[-1]), flush=True)
    import torch
    line = {'device': torch.cuda.get_device_name(0), 'shapes': results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(line, f, indent=1)


if __name__ == '__main__':
    main()
