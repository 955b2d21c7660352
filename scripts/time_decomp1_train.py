"""Timing of the decomposed independent=1 training step (farnn_decomp_ind1_train_step) at the shape of
bench.py's `decomp1` workload: V = 11 000, S = 104, C = 73, rank 50, output rank 70, tanh, B = 256, L = 64 with ragged
lengths, rotating through four batches of the same lengths.  Prints one JSON line:

  lib_us_per_step     HIP-event time of the library step (farnn_decomp_ind1_train_time): median of the per-step times, with
  lib_us_min / _max   their spread
  stage_us            (--stages 1) torch.profiler's device time per kernel name over the timed steps, divided by the steps,
                      largest first, and `dominant` the first of them; a run of its own, after the event-timed steps

  result_sha          sha256 over the loss and every gradient of the last timed step (bytes): two builds whose plain step
                      shares every kernel must print the same one

    python scripts/time_decomp1_train.py [--steps 10] [--warmup 2] [--stages 1] [--use_crf 1] [--farnn 1|2] [--parent_lib 1]

--use_crf 1: farnn_decomp_ind1_crf_train_step with the same 73 labels (the score width becomes 75: START and STOP; the
transitions are the reference's initial ones plus seeded noise in (-0.5, 0.5) where they are not -10000).
--farnn 1 | 2: farnn_decomp_ind1_gated_train_step with seeded gates (Wss ~ N(0, 0.3^2 / S), Wrs ~ N(0, 0.3^2 / R), bs ~
N(0, 0.2^2), sigmoid_exponent 5: the sigmoids stay off saturation), drawn after everything the plain step draws.
--farnn 1 | 2 --train_mode max: farnn_decomp_ind1_gated_max_train_step on the same gates (train_step picks it on a max context).
--parent_lib 1: the library named by FARNN_LIB is a build of the commit before the gated max entry point (its binding is
dropped before the library is loaded); for the plain step in either semiring, the CRF step and the gated sum step.

The line carries no rate: none was measured.  Each GPU step of a job script runs it under its own time limit
(timeout -k 10 ...)."""
import argparse
import json
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--train_mode', choices=('sum', 'max'), default='sum')       # the semiring of the chains
    ap.add_argument('--stages', type=int, default=1)
    ap.add_argument('--use_crf', type=int, default=0)
    ap.add_argument('--farnn', type=int, choices=(0, 1, 2), default=0)
    ap.add_argument('--parent_lib', type=int, default=0)
    a = ap.parse_args()
    import torch
    from re2nn_seq_amd import _lib, synth
    if a.parent_lib:
        assert not (a.farnn and a.train_mode == 'max'), 'the parent build has no gated max step'
        _lib.SIGNATURES.pop('farnn_decomp_ind1_gated_max_train_step')
    from re2nn_seq_amd.farnn.train_step import decomp_ind1_train_step
    V, S, C, R, RO, B, L = 11000, 104, 73, 50, 70, 256, 64
    rng = np.random.RandomState(1234)
    p = synth.random_decomposed_params(V, S, C, R, 100, rng, contractive=True)
    f = lambda *shape, sc=0.2: (rng.randn(*shape) * sc).astype(np.float32)      # noqa: E731
    x0, lengths = synth.random_batch(V, B, L, rng)
    xs = [x0]
    for k in range(1, 4):                         # same lengths, tokens drawn afresh (bench.py batch_variants)
        r = np.random.RandomState(4321 + 7919 * k)
        xk, _ = synth.random_batch(V, B, L, r, min_len=L, full_length_rows=B)
        xk[np.arange(L)[None, :] >= lengths[:, None]] = V - 1
        xs.append(xk)
    labels = [rng.randint(0, C, size=(B, L)).astype(np.int64) for _ in xs]
    trans = None
    if a.use_crf:                                 # (drawn after everything the plain step draws: its inputs stay the same)
        C += 2
        trans = np.zeros((C, C), np.float32)
        trans[:, C - 2] = -10000.0
        trans[C - 1, :] = -10000.0
        trans += np.where(trans > -5000.0, np.random.RandomState(99).uniform(-0.5, 0.5, size=(C, C)), 0.0).astype(np.float32)
    ntok = int(lengths.sum())
    dev = torch.device('cuda', 0)
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev).requires_grad_(True)      # noqa: E731
    ws = [d(p['V_embed']), d(p['S1']), d(p['S2']), d(p['wildcard_mat']), d(f(C, RO, sc=0.5)), d(f(S, RO)), d(f(S, RO)),
          d(p['start_vector']), d(p['final_vector'])]
    xd = [torch.from_numpy(v).to(dev) for v in xs]
    ld = torch.from_numpy(lengths).to(dev)
    labd = [torch.from_numpy(v).to(dev) for v in labels]
    tc = _lib.Decomp1TrainContext(V, S, R, RO, C, nl='tanh', device=0, semiring=a.train_mode)
    td = None if trans is None else d(trans)
    gr = np.random.RandomState(77)
    gates = []
    for _ in range(a.farnn):
        gates += [d(gr.randn(S, S) * 0.3 / np.sqrt(S)), d(gr.randn(R, S) * 0.3 / np.sqrt(R)), d(gr.randn(S) * 0.2)]
    more = dict(gates=tuple(gates), sigmoid_exponent=5.0) if gates else {}

    def one(i):
        for t in ws + gates:
            t.grad = None
        if td is not None:
            td.grad = None
        loss, _ = decomp_ind1_train_step(tc, *ws, None, xd[i % 4], ld, labd[i % 4], valid_tokens=ntok, crf_trans=td, **more)
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
    for t in ws + ([td] if td is not None else []) + gates:
        sha.update(t.grad.cpu().numpy().tobytes())
    words = [int(len(np.unique(v[np.arange(L)[None, :] < lengths[:, None]]))) for v in xs]
    # the stamp of what was measured: sha256 over the library's sources (csrc/*.hip, csrc/*.h, include/farnn.h), names in order
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, 're2nn-seq_amd', 'csrc')
    for path in sorted(os.path.join(csrc, n) for n in os.listdir(csrc) if n.endswith(('.hip', '.h'))) + \
            [os.path.join(ROOT, 'include', 'farnn.h')]:
        with open(path, 'rb') as fh:
            h.update(os.path.basename(path).encode() + b'\0' + fh.read())
    tree = h.hexdigest()[:16]
    out = {'shape': {'V': V, 'S': S, 'C': C, 'R': R, 'RO': RO, 'B': B, 'L': L, 'nl': 'tanh'}, 'valid_tokens': ntok, 'train_mode': a.train_mode,
           'steps': a.steps, 'use_crf': a.use_crf, 'farnn': a.farnn, 'result_sha': sha.hexdigest()[:16], 'lib_us_per_step': float(np.median(per)), 'lib_us_min': float(min(per)),
           'lib_us_max': float(max(per)), 'distinct_words': words, 'loss': float(loss.detach()), 'tree': tree}
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
    print(json.dumps(out, sort_keys=True))


if __name__ == '__main__':
    main()
