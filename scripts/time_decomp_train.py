"""Timing of the decomposed i-FST training step (farnn_decomp_ifst_train_step) in both semirings at the
same shape: bench.py's `train` workload (SNIPS-sized V = 11000, S = 104, K = 73) with rank 250, farnn 2 and the CRF loss,
batch 256 x seqlen 64.  Prints one JSON line with, per semiring,

  lib_us_per_step     HIP-event time of the library step (farnn_train_time)
  step_us_per_step    the whole step as a training loop runs it: zero_grad, word table, the step, backward, Adam
  max_over_sum        the ratio of the library times

    python scripts/time_decomp_train.py [--steps 20] [--warmup 3] [--states 104] [--rank 250] [--farnn 2] [--crf 1]

--teacher kd|pr times, in one job and `--repeats` times each in turn, the plain sum step on the ragged batch, the plain sum
step on a full-length batch (the teacher's chains run B L steps instead of sum(len): that is its yardstick) and the teacher
step (farnn_decomp_ifst_teacher_train_step) on the ragged batch, and prints their medians and spreads, the ratios and the
hash of the sources the library was built from.

Each GPU step of a job script runs it under its own time limit (timeout -k 10 ...)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(a, semiring, teacher=None, full=False):
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
    if full:
        lengths[:] = L
    labels = brng.randint(0, K - (2 if a.crf else 0), size=(B, L)).astype(np.int64)
    xd, ld, lab = torch.from_numpy(x).to(dev), torch.from_numpy(lengths).to(dev), torch.from_numpy(labels).to(dev)
    tc = _lib.TrainContext(V, S, R, K, nl='tanh', threshold=0.5, o_idx=0, use_crf=a.crf, farnn=a.farnn, sigmoid_exponent=5.0,
                           semiring=semiring)
    ntok = int(lengths.sum())
    opt = torch.optim.Adam(list(p.values()), lr=1e-4)
    tch = None
    if teacher:
        re = (brng.rand(B, L, K) * 0.1).astype(np.float32)
        re[brng.rand(B, L, K) < 0.15] = 0.95
        re[..., K - (3 if a.crf else 1):] = 0.0
        tch = (torch.from_numpy(re).to(dev), teacher, 2.0, 0.5)

    def one():
        opt.zero_grad(set_to_none=True)
        loss, _ = decomp_ifst_train_step(tc, p['Vgen'], p['S1'], p['S2'], p['W'], p['C'], p['h0'], p['hT'], None, xd, ld, lab,
                                         crf_trans=p.get('trans'), gates=tuple(p[n] for n in gate_names), valid_tokens=ntok, teacher=tch)
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


def source_hash():
    import hashlib
    h = hashlib.sha256()
    src = os.path.join(ROOT, 're2nn-seq_amd', 'csrc')
    for fn in sorted(os.listdir(src)):
        if fn.endswith(('.hip', '.h')):
            with open(os.path.join(src, fn), 'rb') as f:
                h.update(fn.encode() + b'\0' + f.read())
    return h.hexdigest()[:16]


def teacher_timing(a):
    legs = {'plain_ragged': dict(), 'plain_full_length': dict(full=True), 'teacher_ragged': dict(teacher=a.teacher)}
    times = {k: [] for k in legs}
    for _ in range(a.repeats):                       # in turn, so that drift of the machine falls on all three alike
        for k, kw in legs.items():
            r, ntok, shape = run(a, 'sum', **kw)
            times[k].append(r['lib_us_per_step'])
    V, S, R, K, B, L = shape
    med = {k: float(np.median(v)) for k, v in times.items()}
    out = dict(workload='decomp_train_teacher', teacher=a.teacher, V=V, S=S, R=R, K=K, B=B, L=L, farnn=a.farnn, crf=bool(a.crf),
               steps=a.steps, repeats=a.repeats, source_hash=source_hash(), lib=os.environ.get('FARNN_LIB', 'default'),
               lib_us_per_step={k: dict(median=med[k], min=min(v), max=max(v), runs=v) for k, v in times.items()},
               teacher_over_plain_ragged=round(med['teacher_ragged'] / med['plain_ragged'], 3),
               teacher_over_plain_full_length=round(med['teacher_ragged'] / med['plain_full_length'], 3))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--states', type=int, default=104)
    ap.add_argument('--rank', type=int, default=250)
    ap.add_argument('--farnn', type=int, default=2)
    ap.add_argument('--crf', type=int, default=1)
    ap.add_argument('--teacher', choices=('kd', 'pr'), default=None)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    if a.teacher:
        return teacher_timing(a)
    out = {}
    for semiring in ('sum', 'max'):
        out[semiring], ntok, shape = run(a, semiring)
    V, S, R, K, B, L = shape
    print(json.dumps(dict(workload='decomp_train', V=V, S=S, R=R, K=K, B=B, L=L, farnn=a.farnn, crf=bool(a.crf),
                          valid_tokens=ntok, steps=a.steps, sum=out['sum'], max=out['max'],
                          max_over_sum=round(out['max']['lib_us_per_step'] / out['sum']['lib_us_per_step'], 2))))


if __name__ == '__main__':
    main()
