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

--teacher-max kd|pr does the same for the teacher step in the max semiring (farnn_decomp_ifst_teacher_max_train_step): the
plain sum and plain max steps on the ragged batch, the plain max step on a full-length batch, and the teacher-max step on the
ragged and on the full-length batch; every leg also reports a hash of the tags of its first step (fresh weights, fixed inputs).
--plain-only times the two plain ragged legs alone: with FARNN_LIB naming a library built from another commit (which may lack
the newer entry points) it is the other side of an A/B.  A job script alternates the two and keeps every printed line;
--merge FILE [FILE ...] reads such lines back and writes the medians and spreads per library as one JSON document.

Each GPU step of a job script runs it under its own time limit (timeout -k 10 ...)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def older_library_ok():
    """FARNN_LIB may name a library built from an earlier commit: the entry points it lacks are left unbound (its legs never
    call them)"""
    import ctypes
    import torch  # noqa: F401  (one HIP runtime per process: the library is loaded after torch)
    from re2nn_seq_amd import _lib
    if os.environ.get('FARNN_LIB'):
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib.SIGNATURES if not hasattr(lib, n)]:
            del _lib.SIGNATURES[name]


def run(a, semiring, teacher=None, full=False):
    import hashlib
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
                           semiring=semiring, **(dict(teacher_max=True) if teacher and semiring == 'max' else {}))
    ntok = int(lengths.sum())
    opt = torch.optim.Adam(list(p.values()), lr=1e-4)
    tch = None
    if teacher:
        re = (brng.rand(B, L, K) * 0.1).astype(np.float32)
        re[brng.rand(B, L, K) < 0.15] = 0.95
        re[..., K - (3 if a.crf else 1):] = 0.0
        tch = (torch.from_numpy(re).to(dev), teacher, 2.0, 0.5)

    first_tags = []

    def one():
        opt.zero_grad(set_to_none=True)
        loss, tags = decomp_ifst_train_step(tc, p['Vgen'], p['S1'], p['S2'], p['W'], p['C'], p['h0'], p['hT'], None, xd, ld, lab,
                                         crf_trans=p.get('trans'), gates=tuple(p[n] for n in gate_names), valid_tokens=ntok, teacher=tch)
        if not first_tags:
            first_tags.append(hashlib.sha256(tags.cpu().numpy().tobytes()).hexdigest()[:16])
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
                final_loss=float(loss.detach()), first_tags=first_tags[0]), ntok, (V, S, R, K, B, L)


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


MAX_LEGS = {'plain_sum_ragged': ('sum', dict()), 'plain_max_ragged': ('max', dict()),
            'plain_max_full_length': ('max', dict(full=True)), 'teacher_max_ragged': ('max', dict(teacher=True)),
            'teacher_max_full_length': ('max', dict(teacher=True, full=True))}


def teacher_max_timing(a):
    """one JSON line: every leg `--repeats` times in turn; --plain-only: the two plain ragged legs"""
    older_library_ok()
    legs = {k: v for k, v in MAX_LEGS.items() if not a.plain_only or k in ('plain_sum_ragged', 'plain_max_ragged')}
    times, tags, ntoks = {k: [] for k in legs}, {}, {}
    for _ in range(a.repeats):
        for k, (semiring, kw) in legs.items():
            kw = dict(kw, teacher=a.teacher_max) if kw.get('teacher') else kw
            r, ntok, shape = run(a, semiring, **kw)
            times[k].append(r['lib_us_per_step'])
            tags[k], ntoks[k] = r['first_tags'], ntok
    V, S, R, K, B, L = shape
    print(json.dumps(dict(workload='decomp_train_teacher_max', teacher=a.teacher_max, V=V, S=S, R=R, K=K, B=B, L=L, farnn=a.farnn,
                          crf=bool(a.crf), steps=a.steps, lib=os.environ.get('FARNN_LIB', 'default'),
                          source_hash=None if os.environ.get('FARNN_LIB') else source_hash(), valid_tokens=ntoks, positions=B * L, lib_us_per_step=times, first_tags=tags)))


def merge(files, other):
    """the lines a job kept, per library (`other` names the one FARNN_LIB pointed to): medians, spreads and the tag hashes"""
    rows = []
    for fn in files:
        with open(fn) as f:
            rows += [json.loads(line) for line in f if line.startswith('{')]
    libs = {}
    for r in rows:
        mine = r['lib'] == 'default'
        d = libs.setdefault('this' if mine else other, dict(source_hash=r['source_hash'] if mine else None, lib_us_per_step={}, first_tags={}))
        for k, v in r['lib_us_per_step'].items():
            d['lib_us_per_step'].setdefault(k, []).extend(v)
        for k, v in r['first_tags'].items():
            d['first_tags'].setdefault(k, set()).add(v)
    out = {k: rows[0][k] for k in ('workload', 'teacher', 'V', 'S', 'R', 'K', 'B', 'L', 'farnn', 'crf', 'steps', 'positions')}
    out['valid_tokens'] = max((r['valid_tokens'] for r in rows), key=len)
    out['libraries'] = {}
    for lib, d in libs.items():
        out['libraries'][lib] = dict(source_hash=d['source_hash'], first_tags={k: sorted(v) for k, v in d['first_tags'].items()},
                                     lib_us_per_step={k: dict(median=float(np.median(v)), min=min(v), max=max(v), runs=v)
                                                      for k, v in d['lib_us_per_step'].items()})
    print(json.dumps(out, indent=1, sort_keys=True))


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
    ap.add_argument('--teacher-max', choices=('kd', 'pr'), default=None)
    ap.add_argument('--plain-only', action='store_true')
    ap.add_argument('--merge', nargs='+', default=None)
    ap.add_argument('--other-label', default='other', help='--merge: the name of the library FARNN_LIB pointed to')
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.other_label)
    if a.teacher_max or a.plain_only:
        return teacher_max_timing(a)
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
