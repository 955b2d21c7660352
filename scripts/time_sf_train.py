#!/usr/bin/env python3
"""Step time of farnn_decomp_sf_train_step (FARNN_S_SF's training step) beside the id step on the same
weights, at 256 x 64 ragged: (R 50, farnn 0, CE1) and (R 250, farnn 2, CRF).  Prints ONE JSON line.

    python scripts/time_sf_train.py [--runs 40] [--warmup 10] [--out profiles/sf_train_timing.json]

Method: every figure is the median over `runs` single steps after `warmup` untimed ones, each step timed by the library's own
HIP event pair around its launches (farnn_train_set_profiling / farnn_train_time), with min, max and the inter-quartile range
beside it.  The id step (farnn_decomp_ifst_train_step, unchanged code) runs on a word table whose rows are the batch's vectors
and the ids b L + t.  The two new kernels' own times come from torch.profiler's device-kernel records of the same steps (null
when the profiler records no device kernels).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from re2nn_seq_amd import _lib  # noqa: E402

B, L, S, LABELS = 256, 64, 104, 72
CONFIGS = (dict(name='R50-farnn0-CE1', R=50, farnn=0, crf=False), dict(name='R250-farnn2-CRF', R=250, farnn=2, crf=True))
GATES = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    q1, q3 = np.percentile(a, [25, 75])
    return dict(median_ms=float(np.median(a)), min_ms=float(a[0]), max_ms=float(a[-1]), iqr_ms=float(q3 - q1), runs=len(a))


def timed(tc, step, runs, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    tc.set_profiling(1)
    tc.time()
    ms = []
    for _ in range(runs):
        step()
        t, n = tc.time()
        assert n == 1
        ms.append(t)
    tc.set_profiling(0)
    return stats(ms)


def kernel_times(step, runs):
    """{kernel name prefix: stats} of sf_gate_kernel / sf_dv_kernel over `runs` steps, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(runs):
                step()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            for k in ('sf_gate_kernel', 'sf_dv_kernel'):
                dur = getattr(ev, 'device_time', None) or getattr(ev, 'cuda_time', 0)
                if k in ev.name and dur:
                    out.setdefault(k, []).append(dur / 1000.0)
        return {k: stats(v) for k, v in out.items()} or None
    except Exception as e:      # the profiler is optional: the step times above do not depend on it
        return {'error': repr(e)}


def one(cfg, runs, warmup, dev):
    R, farnn, crf = cfg['R'], cfg['farnn'], cfg['crf']
    K = LABELS + 1 + (2 if crf else 0)
    rng = np.random.RandomState(5)
    f = lambda *shape, sc=0.3: torch.from_numpy((rng.randn(*shape) * sc).astype(np.float32)).to(dev)   # noqa: E731
    Cm = np.zeros((K, S), np.float32)
    Cm[rng.randint(0, K, size=S), np.arange(S)] = (rng.rand(S) < 0.8)
    w = {'S1': f(S, R, sc=1.0 / np.sqrt(S)), 'S2': f(S, R, sc=1.0 / np.sqrt(S)),
         'W': torch.from_numpy(((rng.rand(S, S) < 1.0 / S) * 0.5).astype(np.float32)).to(dev),
         'C': torch.from_numpy(Cm + (rng.rand(K, S) * 0.02).astype(np.float32)).to(dev), 'h0': f(S, sc=0.5), 'hT': f(S, sc=0.5)}
    for g in range(farnn):
        w['Wss%d' % (g + 1)], w['Wrs%d' % (g + 1)], w['bs%d' % (g + 1)] = f(S, S, sc=0.3 / np.sqrt(S)), f(R, S, sc=0.3 / np.sqrt(R)), f(S, sc=0.2)
    if crf:
        tr = (rng.randn(K, K) * 0.1).astype(np.float32)
        tr[:, K - 2] = -10000.0
        tr[K - 1, :] = -10000.0
        w['crf_trans'] = torch.from_numpy(tr).to(dev)
    v = f(B, L, R, sc=0.8)
    lengths_h = rng.randint(1, L + 1, size=B).astype(np.int64)
    lengths_h[0] = L
    lengths = torch.from_numpy(lengths_h).to(dev)
    labels = torch.from_numpy(rng.randint(0, LABELS + 1, size=(B, L)).astype(np.int64)).to(dev)
    ids = torch.arange(B * L, device=dev).reshape(B, L)
    ntok = int(lengths_h.sum())
    out = {n: torch.empty_like(t) for n, t in w.items()}
    dv, dVgen = torch.empty_like(v), torch.empty((B * L, R), device=dev)
    loss, tags = torch.empty(1, device=dev), torch.empty((B, L), dtype=torch.int32, device=dev)
    outputs = {('dtrans' if n == 'crf_trans' else 'd' + n): t.data_ptr() for n, t in out.items()}
    outputs.update(loss=loss.data_ptr(), tags=tags.data_ptr())
    wp = {n: t.data_ptr() for n, t in w.items()}
    kw = dict(nl='tanh', threshold=0.5, o_idx=0, use_crf=crf, farnn=farnn, sigmoid_exponent=5.0)
    sf = _lib.SfTrainContext(S, R, K, **kw)
    idc = _lib.TrainContext(B * L, S, R, K, **kw)

    def sf_step():
        sf.step_vectors(wp, v.data_ptr(), lengths.data_ptr(), labels.data_ptr(), B, L, ntok, outputs, dv.data_ptr())

    def id_step():
        idc.step(dict(wp, Vgen=v.data_ptr()), ids.data_ptr(), lengths.data_ptr(), labels.data_ptr(), B, L, ntok,
                 dict(outputs, dVgen=dVgen.data_ptr()))
    r = dict(config=cfg['name'], B=B, L=L, S=S, R=R, K=K, valid_tokens=ntok, sf_step=timed(sf, sf_step, runs, warmup))
    sf_loss = float(loss)
    r['id_step'] = timed(idc, id_step, runs, warmup)
    r['loss_sf'], r['loss_id'] = sf_loss, float(loss)
    r['sf_over_id'] = r['sf_step']['median_ms'] / r['id_step']['median_ms']
    r['new_kernels'] = kernel_times(sf_step, 10)
    sf.close()
    idc.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=40)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda', 0)
    res = dict(device=torch.cuda.get_device_name(0), method='median of single steps, HIP event pair around each step',
               results=[one(c, a.runs, a.warmup, dev) for c in CONFIGS])
    line = json.dumps(res, sort_keys=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
