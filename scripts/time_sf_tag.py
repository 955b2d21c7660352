#!/usr/bin/env python3
"""What vector input costs: farnn_tag_vectors beside farnn_tag of the same weights, the same vectors given as rows of Vgen.

256 x 64 ragged batches at (R, farnn) = (50, 0) and (250, 2), S = 104 (bench.py's decomposed shape).  Per figure: the median
of 5 runs of 50 back-to-back calls (one pair of events around a run), with the runs' min and max; the token-table kernel and
the recurrence launch by the library's own per-kernel events (farnn_set_profiling) in a pass of their own.  The yardstick is
the id path of the same build, whose kernels the vector path launches unchanged; the difference is the table.

Prints one JSON line and writes profiles/sf_tag_timing.json.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from re2nn_seq_amd import _lib, synth  # noqa: E402

B, L, S, V, C = 256, 64, 104, 11000, 73
RUNS, CALLS, WARMUP = 5, 50, 10


def timed(fn, stream):
    for _ in range(WARMUP):
        fn()
    out = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(CALLS):
            fn()
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / CALLS)
    return {'median_us': float(np.median(out)), 'min_us': float(min(out)), 'max_us': float(max(out)), 'runs': RUNS, 'calls_per_run': CALLS}


def kernel_us(h, fn, which):
    h.set_profiling(1)
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    ms, n = h.kernel_time(which)
    h.set_profiling(0)
    return {'mean_us': ms * 1e3 / max(n, 1), 'launches': int(n)}


def one(R, farnn):
    dev = torch.device('cuda', 0)
    _, q, gates, tr = synth.snips_sized_model(R, farnn, False, S=S, V=V, C=C)
    kw = dict(farnn=farnn, gates=gates, sigmoid_exponent=5, nl='tanh', threshold=0.5, o_idx=0, device=0)
    idh = _lib.create_decomp_ifst(q['Vgen'], q['S1'], q['S2'], q['W'], q['Cout'], q['h0'], q['hT'], **kw)
    sf = _lib.create_decomp_sf(q['S1'], q['S2'], q['W'], q['Cout'], q['h0'], q['hT'], **kw)
    x, lengths = synth.random_batch(V, B, L, np.random.RandomState(3), min_len=5)
    xd, ld = torch.from_numpy(x).to(dev), torch.from_numpy(lengths).to(dev)
    vd = torch.from_numpy(q['Vgen'][x]).to(dev).contiguous()
    flat_a = torch.empty((int(lengths.sum()),), dtype=torch.int64, device=dev)
    flat_b = torch.empty_like(flat_a)
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream
    ids = lambda: idh.tag(xd.data_ptr(), ld.data_ptr(), B, L, _lib.MODE_LOCAL, None, flat_a.data_ptr(), None, s)   # noqa: E731
    vec = lambda: sf.tag_vectors(vd.data_ptr(), ld.data_ptr(), B, L, _lib.MODE_LOCAL, None, flat_b.data_ptr(), None, s)   # noqa: E731
    ids(); vec()
    torch.cuda.synchronize()
    same = bool(torch.equal(flat_a, flat_b))
    r = {'R': R, 'farnn': farnn, 'S': S, 'B': B, 'L': L, 'valid_tokens': int(lengths.sum()), 'flat_tags_equal_id_path': same,
         'recurrence': sf.kernel_name(_lib.KERN_CHAIN),
         'farnn_tag': timed(ids, stream), 'farnn_tag_vectors': timed(vec, stream),
         'token_table_kernel': kernel_us(sf, vec, _lib.KERN_TABLE), 'recurrence_launch_vectors': kernel_us(sf, vec, _lib.KERN_CHAIN),
         'recurrence_launch_ids': kernel_us(idh, ids, _lib.KERN_CHAIN)}
    r['table_cost_us'] = r['farnn_tag_vectors']['median_us'] - r['farnn_tag']['median_us']
    r['table_exceeds_recurrence'] = r['token_table_kernel']['mean_us'] > r['recurrence_launch_vectors']['mean_us']
    idh.close(); sf.close()
    return r


def main():
    assert torch.cuda.is_available(), 'needs an MI355X'
    out = {'device': torch.cuda.get_device_name(0), 'shapes': [one(50, 0), one(250, 2)]}
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'sf_tag_timing.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == '__main__':
    main()
