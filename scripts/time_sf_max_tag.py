#!/usr/bin/env python3
"""What the per-call token blocks of the max-semiring vector-input tagger cost (farnn_decomp_sf_max_create).

256 x 64 ragged batches, S = 104, farnn 0, at R = 50 and R = 250.  Per shape, three figures:
  farnn_tag_vectors   on the max handle: token_blocks_kernel + the dense chain, score and decode kernels;
  farnn_tag           on a max-semiring id handle whose table rows ARE the same vectors (Vgen = v as [B L][R], identity ids): its
                      blocks exist already, so the difference is what building them per call costs;
  create-time         materialise_blocks_kernel's cost for that same table, the one-thread-per-entry baseline of the new kernel:
                      farnn_decomp_ifst_create's wall time in the max semiring minus the sum semiring's (the same uploads, no
                      blocks), median of three each.
A call is timed on its own: one pair of events around it, the stream drained before the next; 10 warm-up calls, then the median
and the inter-quartile range of 40.  token_blocks_kernel by the library's own per-kernel events in a pass of its own, and beside
it the achieved fraction of the packed-FMA rate profiles/r06_pk_rate.txt measured (v_pk_fma_f32, 4 wavefronts per SIMD: 4.76
cycles per instruction, that is 128 / 4.76 FMAs per cycle and SIMD) for the 2 ntok S^2 R flops.

Prints one JSON line and writes profiles/sf_max_tag_timing.json.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from re2nn_seq_amd import _lib, synth  # noqa: E402

B, L, S, V, C = 256, 64, 104, 11000, 73
CALLS, WARMUP = 40, 10
PK_FMA_PER_CYCLE_PER_SIMD = 128 / 4.76
CLOCK_HZ = 2.4e9             # the MI355X's peak engine clock (the rate is an upper bound: the clock under load is lower)


def timed(fn, stream):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(CALLS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    q1, q2, q3 = np.percentile(out, [25, 50, 75])
    return {'median_us': float(q2), 'iqr_us': float(q3 - q1), 'calls': CALLS, 'warmup': WARMUP}


def kernel_us(h, fn, which):
    h.set_profiling(1)
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    ms, n = h.kernel_time(which)
    h.set_profiling(0)
    return {'mean_us': ms * 1e3 / max(n, 1), 'launches': int(n)}


def create_ms(make):
    out = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = make()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        h.close()
    return float(np.median(out))


def one(R, peak_flops):
    dev = torch.device('cuda', 0)
    _, q, gates, tr = synth.snips_sized_model(R, 0, False, S=S, V=V, C=C)
    kw = dict(farnn=0, gates=gates, sigmoid_exponent=5, nl='tanh', threshold=0.5, o_idx=0, device=0)
    w = (q['S1'], q['S2'], q['W'], q['Cout'], q['h0'], q['hT'])
    x, lengths = synth.random_batch(V, B, L, np.random.RandomState(3), min_len=5)
    v = np.ascontiguousarray(q['Vgen'][x])
    table = v.reshape(B * L, R)                            # the same vectors as an id handle's word table
    ids = np.arange(B * L, dtype=np.int64).reshape(B, L)
    make_id = lambda semiring: _lib.create_decomp_ifst(table, *w, semiring=semiring, **kw)   # noqa: E731
    idh = make_id('max')
    sf = _lib.create_decomp_sf_max(*w, **kw)
    xd, ld, vd = torch.from_numpy(ids).to(dev), torch.from_numpy(lengths).to(dev), torch.from_numpy(v).to(dev)
    flat_a = torch.empty((int(lengths.sum()),), dtype=torch.int64, device=dev)
    flat_b = torch.empty_like(flat_a)
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream
    by_ids = lambda: idh.tag(xd.data_ptr(), ld.data_ptr(), B, L, _lib.MODE_LOCAL, None, flat_a.data_ptr(), None, s)   # noqa: E731
    by_vec = lambda: sf.tag_vectors(vd.data_ptr(), ld.data_ptr(), B, L, _lib.MODE_LOCAL, None, flat_b.data_ptr(), None, s)   # noqa: E731
    by_ids(); by_vec()
    torch.cuda.synchronize()
    ntok = int(lengths.sum())
    r = {'R': R, 'farnn': 0, 'S': S, 'B': B, 'L': L, 'valid_tokens': ntok, 'flat_tags_equal_id_path': bool(torch.equal(flat_a, flat_b)),
         'blocks_kernel_name': sf.kernel_name(_lib.KERN_TABLE), 'recurrence': sf.kernel_name(_lib.KERN_CHAIN),
         'farnn_tag_vectors': timed(by_vec, stream), 'farnn_tag': timed(by_ids, stream),
         'token_blocks_kernel': kernel_us(sf, by_vec, _lib.KERN_TABLE),
         'recurrence_launch_vectors': kernel_us(sf, by_vec, _lib.KERN_CHAIN), 'recurrence_launch_ids': kernel_us(idh, by_ids, _lib.KERN_CHAIN)}
    r['blocks_cost_us'] = r['farnn_tag_vectors']['median_us'] - r['farnn_tag']['median_us']
    flops = 2.0 * ntok * S * S * R
    r['token_blocks_flops'] = flops
    r['token_blocks_fraction_of_pk_fma_rate'] = flops / (r['token_blocks_kernel']['mean_us'] * 1e-6) / peak_flops
    idh.close(); sf.close()
    c_max, c_sum = create_ms(lambda: make_id('max')), create_ms(lambda: make_id('sum'))
    r['materialise_blocks_create'] = {'create_max_ms': c_max, 'create_sum_ms': c_sum, 'difference_ms': c_max - c_sum,
                                      'table_rows': B * L, 'note': 'all B L rows, pad positions included'}
    return r


def main():
    assert torch.cuda.is_available(), 'needs an MI355X'
    prop = torch.cuda.get_device_properties(0)
    clock_hz = CLOCK_HZ
    peak = PK_FMA_PER_CYCLE_PER_SIMD * 4 * prop.multi_processor_count * clock_hz * 2
    out = {'device': torch.cuda.get_device_name(0), 'compute_units': prop.multi_processor_count, 'clock_hz_assumed': clock_hz,
           'pk_fma_rate_flops': peak, 'shapes': [one(50, peak), one(250, peak)]}
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'sf_max_tag_timing.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == '__main__':
    main()
