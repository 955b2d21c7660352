#!/usr/bin/env python3
"""Head and tail of the recurrence-only launch around its chain, for the full-length rows of ONE headline launch (profiling
build, FARNN_DBG=2048):

    FARNN_LIB=$PWD/re2nn-seq_amd/csrc/libfarnn_hip_probes.so FARNN_DBG=2048 python scripts/debug/chain_head_stamps.py

chain_regs_body leaves s_memtime at six points of a workgroup's life in slots 8 .. 13 of its g_wg_stamps row (FARNN_HD_STAMP):
entry, selection done, set-up barrier passed, ring primed = first step about to start, chain end, writer drained; the kernel's
wrapper leaves the workgroup's wall-clock start / end (100 MHz) and its shader cycles, which gives the clock that was running."""
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from re2nn_seq_amd import _lib  # noqa: E402

B, L = 256, 64
torch.cuda.set_device(0)
dev = torch.device('cuda', 0)
h, x, lengths, _ = bench.build_workload('ifst', B, L, 0, 50, False)
h.reserve(B, L)
xd, ld = torch.from_numpy(x).to(dev), torch.from_numpy(lengths).to(dev)
tags = torch.empty((B, L), dtype=torch.int32, device=dev)
for _ in range(20):
    h.tag(xd.data_ptr(), ld.data_ptr(), B, L, _lib.MODE_LOCAL, tags.data_ptr(), None, None, torch.cuda.current_stream(dev).cuda_stream)
torch.cuda.synchronize()
lib = _lib.load()
n = 2 * B
buf = np.zeros((n, 16), dtype=np.int64)
rc = lib.farnn_debug_wg_stamps(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(n))
assert rc == 0, rc
seq, ln, st, en, cyc = buf.T[:5]
hd = buf[:, 8:14]
t0 = st.min()
clk = cyc / np.maximum((en - st) * 10.0, 1)              # GHz: shader cycles per ns of the workgroup's own life
print('kernel: %s; %d workgroups, starts within %.2f us, last end +%.2f us (the launch as the workgroups see it)' % (
    h.kernel_name(_lib.KERN_CHAIN), n, (st.max() - t0) * 1e-2, (en.max() - t0) * 1e-2))
print('cycles from the workgroup\'s entry (s_memtime); full-length rows (len %d):' % L)
print('  seq dir | start us  end us | selection done | barrier passed | first step | chain end | writer drained | per step | tail | clock GHz')
full = [i for i in range(n) if ln[i] == L]
for i in sorted(full, key=lambda i: (seq[i], i & 1)):
    e = hd[i] - hd[i, 0]
    print('  %3d  %d  | %7.2f %7.2f | %14d | %14d | %10d | %9d | %14d | %8.1f | %4d | %.3f' % (
        seq[i], i & 1, (st[i] - t0) * 1e-2, (en[i] - t0) * 1e-2, e[1], e[2], e[3], e[4], e[5], (e[4] - e[3]) / float(L), e[5] - e[4], clk[i]))
e = hd[full] - hd[full, :1]
m = e.mean(0)
ck = float(np.median(clk[full]))
print('  mean: selection %.0f, barrier %.0f, first step %.0f (the head), chain %.0f (%.1f per step), tail %.0f cycles; clock median %.3f GHz'
      % (m[1], m[2], m[3], m[4] - m[3], (m[4] - m[3]) / L, m[5] - m[4], ck))
print('  at that clock: head %.2f us, chain %.2f us, tail %.2f us' % (m[3] / ck * 1e-3, (m[4] - m[3]) / ck * 1e-3, (m[5] - m[4]) / ck * 1e-3))
allw = hd - hd[:, :1]
nz = ln > 0
print('  every workgroup with a step (n = %d): selection done %.0f, barrier passed %.0f, first step %.0f cycles (means)' % (
    nz.sum(), allw[nz, 1].mean(), allw[nz, 2].mean(), allw[nz, 3].mean()))
