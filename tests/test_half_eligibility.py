"""csrc/half_exact.h: which f32 block entries the 16-bit image may hold -- exactly the values an IEEE f16 represents as a normal
number or a zero.  The predicate is bit arithmetic shared by the host and the device-side reduction of the create
(csrc/layout.hip.h: half_eligible_kernel); here a small stand-alone program holds it, and the f16 pattern it produces, to a table of
values.  No GPU."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 're2nn-seq_amd', 'csrc')

# (value as a C expression, eligible)
TABLE = [('0.0f', True), ('-0.0f', True), ('1.0f', True), ('-1.0f', True), ('0.125f', True), ('3.875f', True),
         ('6.103515625e-05f', True),             # 2**-14: the smallest normal f16
         ('-6.103515625e-05f', True),
         ('3.0517578125e-05f', False),           # 2**-15: an f16 subnormal
         ('9.5367431640625e-07f', False),        # 2**-20
         ('2048.0f', True), ('-2048.0f', True), ('2049.0f', False), ('65504.0f', True), ('65520.0f', False), ('65536.0f', False),
         ('1.0f / 3.0f', False), ('1.0f + 1.0f / 2048.0f', False), ('1.0f + 1.0f / 1024.0f', True),
         ('1e-45f', False),                      # an f32 subnormal
         ('INFINITY', False), ('-INFINITY', False), ('NAN', False)]

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')       # the compiler the library itself is built with (csrc/build.py)


def _compile(src, exe):
    """host-only C++: the header needs no HIP (-x c++ keeps hipcc from treating the file as device code)"""
    assert os.path.exists(HIPCC), 'the project does not build without {}: nothing to hold the predicate with'.format(HIPCC)
    subprocess.run([HIPCC, '-x', 'c++', '-std=c++17', '-O1', '-I', CSRC, str(src), '-o', str(exe)], check=True)


MAIN = r'''
#include <math.h>
#include <stdio.h>
#include "half_exact.h"
int main(void) {
    const float v[] = {%s};
    for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); i++)
        printf("%%d %%u %%u\n", farnn::half_exact(v[i]) ? 1 : 0, (unsigned)farnn::half_bits_exact(v[i]), (unsigned)farnn::f32_bits(v[i]));
    return 0;
}
'''


def test_half_exact_table(tmp_path):
    src = tmp_path / 'half_table.cpp'
    src.write_text(MAIN % ', '.join(e for e, _ in TABLE))
    exe = tmp_path / 'half_table'
    _compile(src, exe)
    rows = [ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()]
    assert len(rows) == len(TABLE)
    for (expr, want), (ok, hbits, fbits) in zip(TABLE, rows):
        assert bool(int(ok)) == want, expr
        x = np.array([int(fbits)], np.uint32).view(np.float32)[0]
        with np.errstate(over='ignore'):
            back = np.float32(np.float16(x))
        # the predicate IS "(float)(half)x == x and not an f16 subnormal", and the pattern is numpy's f16 of the value
        rt = bool(back == x) and (x == 0 or abs(float(x)) >= 2.0 ** -14) and bool(np.isfinite(x))
        assert rt == want, expr
        if want:
            assert int(hbits) == int(np.array([x], np.float32).astype(np.float16).view(np.uint16)[0]), expr


def test_half_exact_every_f16_pattern_round_trips(tmp_path):
    """all 65 536 f16 patterns widened to f32: eligible iff a zero or a finite normal, and the pattern comes back"""
    src = tmp_path / 'half_all.cpp'
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "half_exact.h"
int main(void) {
    unsigned u;
    while (scanf("%u", &u) == 1) { float x; memcpy(&x, &u, 4); printf("%d %u\n", farnn::half_exact(x) ? 1 : 0, (unsigned)farnn::half_bits_exact(x)); }
    return 0;
}
''')
    exe = tmp_path / 'half_all'
    _compile(src, exe)
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    x = h.view(np.float16).astype(np.float32)
    out = subprocess.run([str(exe)], input='\n'.join(str(int(b)) for b in x.view(np.uint32)), check=True, capture_output=True, text=True).stdout
    got = np.array([ln.split() for ln in out.strip().splitlines()], dtype=np.int64)
    e = (h >> 10) & 31
    want = ((e >= 1) & (e <= 30)) | ((h & 0x7fff) == 0)
    assert np.array_equal(got[:, 0].astype(bool), want)
    assert np.array_equal(got[want, 1], h[want].astype(np.int64))
