"""The tagging dispatch table, pinned: for every configuration of tests/golden/make_golden_dispatch.py (one per branch of the
dispatcher in csrc/farnn_hip.hip) one farnn_tag call reports the same kernel names (before and after the call), the same launch
counts of the three timer slots, the same algorithmic byte counts and the same tags as tests/golden/dispatch_table.json, which
was recorded with the library as it stood before the dispatcher was split into plan + launch.  Strings and integers exactly;
the byte counts are doubles computed from integers and must be equal too.

Not covered (no small shape reaches them): the Viterbi history that does not fit 158 KiB of LDS without FARNN_VITERBI_BP=1
(L in the thousands); B > 1024 on the decomposed models; `chain kernel: LDS ring does not fit` and the other refusals
(tests/test_gpu_create_refusals.py and the parity tests hold their texts); FARNN_CV_STASH and the diagnostic switches of the
profiling build, which change a launch's parameters but not which kernel runs.
"""
import importlib.util
import json
import os

import pytest

from util import GOLDEN, NO_SWITCH, run_module_in_ab_build

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location('make_golden_dispatch', os.path.join(GOLDEN, 'make_golden_dispatch.py'))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, 'dispatch_table.json')) as _f:
    TABLE = json.load(_f)


def _check(cfg):
    want = TABLE[cfg['name']]
    got = gen.record(cfg)
    assert set(got) == set(want)
    for field in sorted(want):
        assert got[field] == want[field], (cfg['name'], field, got[field], want[field])


def test_every_configuration_is_recorded():
    assert sorted(TABLE) == sorted(c['name'] for c in gen.CONFIGS)
    assert all(c['branch'] == TABLE[c['name']]['branch'] for c in gen.CONFIGS)


@pytest.mark.skipif(not NO_SWITCH, reason='the table holds for the default dispatch: the suite was started under a FARNN_* switch')
@pytest.mark.parametrize('cfg', [c for c in gen.CONFIGS if not c['ab']], ids=lambda c: c['name'])
def test_dispatch_table(cfg):
    _check(cfg)


@pytest.mark.skipif(not NO_SWITCH, reason='the table holds for the default dispatch: the suite was started under a FARNN_* switch')
def test_dispatch_table_ab_only_forms():
    """the forms only the A/B build carries (FARNN_CV_ONE, FARNN_NODEST): checked there, in a child process"""
    from re2nn_seq_amd import _lib
    if _lib.ab_build():
        for cfg in gen.CONFIGS:
            if cfg['ab']:
                _check(cfg)
        return
    r = run_module_in_ab_build(os.path.abspath(__file__), k='ab_only_forms', timeout=300)
    if r is not None:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
