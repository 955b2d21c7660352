"""Conditions on the INPUTS of tests/test_gpu_fst4_tag.py, judged by the references alone (no GPU): the cases of
tests/fst4_tag_cases.py are drawn so that a subtly wrong K3 could not pass them.

Every signed case: the float32 oracle sits within tol / 10 of the float64 oracle in assert_float_path's metric |d| / (1 + |ref64|)
(fo.precision(np.float64) on widened inputs); every valid position has a non-zero score row; at most 10 % of the valid positions
are near-tied (top two clamped float64 scores within 2 tol (1 + |top|)) -- a cap: a case over it was redrawn.
Every signed FST 4-D case: at least 20 % of the non-zero terms A a b are negative, and the clip after the sum (mutant a) fails
assert_float_path.  Every case: alpha_{i+1} for alpha_i (b), beta one row off (c) and W4 / W left out (d) fail the case's
comparator.  Every exact case: no order of any of its sums needs more than 24 mantissa bits, so float32 == float64.
Planted ties: the two columns are bit-equal everywhere, and a last-index decode differs at at least half the valid positions.
"""
import numpy as np
import pytest

import fst4_tag_cases as fc


@pytest.mark.parametrize('c', fc.ALL_CASES, ids=fc.case_id)
def test_case_meets_its_conditions(c):
    assert fc.unmet(c) == [], (fc.case_id(c), c.edge)


def test_exemptions_are_the_structural_ones():
    """a mutant may be excused only where the case cannot tell it BY CONSTRUCTION, and each such pair is listed"""
    ids = {fc.case_id(c): c for c in fc.ALL_CASES}
    assert len(fc.EXEMPT) <= 8
    for cid, mu in fc.EXEMPT:
        c = ids[cid]
        assert (c.S <= 4 or c.L == 1) and mu in ('b', 'c') or (c.S == 1 and mu == 'a'), (cid, mu)
    assert set(fc.SEED_BUMP) <= set(ids)


def test_grid_covers_the_launcher_edges():
    """the restated launcher quantities (fc.k3_geometry, fc.k3_lds_bytes) take every value the shape list is there for"""
    for layout in ('fst4', 'ind1'):
        cs = [c for c in fc.CASES if c.layout == layout]
        geo = {fc.k3_geometry(c.S) for c in cs}
        assert {g.NCH for g in geo} == ({1, 2, 4} if layout == 'fst4' else {1})
        assert {1, 2, 3, 5, 16, 17, 32, 33} <= {g.CPR for g in geo}
        assert {0, 1, 4, 13, 31} <= {g.idle for g in geo}
        for kind in ('signed', 'exact'):
            assert {(c.semiring, c.prio) for c in cs if c.kind == kind} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert {c.C for c in cs if c.S == 5} >= {2, 3, 4, 5, 64, 65, 129, 256} | ({257, 300} if layout == 'fst4' else set())
        assert {c.C for c in cs if c.S == 71} >= {2, 3, 4, 5, 64, 65, 129, 256}
        assert {(c.B, c.L) for c in cs if c.S == 5 and c.C == 3} >= {(1, 1), (2, 9), (3, 9), (4, 9), (1100, 3)}
        assert any(not any(c.lengths) for c in cs)
        assert all({0, 1, c.L} <= set(c.lengths) for c in cs if c.B == 4 and any(c.lengths))
        assert all(c.B * c.L <= 40 or c.B == 1100 for c in cs)
    # the two LDS thresholds of independent=1, from the restated sum
    a, b = fc.largest_S_within(fc.LDS_ATTRIBUTE, 3), fc.largest_S_within(fc.LDS_LIMIT, 3)
    assert (a, b) == (108, 200)
    assert fc.k3_lds_bytes(a, 3, True) <= fc.LDS_ATTRIBUTE < fc.k3_lds_bytes(a + 1, 3, True)
    assert fc.k3_lds_bytes(b, 3, True) <= fc.LDS_LIMIT < fc.k3_lds_bytes(b + 1, 3, True)
    S_ind1 = {c.S for c in fc.CASES if c.layout == 'ind1'}
    assert {a, a + 1, b} <= S_ind1 and fc.refused_ind1_S() == b + 1 and b + 1 not in S_ind1
    assert {c.mask for c in fc.CASES if c.layout == 'ind1' and c.kind == 'signed'} == {False, True}
    # the planted ties
    assert {c.tie for c in fc.TIE_CASES if c.layout == 'fst4'} == set(fc.TIE_PAIRS) | {'threshold'}
    assert {c.tie for c in fc.TIE_CASES if c.layout == 'ind1'} == set(fc.TIE_PAIRS[:-1]) | {'threshold'}
    assert all(c.kind == 'exact' for c in fc.TIE_CASES)


def test_threshold_tie_is_decided_by_the_lower_index():
    for c in fc.TIE_CASES:
        if c.tie != 'threshold':
            continue
        r = fc.reference(c)
        at = fc.tied_threshold_positions(r)
        assert at.any()
        assert (r.want[at] < c.C - 1).all() and (r.want[at] != fc.o_idx(c)).all()
        assert (fc.decode_last_index(r.ref32, c)[at] == fc.o_idx(c)).all()


def test_band_rule_accepts_the_oracle_and_refuses_a_shifted_decode():
    """tags_allowed, the GPU module's rule on signed cases: the float32 oracle's own decode passes, the last-index decode of a
    zero row (every column tied) passes too, a decode shifted by one column does not"""
    c = next(c for c in fc.CASES if c.kind == 'signed' and c.layout == 'ind1' and c.S == 17)
    r = fc.reference(c)
    every = np.ones_like(r.mask)
    assert fc.tags_allowed(c, r, np.array(r.want), every)
    wrong = np.where(np.array(r.want64) == 0, 1, 0)
    assert not fc.tags_allowed(c, r, wrong, every)
