"""Conditions on the INPUTS of tests/test_gpu_decomp0_tag.py, judged by the references alone (no GPU): the cases of
tests/decomp0_tag_cases.py are drawn so that a subtly wrong decomp0_score_kernel could not pass them.

Every case with a valid position: the gap rule holds (decomp0_train_ref.check_gap; on the max semiring its decode half on the
oracle pair) with NO position left out of the tag comparison, and the float32 and float64 decodes are equal; the float32
reference sits within tol / 10 of float64 in assert_float_path's metric; every valid position has a non-zero score row; on the
sum semiring fo.decomp_fst_scores in float64 sits within 1e-9 (1 + |.|) of decomp0_train_ref.forward in float64; score_step
without a mutant EQUALS the float32 reference; every applicable mutant fails the comparator.  Tie cases: the two columns are
bit-equal in both references, the pair wins and a last-index decode differs at half or more of the valid positions.
A draw that missed was redrawn (tests/golden/decomp0_tag_seeds.json), never excused.
"""
import numpy as np
import pytest

import decomp0_tag_cases as dc


@pytest.mark.parametrize('c', dc.ALL_CASES, ids=dc.case_id)
def test_case_meets_its_conditions(c):
    assert dc.unmet(c) == [], (dc.case_id(c), c.edge)


def test_exemptions_are_the_structural_ones():
    """a mutant may be excused only where the case cannot tell it BY CONSTRUCTION, and each such pair is listed with its reason"""
    ids = {dc.case_id(c): c for c in dc.ALL_CASES}
    assert len(dc.EXEMPT) <= 6
    for cid, mu, reason in dc._SEEDS['exempt']:
        assert dc.exemption_allowed(ids[cid], mu) and reason, (cid, mu)
    assert set(dc.SEED_BUMP) <= set(ids)
    # (e) is no error where both ranks are multiples of 4: it is not applied there, and is applied everywhere else
    for c in dc.ALL_CASES:
        assert dc.applicable(c, 'e') == (c.R % 4 != 0 or c.RW % 4 != 0)
    assert all(dc.applicable(c, mu) for c in dc.ALL_CASES for mu in 'abcdf')


def test_grid_covers_the_kernel_edges():
    """the restated launcher quantities (dc.d0_geometry) take every value the shape list is there for"""
    cs = dc.CASES
    assert {c.S for c in cs} >= {1, 3, 4, 5, 64, 65, 72, 73, 104, 128, 129}
    assert {c.R for c in cs if c.RW == 3} >= {1, 3, 4, 5, 126, 127, 128, 129, 250}
    assert {c.RW for c in cs if c.R == 5} >= {1, 3, 4, 5, 67}
    assert {c.R + c.RW for c in cs} >= {128, 129, 257}
    assert {c.K for c in cs if not c.crf} >= {2, 3, 4, 5, 63, 64, 65, 128, 129, 130, dc.K_MAX}
    assert {c.K for c in cs if c.crf} >= {4, 5, 64, 65, 128, 129, 130}
    assert {c.L for c in cs} >= {1, 7, 8, 9, 16, 17} and {c.B for c in cs} >= {1, 4, 9}
    geo = [dc.d0_geometry(c.S, c.R, c.RW, c.K, c.L) for c in cs]
    assert {g.col_passes for g in geo} >= {1, 2, 3} and {g.label_passes for g in geo} == {1, 2}
    assert {g.decode_passes for g in geo} == {1, 2, 3, 4} and {g.Kc for g in geo} == {64, 128, 192, 256}
    assert {g.wgs for g in geo} == {1, 2, 3}
    assert any(g.SP != c.S for g, c in zip(geo, cs)) and any(g.Rp != c.R for g, c in zip(geo, cs)) and any(g.RWp != c.RW for g, c in zip(geo, cs))
    for c in cs:
        if c.B >= 4 and any(c.lengths):                      # L, 1, 0 and 1..3 live positions in a last workgroup
            assert {c.L, 1, 0} <= set(c.lengths), dc.case_id(c)
            assert any(1 <= n - (n - 1) // 8 * 8 <= 3 for n in c.lengths if n > 0), dc.case_id(c)
    assert any(not any(c.lengths) for c in cs)
    # an idle token half below a workgroup that exists in full: nlive < ntok < 8
    assert any(0 < n % 8 <= 3 and n < c.L and 4 < min(8, c.L - n // 8 * 8) < 8 for c in cs for n in c.lengths)
    assert {(c.nl, c.farnn) for c in cs if c.semiring == dc.SUM} >= {(n, f) for n in ('none', 'relu', 'tanh', 'relutanh') for f in (0, 1, 2)}
    assert {c.farnn for c in cs if c.semiring == dc.MAX} == {0, 1}
    assert {(c.prio, c.crf, c.mode) for c in cs} == {(p, q, m) for p in (0, 1) for q in (0, 1) for m in (dc.LOCAL, dc.FULL)}
    assert any(c.prio and c.K > 64 and not c.crf for c in cs)
    # the LDS steps, from the restated sum
    shapes = dc.lds_shapes()
    lds = [dc.d0_geometry(4, R, RW, 3, 9).lds for R, RW in shapes]
    assert lds[0] <= dc.LDS_ATTRIBUTE < lds[1] and lds[2] + dc.D0_STATIC_LDS <= dc.LDS_LIMIT < lds[3] + dc.D0_STATIC_LDS
    assert lds[0] == dc.LDS_ATTRIBUTE and lds[3] == dc.LDS_LIMIT and lds[1] - lds[0] == lds[3] - lds[2] == 128
    assert {(c.R, c.RW) for c in cs if c.S == 4 and c.K == 3} == set(shapes[:3])
    assert dc.refused_lds_shape() == (4,) + shapes[3] + (3,) and max(r for r, _ in shapes) <= dc.R_MAX
    assert {c.tie for c in dc.TIE_CASES} == set(dc.TIE_PAIRS) and all(not c.prio and not c.crf for c in dc.TIE_CASES)
    assert [(c.B, c.L) for c in dc.VARYING_CASES] == list(dc.VARYING_SHAPES) and dc.VARYING_CASES[0] == dc.VARYING_CASES[3]
    kinds = {(c.crf, c.farnn) for c in dc.TRAIN_CASES}
    assert kinds >= {(0, 0), (0, 2), (1, 0)} and any(c.R % 4 and c.K > 64 for c in dc.TRAIN_CASES)


def test_one_model_serves_the_varying_shapes():
    refs = [dc.reference(c) for c in dc.VARYING_CASES[:3]]
    for r in refs[1:]:
        assert all(np.array_equal(r.p[n], refs[0].p[n]) for n in refs[0].p) and np.array_equal(r.P, refs[0].P)


def test_the_comparator_accepts_the_reference_and_refuses_a_shifted_decode():
    c = dc.CASES[0]
    r = dc.reference(c)
    assert dc.mismatch(c, r, np.array(r.ref32), np.array(r.want64)) is None
    wrong = np.where(np.array(r.want64) == 0, 1, 0)
    assert dc.mismatch(c, r, np.array(r.ref32), wrong) is not None
