"""The tagging path of the two dense onehot layouts against the oracle, on the cases of tests/fst4_tag_cases.py: FARNN_S_O
(create_onehot_fst4) and FARNN_S_O_I (create_onehot_ind1, both mask_by_output values) through farnn_tag with device pointers --
the chain kernel on the label-summed tensor, then K3 (csrc/fst4_score.hip.h: fst4_score_kernel<NCH>) -- on SIGNED weights, where
the relu inside the 4-D sum and the relu of both recurrences bite, and at the sizes where launch_fst4_score changes what a lane
does (every case's id carries S and C; Case.edge names the launcher quantity).

Scores: exact cases EQUAL the float32 oracle; signed cases pass tests/util.py: assert_float_path at its default 1e-4 against the
float32 and float64 oracles (no per-shape bars).  Tags: the oracle's on exact cases (planted ties included: the first index
wins); on signed cases the float64 decode wherever the top two clamped scores are more than 2 tol (1 + |top|) apart, a column
inside that band elsewhere (tests/test_fst4_tag_cases_cpu.py caps such positions at 10 % of a case, from the references alone).
Every output buffer is pre-filled with a sentinel and has a guard row either side.

FST4_TAG_REPORT=<file>: every signed case appends its worst |got - ref64| / (1 + |ref64|) (a record, never a source for the bar).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import fst4_tag_cases as fc
from util import NO_SWITCH

pytestmark = pytest.mark.gpu

SENT = -7
GUARD = 8                                                  # guard elements either side of the flat tags
ERANGE = -34                                               # include/farnn.h
LDS_TEXT = 'independent=1 scoring needs S*S*4 bytes of LDS'


def _create(c, r):
    from re2nn_seq_amd import _lib
    kw = dict(P=r.P, semiring='max' if c.semiring else 'sum', threshold=fc.THRESHOLD, o_idx=fc.o_idx(c))
    if c.layout == 'fst4':
        return _lib.create_onehot_fst4(*r.model, **kw)
    return _lib.create_onehot_ind1(*r.model, mask_by_output=c.mask, **kw)


def _tag(h, c, x, lengths, mode, tags=True, flat=True, scores=True):
    """one farnn_tag into guarded, pre-filled buffers: (tags [B, L] int64, flat [N], scores [B, L, C]), None for what was not asked"""
    Bn, L = x.shape
    N = int(np.sum(lengths))
    xd, ld = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(lengths)).cuda()
    tg = torch.full((Bn + 2, L), SENT, dtype=torch.int32, device='cuda')
    fl = torch.full((N + 2 * GUARD,), SENT, dtype=torch.int64, device='cuda')
    sc = torch.full((Bn * L + 2, c.C), float(SENT), dtype=torch.float32, device='cuda')
    h.tag(xd.data_ptr(), ld.data_ptr(), Bn, L, mode, tg[1:].data_ptr() if tags else None, fl[GUARD:].data_ptr() if flat else None,
          sc[1:].data_ptr() if scores else None)
    torch.cuda.synchronize()
    tg, fl, sc = tg.cpu().numpy(), fl.cpu().numpy(), sc.cpu().numpy()
    assert (tg[0] == SENT).all() and (tg[-1] == SENT).all(), 'tags: a guard row was written'
    assert (fl[:GUARD] == SENT).all() and (fl[N + GUARD:] == SENT).all(), 'flat tags: a guard was written'
    assert (sc[0] == SENT).all() and (sc[-1] == SENT).all(), 'scores: a guard row was written'
    if not tags:
        assert (tg == SENT).all()
    if not flat:
        assert (fl == SENT).all()
    if not scores:
        assert (sc == SENT).all()
    return (tg[1:-1].astype(np.int64) if tags else None, fl[GUARD:N + GUARD] if flat else None,
            sc[1:-1].reshape(Bn, L, c.C) if scores else None)


def _record(c, got, r):
    if c.kind == 'signed' and os.environ.get('FST4_TAG_REPORT'):
        e = np.abs(got.astype(np.float64) - r.ref64) / (1 + np.abs(r.ref64))
        with open(os.environ['FST4_TAG_REPORT'], 'a') as f:
            f.write('{:<52} {} {} worst {:.3e}\n'.format(fc.case_id(c), c.layout, 'max' if c.semiring else 'sum', float(e.max())))


def _check_scores(c, r, got, what, ref32=None, ref64=None):
    ref32 = r.ref32 if ref32 is None else ref32
    ref64 = r.ref64 if ref64 is None else ref64
    bad = fc.mismatch(c, got, r._replace(ref32=ref32, ref64=ref64))
    assert bad is None, (fc.case_id(c), what, bad)


def _check_tags(c, r, tags, flat, where, what):
    if c.kind == 'exact':
        assert np.array_equal(tags[where], r.want[where]), (fc.case_id(c), what, 'tags')
    else:
        assert fc.tags_allowed(c, r, tags, where), (fc.case_id(c), what, 'tags')
    assert np.array_equal(flat, tags[r.mask]), (fc.case_id(c), what, 'flat tags are not the valid tags, batch-major')
    if c.kind == 'exact':
        assert np.array_equal(flat, r.flat), (fc.case_id(c), what, 'flat tags')


def _check_case(c, h, r, record=False):
    """every mode and every output combination of one handle on one case"""
    from re2nn_seq_amd import _lib
    everywhere = np.ones_like(r.mask)
    # FULL: all L positions, scores unclamped
    tags, flat, sc = _tag(h, c, r.x, r.lengths, _lib.MODE_FULL)
    if record:
        _record(c, sc, r)
    _check_scores(c, r, sc, 'full')
    _check_tags(c, r, tags, flat, everywhere, 'full')
    full = (tags, flat, sc)
    # LOCAL: valid positions; pads are zero rows and -1
    tags, flat, sc = _tag(h, c, r.x, r.lengths, _lib.MODE_LOCAL)
    assert not sc[~r.mask].any() and (tags[~r.mask] == -1).all(), (fc.case_id(c), 'local: pads')
    pad0 = lambda a: np.where(r.mask[..., None], a, 0)     # noqa: E731
    _check_scores(c, r, sc, 'local', pad0(r.ref32), pad0(r.ref64))
    _check_tags(c, r, tags, flat, r.mask, 'local')
    local = (tags, flat, sc)
    # RE: FULL, the last column capped at the threshold as fo.decode_argmax caps it
    tags, flat, sc = _tag(h, c, r.x, r.lengths, _lib.MODE_RE)
    _check_scores(c, r, sc, 're', fc.clamped(r.ref32), fc.clamped(r.ref64))
    assert np.array_equal(tags, full[0]) and np.array_equal(flat, full[1]), (fc.case_id(c), 're: tags')
    # each output on its own: what the call with all three gave (checked above), and nothing else written
    for mode, ref in ((_lib.MODE_FULL, full), (_lib.MODE_LOCAL, local)):
        for k in range(3):
            ask = [False] * 3
            ask[k] = True
            got = _tag(h, c, r.x, r.lengths, mode, *ask)
            assert np.array_equal(got[k], ref[k]), (fc.case_id(c), 'mode', mode, ('tags', 'flat', 'scores')[k] + ' only')


@pytest.mark.parametrize('c', fc.CASES + fc.TIE_CASES, ids=fc.case_id)
def test_tagging_vs_oracle(c):
    from re2nn_seq_amd import _lib
    r = fc.reference(c)
    h = _create(c, r)
    try:
        assert h.num_columns() == c.C
        if NO_SWITCH:
            assert h.kernel_name(_lib.KERN_SCORE) == ('fst4_score_kernel' if c.layout == 'fst4' else 'ind1_score_kernel')
        _check_case(c, h, r, record=True)
    finally:
        h.close()


@pytest.mark.parametrize('c', fc.CHAIN_CASES, ids=fc.case_id)
def test_chain_forms_in_front_of_k3(c, monkeypatch):
    """S = 71, 104, 130 (the register-fed chain, its wide form, the LDS ring) under the default dispatch and under FARNN_NOREGS=1
    (the LDS-ring kernel at every S; the switches are read at create): the same bar for both, and on exact models the same bits"""
    from re2nn_seq_amd import _lib
    r = fc.reference(c)
    scores = []
    for env in ({}, {'FARNN_NOREGS': '1'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        h = _create(c, r)
        try:
            _check_case(c, h, r)
            scores.append(_tag(h, c, r.x, r.lengths, _lib.MODE_FULL)[2])
        finally:
            h.close()
    if c.kind == 'exact':
        assert np.array_equal(scores[0], scores[1])


@pytest.mark.parametrize('cases', fc.VARYING_CASES, ids=lambda cs: cs[0].layout)
def test_one_handle_varying_shapes(cases):
    """(B, L) = (4, 9), (2, 3), (7, 12), (4, 9) through ONE handle: the stash stride changes with L, the workspace grows once"""
    from re2nn_seq_amd import _lib
    refs = [fc.reference(c) for c in cases]
    for r in refs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(r.model, refs[0].model)) and np.array_equal(r.P, refs[0].P)
    h = _create(cases[0], refs[0])
    try:
        outs = []
        for c, r in zip(cases, refs):
            tags, flat, sc = _tag(h, c, r.x, r.lengths, _lib.MODE_FULL)
            _check_scores(c, r, sc, 'full')
            _check_tags(c, r, tags, flat, np.ones_like(r.mask), 'full')
            ltags, lflat, _ = _tag(h, c, r.x, r.lengths, _lib.MODE_LOCAL)
            _check_tags(c, r, ltags, lflat, r.mask, 'local')
            outs.append((tags, flat, sc))
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[-1]))
    finally:
        h.close()


@pytest.mark.parametrize('cases', fc.VARYING_CASES, ids=lambda cs: cs[0].layout)
def test_out_of_vocabulary_token_ids_are_treated_as_pad(cases):
    """token ids outside [0, V) never index the blocks: they behave like the pad word V - 1 (as the i-FST's test of this name pins it)"""
    from re2nn_seq_amd import _lib
    c = cases[0]
    r = fc.reference(c)
    lengths = np.full(c.B, c.L, np.int64)
    bad = np.array(r.x); bad[0, 2] = c.V + 1000; bad[1, 0] = -5; bad[2, 7] = 2 ** 40
    good = bad.copy(); good[0, 2] = good[1, 0] = good[2, 7] = c.V - 1
    h = _create(c, r)
    try:
        outs = [_tag(h, c, xx, lengths, _lib.MODE_FULL) for xx in (bad, good)]
    finally:
        h.close()
    assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))
    _check_scores(c, r, outs[1][2], 'pad ids', fc.oracle_scores(c, r.model, r.P, good, lengths),
                  fc.oracle_scores(c, r.model, r.P, good, lengths, np.float64))


def _ind1_arrays(S, Cn=3, V=5):
    z = np.zeros
    return z((V, S, S), np.float32), z((S, S), np.float32), z((Cn, S, S), np.float32), np.ones(S, np.float32), np.ones(S, np.float32)


def test_ind1_lds_limit_is_refused_at_create():
    """independent=1 keeps (alpha beta^T) .* Tf[x_i] of a token in LDS.  The largest S that fits 160 KiB tags and matches the oracle
    (test_tagging_vs_oracle: the case 'LDS: the largest S within 160 KiB'); the first that does not is refused by the CREATE, with
    FARNN_ERANGE and the LDS message, and no handle comes back: nothing fails at farnn_tag that a create could have refused."""
    from re2nn_seq_amd import _lib
    S = fc.refused_ind1_S()
    assert fc.k3_lds_bytes(S - 1, 3, True) <= fc.LDS_LIMIT < fc.k3_lds_bytes(S, 3, True)
    assert any(c.layout == 'ind1' and c.S == S - 1 for c in fc.CASES)
    T, W, O, h0, hT = _ind1_arrays(S)
    for mask in (False, True):
        with pytest.raises(_lib.FarnnError) as e:
            _lib.create_onehot_ind1(T, W, O, h0, hT, mask_by_output=mask)
        assert 'code {}'.format(ERANGE) in str(e.value) and LDS_TEXT in str(e.value), str(e.value)
    with pytest.raises(_lib.FarnnError) as e:                # the edge-list create builds the same handle
        _lib.create_onehot_ind1_from_edges(5, S, 3, [0], [0], [1], [0], h0, hT)
    assert 'code {}'.format(ERANGE) in str(e.value) and LDS_TEXT in str(e.value), str(e.value)
    # the C ABI: the code, and the out pointer cleared
    lib = _lib.load()
    d = _lib.OnehotInd1Desc(5, S, 3, _lib.ptr(T), _lib.ptr(W), _lib.ptr(O), _lib.ptr(h0), _lib.ptr(hT), None, _lib.SEMIRING['sum'], 0, 0.5, 0, 0)
    out = C.c_void_p(0xdead)
    assert lib.farnn_onehot_ind1_create(C.byref(d), 0, C.byref(out)) == ERANGE and not out.value
    # FST 4-D keeps no such image: the same S creates
    z = np.zeros
    _lib.create_onehot_fst4(z((5, 3, S, S), np.float32), z((3, S, S), np.float32), h0, hT).close()
