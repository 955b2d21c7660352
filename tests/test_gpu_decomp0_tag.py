"""The tagging path of the decomposed FST (FARNN_S_D_W, --independent 0) against its references, on the cases of
tests/decomp0_tag_cases.py: create_decomp_fst and farnn_tag with device pointers -- the create-time folds (scale_by_colsum_kernel,
output_sum_kernel), the recurrence on the folded tables, then decomp0_score_kernel (csrc/decomp1_score.hip.h) on the unscaled
Vgen -- at the sizes where that kernel changes what a thread does (every case's id carries S, R, RW, K, B, L; Case.edge names the
edge in words).

Scores, at the valid positions: tests/util.py: assert_float_path at its default 1e-4 against the float32 and float64 references
(no per-shape bars).  Tags: `tags` at the valid positions and `flat` EQUAL the float64 decode (tests/test_decomp0_tag_cases_cpu.py
holds every case to the gap rule with no position left out), and equal the decode of the kernel's own scores; under the CRF the
float64 Viterbi path.  LOCAL mode: pads are exact zeros and -1.  FULL mode: every position finite, every tag a column or o_idx (behind a Viterbi path, which ends at the length, -1).
Every output is pre-filled with a sentinel (scores NaN, tags -7), the flat tags have one guard entry behind sum(lengths), and each
output asked for alone equals the call with all three bit for bit.

D0_TAG_REPORT=<file>: every case appends its worst |got - ref64| / (1 + |ref64|) before it asserts (a record, never a source for
the bar; profiles/decomp0_tag_error.txt is one such run).
"""
import os

import numpy as np
import pytest
import torch

import decomp0_tag_cases as dc
from util import NO_SWITCH, assert_float_path

pytestmark = pytest.mark.gpu

SENT = -7
ERANGE = -34                                               # include/farnn.h
LIB_NAMES = {'Vgen': 'Vgen', 'C_embed': 'Ce', 'S1': 'S1', 'S2': 'S2', 'C_wildcard': 'Cw', 'S1_wildcard': 'S1w', 'S2_wildcard': 'S2w',
             'wildcard_wildcard': 'WW', 'h0': 'h0', 'hT': 'hT', 'Wss1': 'Wss1', 'Wrs1': 'Wrs1', 'bs1': 'bs1', 'Wss2': 'Wss2',
             'Wrs2': 'Wrs2', 'bs2': 'bs2'}
RECURRENCES = ('decomp_regs_kernel', 'decomp_rows_kernel', 'decomp_chain_kernel')


def _create(c, p, P, trans):
    from re2nn_seq_amd import _lib
    gates = {g: p[g] for g in dc.GATES if g in p}
    return _lib.create_decomp_fst(p['Vgen'], p['C_embed'], p['S1'], p['S2'], p['C_wildcard'], p['S1_wildcard'], p['S2_wildcard'],
                                  p['wildcard_wildcard'], p['h0'], p['hT'], P=P, farnn=c.farnn, gates=gates or None,
                                  sigmoid_exponent=dc.SIG_K, nl=c.nl, semiring='max' if c.semiring else 'sum', threshold=dc.THRESHOLD,
                                  o_idx=dc.o_idx(c), use_crf=bool(c.crf), crf_trans=trans)


def _buffers(Bn, L, K, N):
    return (torch.full((Bn, L), SENT, dtype=torch.int32, device='cuda'), torch.full((N + 1,), SENT, dtype=torch.int64, device='cuda'),
            torch.full((Bn, L, K), float('nan'), dtype=torch.float32, device='cuda'))


def _tag(h, K, x, lengths, mode, tags=True, flat=True, scores=True):
    """one farnn_tag into pre-filled buffers: (tags [B, L] int64, flat [N], scores [B, L, K]), None for what was not asked"""
    from re2nn_seq_amd import _lib
    Bn, L = x.shape
    N = int(np.sum(lengths))
    xd, ld = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(lengths)).cuda()
    tg, fl, sc = _buffers(Bn, L, K, N)
    h.tag(xd.data_ptr(), ld.data_ptr(), Bn, L, _lib.MODE_FULL if mode == dc.FULL else _lib.MODE_LOCAL, tg.data_ptr() if tags else None,
          fl.data_ptr() if flat else None, sc.data_ptr() if scores else None)
    torch.cuda.synchronize()
    tg, fl, sc = tg.cpu().numpy(), fl.cpu().numpy(), sc.cpu().numpy()
    assert fl[N] == SENT, 'flat tags: the guard was written'
    if not tags:
        assert (tg == SENT).all()
    if not flat:
        assert (fl == SENT).all()
    if not scores:
        assert np.isnan(sc).all()
    return tg.astype(np.int64) if tags else None, fl[:N] if flat else None, sc if scores else None


def _record(c, got, r):
    if os.environ.get('D0_TAG_REPORT') and r.mask.any():
        e = np.abs(got.astype(np.float64) - r.ref64)[r.mask] / (1 + np.abs(r.ref64[r.mask]))
        with open(os.environ['D0_TAG_REPORT'], 'a') as f:
            f.write('{:<64} worst {:.3e}\n'.format(dc.case_id(c), float(e.max())))


def _check_outputs(c, r, tags, flat, sc, what):
    """one call's three outputs against the references, in the case's mode"""
    cid = dc.case_id(c)
    m = r.mask
    assert_float_path(sc[m], r.ref32[m], r.ref64[m], err_msg='{} {}'.format(cid, what))
    assert np.array_equal(tags[m], r.flat64), (cid, what, 'tags are not the float64 decode')
    assert np.array_equal(flat, r.flat64), (cid, what, 'flat tags are not the float64 decode')
    assert np.array_equal(tags[m], dc.decode(c, sc, r.lengths, r.trans)[m]), (cid, what, 'tags are not the decode of the returned scores')
    if c.mode == dc.LOCAL:
        assert (sc[~m] == 0).all() and (tags[~m] == -1).all(), (cid, what, 'pads')
    else:
        assert np.isfinite(sc).all(), (cid, what, 'a position that is not finite')
        if c.crf:       # the Viterbi launch behind the score kernel decodes a path of len positions: its pads are -1 in FULL mode too
            assert (tags[~m] == -1).all(), (cid, what, 'pads behind a Viterbi path')
            tags = tags[m]
        assert (((tags >= 0) & (tags < c.K)) | (tags == dc.o_idx(c))).all(), (cid, what, 'a tag that is no column')
    if c.tie is not None:
        c1, c2 = c.tie
        assert np.array_equal(sc[..., c1], sc[..., c2]), (cid, what, 'the planted columns differ')
        won = dc.tie_wins(c, r)
        assert 2 * won.sum() >= m.sum() and (tags[won] == c1).all(), (cid, what, 'the lower index must win')


def _check_case(c, h, r, record=False):
    """the call with every output, then each output on its own"""
    tags, flat, sc = _tag(h, c.K, r.x, r.lengths, c.mode)
    if record:
        _record(c, sc, r)
    _check_outputs(c, r, tags, flat, sc, c.mode)
    every = (tags, flat, sc)
    for k in range(3):
        ask = [False] * 3
        ask[k] = True
        got = _tag(h, c.K, r.x, r.lengths, c.mode, *ask)
        assert np.array_equal(got[k], every[k], equal_nan=k == 2), (dc.case_id(c), ('tags', 'flat', 'scores')[k] + ' only')
    return every


@pytest.mark.parametrize('c', dc.CASES + dc.TIE_CASES, ids=dc.case_id)
def test_tagging_vs_references(c):
    from re2nn_seq_amd import _lib
    r = dc.reference(c)
    h = _create(c, r.p, r.P, r.trans)
    try:
        assert h.num_columns() == c.K
        _check_case(c, h, r, record=True)
        if NO_SWITCH:
            assert h.kernel_name(_lib.KERN_SCORE) == 'decomp0_score_kernel'
            rec = h.kernel_name(_lib.KERN_CHAIN)
            assert rec in RECURRENCES and (rec == 'decomp_chain_kernel' or c.semiring == dc.SUM), rec
    finally:
        h.close()


def test_one_handle_varying_shapes():
    """(B, L) = (4, 9), (2, 3), (7, 17), (4, 9) through ONE handle: the stash stride changes with L, the workspace grows once"""
    cases = dc.VARYING_CASES
    refs = [dc.reference(c) for c in cases]
    h = _create(cases[0], refs[0].p, refs[0].P, refs[0].trans)
    try:
        outs = []
        for c, r in zip(cases, refs):
            outs.append(_check_case(c, h, r))
            lc = c._replace(mode=dc.LOCAL)
            _check_outputs(lc, r, *_tag(h, c.K, r.x, r.lengths, dc.LOCAL), what='local')
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[-1]))
    finally:
        h.close()


def _zero_model(S, R, RW, K, V=5):
    z = lambda *s: np.zeros(s, np.float32)     # noqa: E731
    return dict(Vgen=z(V, R), C_embed=z(K, R), S1=z(S, R), S2=z(S, R), C_wildcard=z(K, RW), S1_wildcard=z(S, RW), S2_wildcard=z(S, RW),
                wildcard_wildcard=z(S, S), h0=np.ones(S, np.float32), hT=np.ones(S, np.float32))


def test_the_lds_limit_is_refused_before_any_output_is_written():
    """The three accepted LDS shapes run in test_tagging_vs_references.  The first shape beyond 160 KiB creates (no create-time
    bound depends on the score kernel's tile) and is refused by farnn_tag with FARNN_ERANGE before the score kernel, the only
    writer of outputs, is launched: every sentinel stays.  A fresh handle at a small shape tags correctly afterwards."""
    from re2nn_seq_amd import _lib
    S, R, RW, K = dc.refused_lds_shape()
    assert dc.d0_geometry(S, R, RW, K, 9).lds + dc.D0_STATIC_LDS > dc.LDS_LIMIT >= dc.d0_geometry(S, R, RW - 1, K, 9).lds + dc.D0_STATIC_LDS
    c = dc.CASES[0]._replace(S=S, R=R, RW=RW, K=K, V=5)
    h = _create(c, _zero_model(S, R, RW, K), None, None)
    try:
        for mode in (_lib.MODE_LOCAL, _lib.MODE_FULL):
            tg, fl, sc = _buffers(4, 9, K, 16)
            x = torch.zeros((4, 9), dtype=torch.int64, device='cuda')
            ln = torch.tensor([9, 1, 0, 6], dtype=torch.int64, device='cuda')
            with pytest.raises(_lib.FarnnError) as e:
                h.tag(x.data_ptr(), ln.data_ptr(), 4, 9, mode, tg.data_ptr(), fl.data_ptr(), sc.data_ptr())
            torch.cuda.synchronize()
            assert 'code {}'.format(ERANGE) in str(e.value) and 'LDS' in str(e.value), str(e.value)
            assert bool((tg == SENT).all()) and bool((fl == SENT).all()) and bool(torch.isnan(sc).all())
    finally:
        h.close()
    c = dc.CASES[0]
    r = dc.reference(c)
    h = _create(c, r.p, r.P, r.trans)
    try:
        _check_outputs(c, r, *_tag(h, c.K, r.x, r.lengths, c.mode), what='after the refusal')
    finally:
        h.close()


def test_more_than_256_label_columns_are_refused_at_create():
    """K = 257 (Kc = 320) never reaches the score kernel: decomp_geometry refuses it, so the grid's largest K is 256"""
    from re2nn_seq_amd import _lib
    assert max(c.K for c in dc.CASES) == dc.K_MAX
    with pytest.raises(_lib.FarnnError) as e:
        _create(dc.CASES[0], _zero_model(5, 6, 3, dc.K_MAX + 1), None, None)
    assert 'code {}'.format(ERANGE) in str(e.value) and 'more than 256 label columns' in str(e.value), str(e.value)


@pytest.mark.parametrize('c', dc.TRAIN_CASES, ids=dc.case_id)
def test_the_training_step_decodes_the_same_tags(c):
    """farnn_decomp_fst_train_step computes the same scores by other kernels (an MFMA score head over 16-position tiles): one step on
    the same weights and batch decodes the tagging handle's tags at every valid position"""
    from re2nn_seq_amd import _lib
    r = dc.reference(c)
    h = _create(c, r.p, r.P, r.trans)
    try:
        tags = _tag(h, c.K, r.x, r.lengths, dc.LOCAL)[0]
    finally:
        h.close()
    dev = torch.device('cuda', 0)
    tc = _lib.DecompFstTrainContext(c.V, c.S, c.R, c.RW, c.K, nl=c.nl, threshold=dc.THRESHOLD, o_idx=dc.o_idx(c), device=0, use_crf=bool(c.crf),
                                    farnn=c.farnn, sigmoid_exponent=dc.SIG_K)
    t = {n: torch.from_numpy(np.array(a)).to(dev).contiguous() for n, a in r.p.items()}
    g = {n: torch.zeros_like(a) for n, a in t.items()}
    weights = {LIB_NAMES[n]: a.data_ptr() for n, a in t.items()}
    outputs = {'d' + LIB_NAMES[n]: a.data_ptr() for n, a in g.items()}
    keep = []
    if r.P is not None:
        keep.append(torch.from_numpy(np.array(r.P)).to(dev))
        weights['P'] = keep[-1].data_ptr()
    if r.trans is not None:
        keep += [torch.from_numpy(np.array(r.trans)).to(dev), torch.zeros((c.K, c.K), device=dev)]
        weights['crf_trans'], outputs['dtrans'] = keep[-2].data_ptr(), keep[-1].data_ptr()
    rng = np.random.RandomState(c.seed + 2)
    labels = rng.randint(0, c.K - (2 if c.crf else 0), size=(c.B, c.L)).astype(np.int64)
    xd, ld, lab = (torch.from_numpy(np.array(a)).to(dev) for a in (r.x, r.lengths, labels))
    loss = torch.zeros((1,), dtype=torch.float32, device=dev)
    got = torch.full((c.B, c.L), SENT, dtype=torch.int32, device=dev)
    outputs['loss'], outputs['tags'] = loss.data_ptr(), got.data_ptr()
    try:
        tc.step(weights, xd.data_ptr(), ld.data_ptr(), lab.data_ptr(), c.B, c.L, int(r.lengths.sum()), outputs, torch.cuda.current_stream(dev).cuda_stream)
    finally:
        torch.cuda.synchronize(dev)
        tc.close()
    got = got.cpu().numpy().astype(np.int64)
    assert np.isfinite(float(loss.cpu()))
    assert np.array_equal(got[r.mask], tags[r.mask]), dc.case_id(c)
    assert np.array_equal(got[r.mask], r.flat64), dc.case_id(c)
