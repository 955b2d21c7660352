"""Every form of the CRF decode on EXACT ties, where the first index of the maximum must win (torch.max's rule, crf.py:147-149):
viterbi_hist_kernel with the scores computed inside it and behind the score kernel (csrc/viterbi_hist.hip.h: eight lanes per tag
pair, 32-source blocks + leftover slots, the tail wavefront, the back-trace's ballot over 64-lane slices), the stored-back-pointer
viterbi_kernel (csrc/score_decode.hip.h), and the one-launch form of the A/B build -- on the planted models of
tests/crf_tie_cases.py: integer scores that every form computes bit for bit, transitions under which 25-100 % of the decoded
path's arg-maxima are tied (tests/test_crf_tie_cases_cpu.py holds the inputs to their coverage floors and shows that a decode
taking the last index instead gives other tags in most sequences).  Tags must EQUAL the oracle's; there is no tolerance.

Also the non-CRF decode of the same models (score_tile_kernel / label_map_score_kernel / the decode beside the recurrence), where
the last column clamped to the threshold ties a label in front of it.
"""
import os

import numpy as np
import pytest
import torch

import crf_tie_cases as tc
from util import NO_SWITCH, ab_build, run_module_in_ab_build

pytestmark = pytest.mark.gpu

FORMS = {'default': {}, 'unfused': {'FARNN_VITERBI_UNFUSED': '1'}, 'backpointers': {'FARNN_VITERBI_BP': '1', 'FARNN_VITERBI_UNFUSED': '1'},
         'nolabelmap': {'FARNN_NOLABELMAP': '1'}}


def _params():
    out = []
    for c in tc.CASES:
        for form, env in FORMS.items():
            if form == 'nolabelmap' and c.o_kind != 'labelmap':
                continue
            # the kernel this (case, form) takes: the 158 KiB condition of launch_viterbi, restated in crf_tie_cases.expected_form
            out.append(pytest.param(c, form, id='{}-{}-{}'.format(tc.case_id(c), form, tc.expected_form(c.K, c.S, c.L, tuple(env)))))
    return out


def _tag(h, r, mode, scores=False):
    Bn, L = r.x.shape
    xd, ld = torch.from_numpy(np.array(r.x)).cuda(), torch.from_numpy(np.array(r.lengths)).cuda()
    tags = torch.full((Bn, L), -7, dtype=torch.int32, device='cuda')
    flat = torch.full((int(r.lengths.sum()),), -7, dtype=torch.int64, device='cuda')
    sc = torch.full((Bn, L, h.num_columns()), -7.0, dtype=torch.float32, device='cuda') if scores else None
    h.tag(xd.data_ptr(), ld.data_ptr(), Bn, L, mode, tags.data_ptr(), flat.data_ptr(), sc.data_ptr() if scores else None)
    torch.cuda.synchronize()
    return tags.cpu().numpy().astype(np.int64), flat.cpu().numpy(), sc.cpu().numpy() if scores else None


def _check_crf(c, env, monkeypatch, expect_chain=None):
    from re2nn_seq_amd import _lib
    r = tc.reference(c)
    for k, v in env.items():                                # (the switches are read when the handle is created)
        monkeypatch.setenv(k, v)
    T, W, O, h0, hT = r.model
    h = _lib.create_onehot_ifst(T, W, O, h0, hT, threshold=c.threshold, o_idx=c.o_idx, use_crf=True, crf_trans=r.tr)
    try:
        assert h.num_columns() == c.K
        # a wrong SCORE is not a wrong decode: what the handle returns (the score kernel's view of the recurrence) is the planted
        # columns bit for bit, the START / STOP columns zero, the pads zero
        _, _, sc = _tag(h, r, _lib.MODE_LOCAL, scores=True)
        assert np.array_equal(sc[r.mask], r.ext[r.mask]), 'scores differ from the planted columns'
        assert not sc[~r.mask].any()
        for mode in (_lib.MODE_LOCAL, _lib.MODE_FULL):
            tags, flat, _ = _tag(h, r, mode)
            what = (tc.case_id(c), sorted(env), 'full' if mode == _lib.MODE_FULL else 'local')
            bad = [b for b in range(tc.B) if not np.array_equal(tags[b][r.mask[b]], r.want[b][r.mask[b]])]
            assert not bad, (what, 'sequences', bad, 'lengths', [c.lengths[b] for b in bad])
            assert (tags[~r.mask] == -1).all(), what
            assert np.array_equal(flat, r.flat), what
            # Which Viterbi kernel ran cannot be read back: kernel_name(KERN_SCORE) is one constant for every CRF handle.  The kernel in
            # the case id is the RESTATED expectation (crf_tie_cases.expected_form), checked against the dispatch's source on the CPU
            # only.  The name does tell the one-launch form from the others (the A/B build carries both).
            chain = h.kernel_name(_lib.KERN_CHAIN)
            if NO_SWITCH:
                assert ('chain_viterbi' in chain) == (expect_chain is not None), (what, chain)
    finally:
        h.close()


@pytest.mark.parametrize('c,form', _params())
def test_crf_decode_on_planted_ties(c, form, monkeypatch):
    _check_crf(c, FORMS[form], monkeypatch)


def _one_launch_range(c):
    return 32 <= c.K <= 131 and c.L <= 64 and c.S <= 108     # the form's range (tests/test_gpu_chain_viterbi.py)


def test_crf_decode_on_planted_ties_one_launch_form(monkeypatch):
    """FARNN_CV_ONE=1: recurrence + scores + the same decode body in one launch (csrc/chain_viterbi.hip), compiled into the A/B build"""
    if not ab_build():
        pytest.skip('the one-launch CRF step is compiled into the A/B build only (test_one_launch_form_in_the_ab_build runs it there)')
    n = 0
    for c in tc.CASES:
        if _one_launch_range(c):
            _check_crf(c, {'FARNN_CV_ONE': '1'}, monkeypatch, expect_chain='chain_viterbi_kernel')
            n += 1
    assert n >= 30


def test_one_launch_form_in_the_ab_build():
    r = run_module_in_ab_build(os.path.abspath(__file__), k='test_crf_decode_on_planted_ties_one_launch_form')
    if r is None:
        pytest.skip('already the A/B build, or libfarnn_hip_probes.so was not built (csrc/build.py --probes)')
    assert r.returncode == 0 and ' passed' in r.stdout and ' failed' not in r.stdout and ' skipped' not in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


ARGMAX_FORMS = {'default': {}, 'nofuse': {'FARNN_NOFUSE': '1'}, 'nolabelmap': {'FARNN_NOLABELMAP': '1'},
                'nofuse+nolabelmap': {'FARNN_NOFUSE': '1', 'FARNN_NOLABELMAP': '1'}}


@pytest.mark.parametrize('a,form', [pytest.param(a, f, id=tc.argmax_case_id(a) + '-' + f) for a in tc.ARGMAX_CASES
                                    for f in (tuple(ARGMAX_FORMS) if a.case.o_kind == 'labelmap' else ('default', 'nofuse'))])
def test_argmax_decode_on_threshold_ties(a, form, monkeypatch):
    """use_crf = False: the last column clamped to the threshold against the labels in front of it, in each of the three decodes:
    beside the recurrence (bs_score_tiles, csrc/beside.hip.h: the default of a dense model where its score tiles fit, and of a label
    map over more than 72 states), label_map_score_kernel (the default of a label map over up to 72 states; FARNN_NOFUSE=1 beyond) and
    score_tile_kernel (FARNN_NOFUSE=1 for a dense model, with FARNN_NOLABELMAP=1 for a label map).  Under FARNN_NOFUSE=1 the score
    launch really ran, so kernel_name(KERN_SCORE) tells which one; '<fused' in kernel_name(KERN_CHAIN) tells the first form."""
    from re2nn_seq_amd import _lib
    c, r, g = a.case, tc.reference(a.case), tc.argmax_reference(a)
    if a.case.o_kind == 'dense' or a.threshold == 0.0:
        assert g.threshold_ties >= 1                        # (counted from the oracle)
    for k, v in ARGMAX_FORMS[form].items():
        monkeypatch.setenv(k, v)
    lm = c.o_kind == 'labelmap' and 'nolabelmap' not in form
    T, W, O, h0, hT = r.model
    h = _lib.create_onehot_ifst(T, W, O, h0, hT, threshold=a.threshold, o_idx=c.o_idx)
    try:
        # with the scores asked for (never the label-map scan): the scores AND the tags of that call
        tags, flat, sc = _tag(h, r, _lib.MODE_FULL, scores=True)
        assert np.array_equal(sc, g.scores), 'scores differ from the oracle'
        assert np.array_equal(tags, g.want) and np.array_equal(flat, g.flat), (tc.argmax_case_id(a), form, 'with scores')
        if NO_SWITCH and 'nofuse' in form:
            assert '<fused' not in h.kernel_name(_lib.KERN_CHAIN) and h.kernel_name(_lib.KERN_SCORE) == 'score_tile_kernel'
        for mode in (_lib.MODE_LOCAL, _lib.MODE_FULL):
            tags, flat, _ = _tag(h, r, mode)
            what = (tc.argmax_case_id(a), form, 'full' if mode == _lib.MODE_FULL else 'local')
            if mode == _lib.MODE_FULL:
                assert np.array_equal(tags, g.want), what
            else:
                assert np.array_equal(tags[r.mask], g.want[r.mask]) and (tags[~r.mask] == -1).all(), what
            assert np.array_equal(flat, g.flat), what
            if not NO_SWITCH:
                continue                                    # (under a dispatch switch from outside: results only)
            chain, score = h.kernel_name(_lib.KERN_CHAIN), h.kernel_name(_lib.KERN_SCORE)
            if 'nofuse' in form:
                assert '<fused' not in chain and score == ('label_map_score_kernel' if lm else 'score_tile_kernel'), (what, chain, score)
            elif lm and c.S <= 72:
                assert '<fused' not in chain and score == 'label_map_score_kernel', (what, chain, score)
            elif c.S <= 72 and c.K - 2 > 192:
                # (four 64-column chunks of score tiles do not fit the 80 KiB a workgroup has beside a second one: launch_chain
                #  falls back to the recurrence alone, and the score kernel follows)
                assert '<fused' not in chain and score == 'score_tile_kernel', (what, chain, score)
            else:
                assert '<fused' in chain, (what, chain)
    finally:
        h.close()
