"""The 16-bit image of the onehot i-FST's blocks (csrc/layout.hip.h: half_image_kernel; csrc/chain_dest.hip.h: the H16 form of the
destination-split recurrence, `chain_regs_kernel<f16 blocks>`).

A model whose premixed block entries are all f16 values exactly gets the image at create, and the recurrence-only launch reads it:
the same f32 products into the same accumulators in the same order, from half the bytes.  So for an eligible model the tags and the
scores derived from the stash are BIT-IDENTICAL to the same library under FARNN_NOHALF=1 (the f32 blocks; computed once, by one
child process that runs this file as a script), whatever the weights -- also where the order of the additions matters.  Against
the oracle: bit-identical wherever the oracle itself is exact (its float32 and float64 evaluations agree at every entry: the 0/1
automata, most of the 2048 / -2048 ones); where it is not (dyadic non-integer weights, doubling loops behind a 2048: numpy rounds products and sums separately, the
kernels fuse them) the project's one rule for a floating-point path (tests/util.py: assert_float_path) -- the oracle's own distance
from float64 is the bar there, not a constant of this test.

  * state counts 1, 5 (lanes without a row), 8, 9 (the first 16-byte chunk of f16), 40, 41 (columns a lane's second image chunk
    starts at), 71, 72;  V = 12, C = 6;
  * one batch of nine sequences of lengths 0, 1, 3, 4, 5 (around the ring depth, 4), 14 = L, ...; a batch of one sequence;
  * tags only (recurrence + label-map score launch) and scores (FARNN_NOFUSE=1: recurrence + score tiles read the stash);
  * the CRF path (K = C + 2), tags only with no switch set (the default dispatch) and with scores: against the child.
An ineligible model (one entry 1/3, 2049, 65520, 2**-20; only in W; only in the last word's block), S = 73 and the max semiring
keep the f32 form and equal the oracle as before.
No entry point of the library rewrites the blocks of a live handle (every writer of Mf / Mb is a stage of a create), so there is no
stale image to test through one; the last test re-creates a handle with one entry rewritten and back.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import farnn_oracle as fo                    # noqa: E402
from util import NO_SWITCH, assert_float_path, in_float64   # noqa: E402

pytestmark = pytest.mark.gpu

V, C, L = 12, 6, 14
RING = 4                                                  # csrc/chain_regs_params.hip.h: RD_D
LENGTHS = [0, 1, RING - 1, RING, RING + 1, L, L, 2, 7]
STATES = [1, 5, 8, 9, 40, 41, 71, 72]
KINDS = ['01', 'dyadic', 'big']
HALF_NAME, F32_NAME = 'chain_regs_kernel<f16 blocks>', 'chain_regs_kernel'


def _model(S, kind, seed=0):
    from re2nn_seq_amd import synth
    rng = np.random.RandomState(1000 * S + seed)
    T, W, O, h0, hT = synth.random_ifst_tensors(V, S, C, rng, edges_per_word=max(3.0, 0.6 * S), n_final=min(2, S))
    if kind == 'dyadic':
        # multiples of 1/8 up to magnitude 4 (T + W: up to 8), most of them non-integers: every entry an f16 exactly, the
        # state values soon need more than 24 bits
        kT = rng.randint(1, 33, size=T.shape) * rng.choice([-1, 1], size=T.shape)
        kW = rng.randint(1, 33, size=W.shape) * rng.choice([-1, 1], size=W.shape)
        T = (T * kT / 8.0).astype(np.float32)
        W = (W * kW / 8.0).astype(np.float32)
    elif kind == 'big':
        # premixed entries 2048 and -2048 (T + W), from the start state: two sequences of the batches below begin with words 0 and 1
        T[0, 0, S - 1] = 2048.0 - W[0, S - 1]
        T[1, 0, S - 1] = -2048.0 - W[0, S - 1]
    return T, W, O, h0, hT


def _batches(seed):
    rng = np.random.RandomState(seed)
    lengths = np.asarray(LENGTHS, np.int64)
    x = np.full((len(lengths), L), V - 1, dtype=np.int64)
    for b, n in enumerate(lengths):
        x[b, :n] = rng.randint(0, V - 1, size=int(n))
    x[5, 0], x[6, 0] = 0, 1
    x1 = x[5:6].copy()
    return [(x, lengths), (x1, np.asarray([L], np.int64))]


def _run(model, x, lengths, want_scores, use_crf=False, semiring='sum'):
    """one farnn_tag call on a fresh handle; (tags, scores or None, recurrence kernel label)"""
    import torch
    from re2nn_seq_amd import _lib
    if want_scores:
        os.environ['FARNN_NOFUSE'] = '1'                  # (read at create) recurrence-only launch, the score tiles read the stash
    try:
        h = _lib.create_onehot_ifst(*model, use_crf=use_crf, semiring=semiring)
    finally:
        if want_scores:
            del os.environ['FARNN_NOFUSE']
    B = x.shape[0]
    K = h.num_columns()
    xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(lengths).cuda()
    tags = torch.full((B, L), -7, dtype=torch.int32, device='cuda')
    scores = torch.full((B, L, K), -7.0, dtype=torch.float32, device='cuda') if want_scores else None
    h.tag(xd.data_ptr(), ld.data_ptr(), B, L, _lib.MODE_LOCAL, tags.data_ptr(), None, scores.data_ptr() if want_scores else None)
    torch.cuda.synchronize()
    name = h.kernel_name(_lib.KERN_CHAIN)
    h.close()
    return tags.cpu().numpy(), (scores.cpu().numpy() if want_scores else None), name


def _eligible_results():
    """every eligible case under the switches of THIS process: {key: array}"""
    out = {}
    for S in STATES:
        for kind in KINDS:
            model = _model(S, kind)
            for bi, (x, lengths) in enumerate(_batches(S)):
                key = 'S{}_{}_b{}'.format(S, kind, bi)
                tags, _, name = _run(model, x, lengths, False)
                tags2, scores, name2 = _run(model, x, lengths, True)
                out[key + '_tags'], out[key + '_tags2'], out[key + '_scores'] = tags, tags2, scores
                out[key + '_names'] = np.asarray([name, name2])
    model = _model(41, 'dyadic')
    x, lengths = _batches(41)[0]
    tags0, _, name0 = _run(model, x, lengths, False, use_crf=True)     # the default CRF dispatch: recurrence + score / Viterbi kernel
    tags, scores, name = _run(model, x, lengths, True, use_crf=True)
    out['crf_tags0'], out['crf_tags'], out['crf_scores'], out['crf_names'] = tags0, tags, scores, np.asarray([name0, name])
    return out


@pytest.fixture(scope='module')
def both(tmp_path_factory):
    """(this process's results, the FARNN_NOHALF=1 child's): each computed once"""
    mine = _eligible_results()
    path = str(tmp_path_factory.mktemp('half') / 'nohalf.npz')
    env = dict(os.environ, FARNN_NOHALF='1')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return mine, dict(np.load(path))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('S', STATES)
def test_eligible_model_reads_the_image_and_changes_no_bit(S, kind, both):
    mine, child = both
    model = _model(S, kind)
    for bi, (x, lengths) in enumerate(_batches(S)):
        key = 'S{}_{}_b{}'.format(S, kind, bi)
        what = '{} B={}'.format(key, x.shape[0])
        if NO_SWITCH:
            assert list(mine[key + '_names']) == [HALF_NAME, HALF_NAME], what
            assert list(child[key + '_names']) == [F32_NAME, F32_NAME], what
        mask = np.arange(L)[None, :] < lengths[:, None]
        # the same library on the f32 blocks: every bit
        assert np.array_equal(mine[key + '_tags'], child[key + '_tags']), what
        assert np.array_equal(mine[key + '_tags2'], child[key + '_tags2']), what
        assert np.array_equal(mine[key + '_scores'].view(np.uint32), child[key + '_scores'].view(np.uint32)), what
        # the oracle
        with np.errstate(all='ignore'):
            ref = fo.onehot_ifst_scores(*model, x, lengths)
            ref64 = in_float64(lambda p, *a: fo.onehot_ifst_scores(p['T'], p['W'], p['O'], p['h0'], p['hT'], *a),
                               dict(zip(('T', 'W', 'O', 'h0', 'hT'), model)), x, lengths)
        assert np.isfinite(ref).all(), what
        got = mine[key + '_scores']
        exact = np.array_equal(ref.astype(np.float64), ref64)
        print('{}: oracle exact {}, max |got - ref32| {:.3e}, max |ref32 - ref64| {:.3e}'.format(
            what, exact, float(np.abs(got[mask] - ref[mask]).max()) if mask.any() else 0.0, float(np.abs(ref - ref64).max())))
        assert exact or kind != '01', what                   # (the 0/1 automata stay inside fp32's exact range; the others: the oracle decides)
        want = fo.decode_argmax(ref, 0.5, 0)
        if exact:
            assert np.array_equal(got[mask], ref[mask]), what
            safe = mask
        else:
            assert_float_path(got[mask], ref[mask], ref64[mask], err_msg=what)
            refc = ref64.copy(); refc[..., -1] = np.minimum(refc[..., -1], 0.5)
            top2 = np.sort(refc, axis=-1)[..., -2:]
            safe = mask & ((top2[..., 1] - top2[..., 0]) > 2e-4 * (1.0 + np.abs(ref64).max(-1)) + 2 * np.abs(ref - ref64).max(-1))
        for t in (mine[key + '_tags'], mine[key + '_tags2']):
            assert np.array_equal(t[safe], want[safe]), what
            assert (t[~mask] == -1).all(), what


def test_crf_path_reads_the_image_and_changes_no_bit(both):
    mine, child = both
    if NO_SWITCH:
        assert list(mine['crf_names']) == [HALF_NAME, HALF_NAME]
        assert list(child['crf_names']) == [F32_NAME, F32_NAME]
    assert np.array_equal(mine['crf_tags0'], child['crf_tags0'])
    assert mine['crf_scores'].shape[-1] == C + 2
    assert np.array_equal(mine['crf_tags'], child['crf_tags'])
    assert np.array_equal(mine['crf_scores'].view(np.uint32), child['crf_scores'].view(np.uint32))


def _f32_form_equals_oracle(model, S, what, semiring='sum'):
    x, lengths = _batches(S)[0]
    tags, _, name = _run(model, x, lengths, False, semiring=semiring)
    if NO_SWITCH:
        assert name == (F32_NAME if S <= 72 else name) and 'f16' not in name, (what, name)
        assert name.startswith('chain_regs_kernel' if S <= 72 else 'chain_wide_kernel'), (what, name)
    _, scores, name2 = _run(model, x, lengths, True, semiring=semiring)
    assert 'f16' not in name2, (what, name2)
    sem = fo.SEMIRING_MAX if semiring == 'max' else fo.SEMIRING_SUM
    with np.errstate(all='ignore'):
        ref = fo.onehot_ifst_scores(*model, x, lengths, semiring=sem)
        ref64 = in_float64(lambda p, *a: fo.onehot_ifst_scores(p['T'], p['W'], p['O'], p['h0'], p['hT'], *a, semiring=sem),
                           dict(zip(('T', 'W', 'O', 'h0', 'hT'), model)), x, lengths)
    mask = np.arange(L)[None, :] < lengths[:, None]
    assert_float_path(scores[mask], ref[mask], ref64[mask], err_msg=what)
    want = fo.decode_argmax(ref, 0.5, 0)
    refc = ref64.copy(); refc[..., -1] = np.minimum(refc[..., -1], 0.5)
    top2 = np.sort(refc, axis=-1)[..., -2:]
    safe = mask & ((top2[..., 1] - top2[..., 0]) > 2e-4 * (1.0 + np.abs(ref64).max(-1)) + 2 * np.abs(ref - ref64).max(-1))
    assert np.array_equal(tags[safe], want[safe]), what
    return name


@pytest.mark.parametrize('value', [1.0 / 3.0, 2049.0, 65520.0, 2.0 ** -20], ids=['third', '2049', '65520', 'f16_subnormal'])
def test_one_ineligible_entry_keeps_the_f32_form(value):
    T, W, O, h0, hT = _model(9, '01')
    T[3, 0, 8] = value
    _f32_form_equals_oracle((T, W, O, h0, hT), 9, 'entry {}'.format(value))


def test_ineligible_value_only_in_the_wildcard_matrix():
    T, W, O, h0, hT = _model(9, '01')
    W[1, 2] = 1.0 / 3.0
    _f32_form_equals_oracle((T, W, O, h0, hT), 9, 'W entry 1/3')


def test_ineligible_value_only_in_the_last_words_block():
    T, W, O, h0, hT = _model(9, '01')
    T[V - 1, 8, 7] = 1.0 / 3.0
    _f32_form_equals_oracle((T, W, O, h0, hT), 9, 'last word entry 1/3')


def test_wide_form_has_no_image():
    _f32_form_equals_oracle(_model(73, '01'), 73, 'S = 73')


def test_max_semiring_has_no_image():
    _f32_form_equals_oracle(_model(9, '01'), 9, 'max semiring', semiring='max')


def test_a_rewritten_entry_never_meets_an_old_image():
    """the blocks of a handle are written by its create alone: new weights are a new handle, whose image is checked again"""
    T, W, O, h0, hT = _model(9, '01')
    x, lengths = _batches(9)[0]
    i = tuple(np.argwhere(T[:V - 1] == 1.0)[0])
    before, _, name = _run((T, W, O, h0, hT), x, lengths, False)
    if NO_SWITCH:
        assert name == HALF_NAME
    T[i] = 1.0 / 3.0
    _f32_form_equals_oracle((T, W, O, h0, hT), 9, 'entry rewritten to 1/3')
    T[i] = 1.0
    again, _, _ = _run((T, W, O, h0, hT), x, lengths, False)
    assert np.array_equal(before, again)


if __name__ == '__main__':                                # the child: the same cases under the parent's environment + FARNN_NOHALF=1
    np.savez(sys.argv[1], **_eligible_results())
