"""The LDS instructions of the destination-split recurrence's step (csrc/chain_dest.hip.h; the recurrence-only launch,
`chain_regs_kernel` and `chain_regs_kernel<f16 blocks>`).

On the 16-bit image of a model whose o (the column sums of the output matrix) is all ones, a chain's exchange word is its `hist` word
bit for bit, and `chain_regs_one_kernel` stores ONE word per step, into `hist` rows 80 floats apart; the partners read the state of
step t from `hist` row t: pad columns S .. 79 of every row must be exact zeros, the writer copies SP floats out of every 80.  A model
with a general o (states that carry no label: o has zeros) and a model without the image keep the two-store kernel.
The arithmetic is untouched, so:

  * where every partial sum is exactly representable in float32 (checked HERE on the CPU, in float64: `_exact_model_run` bounds
    every sum of a step by the sum of its terms' magnitudes and takes the lowest set bit of any term as the grid they live on) tags
    and scores equal oracle/farnn_oracle.py EXACTLY: 0/1 automata, small dyadic weights (0.5, 1, 2, -1), one entry 2049 (no f16:
    the f32 form), without a non-linearity and with relu -- 508 of the 572 such cases, every short batch among them;
  * with tanh nothing is exact, and in 64 long batches (70 steps) the path counts leave that range: there the project's rule for a
    floating-point path (tests/util.py, assert_float_path: the oracle's own distance from float64 is the bar);
  * the handle that reads the 16-bit image equals the FARNN_NOHALF=1 handle bit for bit, tags and scores, in every case (one child
    process computes them all once).

Shapes: S in {1, 5, 12, 13, 59, 60, 61, 68, 69, 71, 72} (rows per wavefront 1 .. 12, pad widths 0 .. 3, the wavefront that owns
state chunks 15 - 17); lengths 0, 1, 2, 3, 4, 5, 7, 8, 9, 64, 65, 70 in buffers of L = 70, 64, 9, 5, 1 (ring depth 4, the steady /
checked boundary at 2 x 4 steps, the address window beyond 64 steps); B = 9, 3, 2, 1; modes LOCAL and FULL.
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

V, C = 12, 6
STATES = [1, 5, 12, 13, 59, 60, 61, 68, 69, 71, 72]
# (buffer length L, lengths): together every length of {0, 1, 2, 3, 4, 5, 7, 8, 9, 64, 65, 70} and B = 9, 3, 2, 1
BATCHES = [(70, [70, 0, 65, 64, 9, 8, 7, 5, 4]), (9, [9, 3, 1]), (64, [64, 2]), (5, [0]), (1, [1])]
KINDS = ['01', '01_unlabelled', 'dyadic', 'dyadic_unlabelled', 'no_f16']
NLS = ['none', 'relu', 'tanh']
HALF_NAME, F32_NAME = 'chain_regs_kernel<f16 blocks>', 'chain_regs_kernel'


def _model(S, kind):
    from re2nn_seq_amd import synth
    rng = np.random.RandomState(77 * S + len(kind))
    T, W, O, h0, hT = synth.random_ifst_tensors(V, S, C, rng, edges_per_word=max(3.0, 0.6 * S), n_final=min(2, S))
    if kind.startswith('dyadic'):
        # a few edges at 0.5, 2 and -1: few enough that 70 steps stay on a grid float32 holds (checked, _exact_model_run)
        idx = np.argwhere(T == 1.0)
        for n, (v, i, j) in enumerate(idx[rng.permutation(len(idx))[:max(3, len(idx) // 8)]]):
            T[v, i, j] = (0.5, 2.0, -1.0)[n % 3]
        h0 = (h0 * 0.5).astype(np.float32)
    if kind == 'no_f16':
        T[3, 0, S - 1] = 2049.0 - W[0, S - 1]             # an integer no f16 holds: the f32 form
    if S == 1 or kind == 'no_f16':
        h0, hT = (h0 * 2.0 ** -40).astype(np.float32), (hT * 2.0 ** -40).astype(np.float32)   # (one state doubles 70 times, the 2049 edge feeds loops: stay inside float32)
    if kind.endswith('unlabelled') and S > 1:
        O[:, rng.permutation(S)[:max(1, S // 3)]] = 0.0   # states that carry no label: o has zeros, the backward chain keeps two stores
    return T, W, O, h0, hT


def _batch(L, lengths, seed):
    rng = np.random.RandomState(seed)
    lengths = np.asarray(lengths, np.int64)
    x = np.full((len(lengths), L), V - 1, dtype=np.int64)
    for b, n in enumerate(lengths):
        x[b, :n] = rng.randint(0, V - 1, size=int(n))
    if lengths[0] > 0:
        x[0, 0] = 3                                       # (no_f16: the 2049 edge leaves the start state on word 3)
    return x, lengths


def _lowbit(a):
    """the value of the lowest set bit of every float64 in `a` (inf where a == 0)"""
    m, e = np.frexp(np.abs(a))
    mi = (m * 2.0 ** 53).astype(np.int64)
    lb = (mi & -mi).astype(np.float64) * 2.0 ** (e.astype(np.float64) - 53)
    return np.where(a == 0, np.inf, lb)


def _exact(terms, axis):
    """every partial sum of `terms` along `axis`, in any order, is a float32 exactly: they are multiples of the smallest lowest bit of
    any term and no larger than the sum of the magnitudes; that quotient stays below 2^24"""
    mag = np.abs(terms).sum(axis)
    grid = _lowbit(terms).min(axis)
    ok = (mag == 0) | (mag / np.where(np.isfinite(grid), grid, 1.0) < 2.0 ** 24)
    return bool(ok.all()) and bool((np.abs(terms) < 2.0 ** 126).all())


def _exact_model_run(model, x, lengths, relu, full):
    """the recurrences and the scores of oracle.onehot_ifst_scores in float64, step by step, with `_exact` on every sum that the
    kernels form (a step's dot products, the scaling by o, the score sums): True when float32 holds all of them exactly"""
    T, W, O, h0, hT = (np.asarray(a, np.float64) for a in model)
    B, L = x.shape
    Tf, o = T + W, O.sum(0)
    n = lengths                                           # (FULL mode too: the backward chain reverses the sequence's own prefix)
    xb = fo.reverse_prefix(x, n)
    hf, hb = np.repeat(h0[None], B, 0), np.repeat(hT[None], B, 0)
    fw, bw = [hf], [hb]
    ok = True
    for i in range(L):
        pf = hf[:, :, None] * Tf[x[:, i]]                                   # [B, from, to]
        pb = (hb * o)[:, None, :] * Tf[xb[:, i]]                            # [B, to, from]
        ok = ok and _exact(pf, 1) and _exact(pb, 2) and _exact((pf.sum(1) * o)[..., None], 2)
        hf, hb = pf.sum(1) * o, pb.sum(2)
        if relu:
            hf, hb = np.maximum(hf, 0), np.maximum(hb, 0)
        fw.append(hf); bw.append(hb)
    fw, bw = np.stack(fw, 1), np.stack(bw, 1)
    rb = fo.reverse_prefix(bw, np.asarray(n) + 1)
    ab = fw[:, 1:] * rb[:, 1:L + 1]
    return ok and _exact(ab[:, :, None, :] * O[None, None], 3)


def _run(model, x, lengths, nl, mode_full, want_scores):
    import torch
    from re2nn_seq_amd import _lib
    if want_scores:
        os.environ['FARNN_NOFUSE'] = '1'                  # (read at create) recurrence-only launch, the score tiles read the stash
    try:
        h = _lib.create_onehot_ifst(*model, nl=nl)
    finally:
        if want_scores:
            del os.environ['FARNN_NOFUSE']
    B, L = x.shape
    K = h.num_columns()
    xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(lengths).cuda()
    tags = torch.full((B, L), -7, dtype=torch.int32, device='cuda')
    scores = torch.full((B, L, K), -7.0, dtype=torch.float32, device='cuda') if want_scores else None
    h.tag(xd.data_ptr(), ld.data_ptr(), B, L, _lib.MODE_FULL if mode_full else _lib.MODE_LOCAL, tags.data_ptr(), None,
          scores.data_ptr() if want_scores else None)
    torch.cuda.synchronize()
    name = h.kernel_name(_lib.KERN_CHAIN)
    h.close()
    return tags.cpu().numpy(), (scores.cpu().numpy() if want_scores else None), name


def _cases():
    for S in STATES:
        for kind in KINDS:
            for nl in NLS:
                # every batch for the plain and the unlabelled 0/1 automata; the long and the short batch elsewhere
                batches = range(len(BATCHES)) if kind.startswith('01') and nl == 'none' else (0, 1)
                for bi in batches:
                    for full in (False, True):
                        yield S, kind, nl, bi, full


def _key(S, kind, nl, bi, full):
    return 'S{}_{}_{}_b{}_{}'.format(S, kind, nl, bi, 'full' if full else 'local')


def _results():
    """every case under the switches of THIS process: {key: array}"""
    out = {}
    for S, kind, nl, bi, full in _cases():
        model = _model(S, kind)
        x, lengths = _batch(*BATCHES[bi], seed=S + bi)
        key = _key(S, kind, nl, bi, full)
        tags, _, name = _run(model, x, lengths, nl, full, False)
        tags2, scores, name2 = _run(model, x, lengths, nl, full, True)
        out[key + '_tags'], out[key + '_tags2'], out[key + '_scores'] = tags, tags2, scores
        out[key + '_names'] = np.asarray([name, name2])
    return out


@pytest.fixture(scope='module')
def both(tmp_path_factory):
    """(this process's results, the FARNN_NOHALF=1 child's): each computed once"""
    mine = _results()
    path = str(tmp_path_factory.mktemp('step_lds') / 'nohalf.npz')
    env = dict(os.environ, FARNN_NOHALF='1')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return mine, dict(np.load(path))


@pytest.mark.parametrize('nl', NLS)
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('S', STATES)
def test_step_equals_the_oracle_and_the_f32_blocks(S, kind, nl, both):
    mine, child = both
    model = _model(S, kind)
    n_exact = 0
    for S_, kind_, nl_, bi, full in _cases():
        if (S_, kind_, nl_) != (S, kind, nl):
            continue
        x, lengths = _batch(*BATCHES[bi], seed=S + bi)
        B, L = x.shape
        key = _key(S, kind, nl, bi, full)
        if NO_SWITCH:
            want_name = F32_NAME if kind == 'no_f16' else HALF_NAME
            assert list(mine[key + '_names']) == [want_name, want_name], key
            assert list(child[key + '_names']) == [F32_NAME, F32_NAME], key
        # the same library on the f32 blocks: every bit
        assert np.array_equal(mine[key + '_tags'], child[key + '_tags']), key
        assert np.array_equal(mine[key + '_tags2'], child[key + '_tags2']), key
        assert np.array_equal(mine[key + '_scores'].view(np.uint32), child[key + '_scores'].view(np.uint32)), key
        # the oracle runs every sequence over the whole buffer (pad words included), as FULL mode does; LOCAL mode stops at the length
        n = lengths
        mask = np.ones((B, L), bool) if full else np.arange(L)[None, :] < lengths[:, None]
        code = fo.NL_CODES[nl]
        with np.errstate(all='ignore'):
            ref = fo.onehot_ifst_scores(*model, x, n, nl=code)
        got = mine[key + '_scores']
        want = fo.decode_argmax(ref, 0.5, 0)
        exact = nl != 'tanh' and _exact_model_run(model, x, lengths, nl == 'relu', full)
        n_exact += exact
        assert np.isfinite(ref[mask]).all(), key
        if exact:
            assert np.array_equal(got[mask], ref[mask]), key
            safe = mask
        else:
            # tanh, and the few long batches whose path counts leave float32's exact range (the 2049 edge, the densest automata)
            ref64 = in_float64(lambda p, *a: fo.onehot_ifst_scores(p['T'], p['W'], p['O'], p['h0'], p['hT'], *a, nl=code),
                               dict(zip(('T', 'W', 'O', 'h0', 'hT'), model)), x, n)
            assert_float_path(got[mask], ref[mask], ref64[mask], err_msg=key)
            refc = ref64.copy(); refc[..., -1] = np.minimum(refc[..., -1], 0.5)
            top2 = np.sort(refc, axis=-1)[..., -2:]
            safe = mask & ((top2[..., 1] - top2[..., 0]) > 2e-4 * (1.0 + np.abs(ref64).max(-1)) + 2 * np.abs(ref - ref64).max(-1))
        for t in (mine[key + '_tags'], mine[key + '_tags2']):
            assert np.array_equal(t[safe], want[safe]), key
            assert (t[~mask] == -1).all(), key
    assert nl == 'tanh' or n_exact >= 2, 'every model without tanh is exact in float32 on its short batch at least'


if __name__ == '__main__':                                # the child: the same cases under the parent's environment + FARNN_NOHALF=1
    np.savez(sys.argv[1], **_results())
