"""The head of the recurrence-only launch (csrc/chain_regs.hip.h, HEAD), with the label-map score launch behind it.

What the head does differently from the forms that kept theirs: wavefront 0 selects (sequence, length) WHILE the other seven store
the set-up, two words of LDS hand the pair on behind ONE barrier; of `hist` only row 0 and the pad columns are initialised; the
block offsets go to LDS only for a sequence of more than 64 steps (in front of a second barrier).  What can go wrong: a word of the
set-up that nobody stores any more, a pad column left as it was, ties of the selection resolved otherwise (two workgroups on one
sequence, another none), the 64-step seam.  So:

  * B in {1, 2, 3, 64, 65, 257}, L in {1, 2, 31, 32, 33, 63, 64, 65, 130}, S in {1, 4, 71, 72}: eleven (B, L, S) that hold every
    value (L = 65 and 130 fill the offsets and reload the window; 32 | 33: one and two trips of the score launch's sixteen
    wavefronts over a sequence -- the two sides of the switch a two-workgroup form of that launch had; it was measured and dropped);
  * lengths with 0, 1, L and long runs of equal lengths (the selection's ties);
  * MODE_LOCAL, MODE_FULL and the flat output, guard rows around `tags` and `flat`;
  * a 0 / 1 automaton and a dyadic non-integer one (some words' blocks halved: every state of a step carries the same power of
    two, so float32 stays exact) -- the f16 kernel: tags equal the C port's and the FARNN_NOHALF=1 child's, every bit;
  * the dyadic model with one entry 1/3 -- the f32 destination-split kernel: scores within 1e-4 of the oracle, tags equal outside
    2e-4 margins (bench.py's parity rule);
  * the stash's pad columns, read back from the A/B build (the one library with a read-back), after a call at a larger (B, L);
  * one step captured into a graph at two batch sizes, replayed.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import c_port                                # noqa: E402
from oracle import farnn_oracle as fo                    # noqa: E402
from util import NO_SWITCH                               # noqa: E402

pytestmark = pytest.mark.gpu

V, C = 12, 5
CASES = [(1, 1, 1), (2, 2, 4), (3, 31, 71), (64, 32, 72), (65, 33, 71), (257, 63, 4), (257, 64, 71), (3, 65, 72), (65, 130, 71),
         (1, 64, 71), (2, 130, 4)]
KINDS = ['01', 'dyadic', 'third']
HALF_NAME, F32_NAME, SCORE_NAME = 'chain_regs_kernel<f16 blocks>', 'chain_regs_kernel', 'label_map_score_kernel'
GUARD = 64


def _model(S, kind):
    from re2nn_seq_amd import synth
    rng = np.random.RandomState(77 * S + 5)
    T, W, O, h0, hT = synth.random_ifst_tensors(V, S, C, rng, edges_per_word=max(1.0, 0.5 * S), n_final=min(2, S))
    if S <= 4:
        # (T + W stays 0 / 1 and upper triangular: no doubling loop -- 130 steps of one overflow f32)
        W = np.diag(np.diag(W)).astype(np.float32)
        T = np.triu(T * (W == 0.0)[None]).astype(np.float32)
    if kind != '01':
        # every fourth word's block (wildcard included) halved, the wildcard folded in: all entries 0, 1/2 or 1
        T = (T + W[None]).astype(np.float32)
        T[::4] *= 0.5
        W = np.zeros_like(W)
    if kind == 'third':
        T[3, 0, min(S - 1, 8)] = 1.0 / 3.0
    return T, W, O, h0, hT


def _batch(B, L):
    rng = np.random.RandomState(1000 * B + L)
    lengths = rng.randint(0, L + 1, size=B).astype(np.int64)
    lengths[B // 4:B // 2] = max(L // 2, 1)              # a long run of equal lengths
    lengths[B - B // 8:] = L                             # ... and one of full-length rows
    head = [L, 0, 1, L][:B]
    lengths[:len(head)] = head
    x = np.full((B, L), V - 1, dtype=np.int64)
    for b, n in enumerate(lengths):
        x[b, :n] = rng.randint(0, V - 1, size=int(n))
    return x, lengths


def _tag(h, x, lengths, mode, want_flat, want_scores=False):
    """one farnn_tag call with guard rows around `tags` and `flat`: (tags, flat or None, scores or None, kernel names)"""
    import torch
    from re2nn_seq_amd import _lib
    B, L = x.shape
    xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(lengths).cuda()
    tags = torch.full((B + 2, L), -7, dtype=torch.int32, device='cuda')
    n = B * L if mode == _lib.MODE_FULL else int(lengths.sum())
    flat = torch.full((n + 2 * GUARD,), -7, dtype=torch.int64, device='cuda') if want_flat else None
    scores = torch.full((B, L, h.num_columns()), -7.0, dtype=torch.float32, device='cuda') if want_scores else None
    h.tag(xd.data_ptr(), ld.data_ptr(), B, L, mode, tags[1:].data_ptr(), flat[GUARD:].data_ptr() if want_flat else None,
          scores.data_ptr() if want_scores else None)
    torch.cuda.synchronize()
    tags = tags.cpu().numpy()
    assert (tags[0] == -7).all() and (tags[-1] == -7).all(), 'a store outside tags'
    if want_flat:
        flat = flat.cpu().numpy()
        assert (flat[:GUARD] == -7).all() and (flat[GUARD + n:] == -7).all(), 'a store outside flat'
        flat = flat[GUARD:GUARD + int(lengths.sum())]
    return (tags[1:-1], flat, scores.cpu().numpy() if want_scores else None,
            (h.kernel_name(_lib.KERN_CHAIN), h.kernel_name(_lib.KERN_SCORE)))


def _results():
    """every case under the switches of THIS process: {key: array}"""
    from re2nn_seq_amd import _lib
    out = {}
    for B, L, S in CASES:
        x, lengths = _batch(B, L)
        for kind in KINDS:
            key = 'B{}_L{}_S{}_{}'.format(B, L, S, kind)
            h = _lib.create_onehot_ifst(*_model(S, kind))
            out[key + '_local'], out[key + '_flat'], _, names = _tag(h, x, lengths, _lib.MODE_LOCAL, True)
            out[key + '_full'], _, _, names2 = _tag(h, x, lengths, _lib.MODE_FULL, False)
            out[key + '_local2'], _, _, _ = _tag(h, x, lengths, _lib.MODE_LOCAL, False)     # the handle again, after FULL
            h.close()
            out[key + '_names'] = np.asarray(names + names2)
    return out


@pytest.fixture(scope='module')
def both(tmp_path_factory):
    """(this process's results, the FARNN_NOHALF=1 child's): each computed once"""
    mine = _results()
    path = str(tmp_path_factory.mktemp('head') / 'nohalf.npz')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'results', path], env=dict(os.environ, FARNN_NOHALF='1'),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return mine, dict(np.load(path))


_REFS = {}


def _oracle(B, L, S, kind):
    """(float32 oracle scores, C-port tags) of a case: computed once"""
    key = (B, L, S, kind)
    if key not in _REFS:
        T, W, O, h0, hT = _model(S, kind)
        x, lengths = _batch(B, L)
        with np.errstate(all='ignore'):
            ref = fo.onehot_ifst_scores(T, W, O, h0, hT, x, lengths)
        ctags, _, _ = c_port.onehot_ifst_tag(T + W, O, h0, hT, x, lengths, nthreads=4)
        _REFS[key] = (ref, ctags)
    return _REFS[key]


@pytest.mark.parametrize('B,L,S', CASES, ids=['B{}-L{}-S{}'.format(*c) for c in CASES])
@pytest.mark.parametrize('kind', KINDS[:2])
def test_f16_kernel_tags_every_bit(B, L, S, kind, both):
    mine, child = both
    x, lengths = _batch(B, L)
    ref, ctags = _oracle(B, L, S, kind)
    key = 'B{}_L{}_S{}_{}'.format(B, L, S, kind)
    if NO_SWITCH:
        assert list(mine[key + '_names']) == [HALF_NAME, SCORE_NAME] * 2, key
        assert list(child[key + '_names']) == [F32_NAME, SCORE_NAME] * 2, key
    valid = np.arange(L)[None, :] < lengths[:, None]
    assert np.isfinite(ref).all(), key
    want_full = fo.decode_argmax(ref, 0.5, 0)
    assert np.array_equal(want_full[valid], ctags[valid]), key + ': the two oracles disagree'
    for part in ('_local', '_local2'):
        assert np.array_equal(mine[key + part], ctags), key + part            # (-1 at the pads in both)
        assert np.array_equal(mine[key + part], child[key + part]), key + part
    assert np.array_equal(mine[key + '_full'], want_full), key
    assert np.array_equal(mine[key + '_full'], child[key + '_full']), key
    assert np.array_equal(mine[key + '_flat'], ctags[valid]), key
    assert np.array_equal(mine[key + '_flat'], child[key + '_flat']), key


@pytest.mark.parametrize('B,L,S', CASES, ids=['B{}-L{}-S{}'.format(*c) for c in CASES])
def test_f32_kernel_by_the_parity_rule(B, L, S, both, monkeypatch):
    from re2nn_seq_amd import _lib
    mine, _ = both
    x, lengths = _batch(B, L)
    ref, _ = _oracle(B, L, S, 'third')
    key = 'B{}_L{}_S{}_third'.format(B, L, S)
    if NO_SWITCH:
        assert list(mine[key + '_names']) == [F32_NAME, SCORE_NAME] * 2, key
    monkeypatch.setenv('FARNN_NOFUSE', '1')              # (read at create) the recurrence-only launch, the score tiles read the stash
    h = _lib.create_onehot_ifst(*_model(S, 'third'))
    tags_s, _, scores, names = _tag(h, x, lengths, _lib.MODE_LOCAL, False, True)
    h.close()
    assert 'f16' not in names[0]
    valid = np.arange(L)[None, :] < lengths[:, None]
    if not valid.any():
        return
    err = float(np.abs(scores[valid] - ref[valid]).max())
    print('{}: max score error {:.3e}, max |ref| {:.3e}'.format(key, err, float(np.abs(ref[valid]).max())))
    assert err <= 1e-4 * max(1.0, float(np.abs(ref[valid]).max())), key
    want = fo.decode_argmax(ref, 0.5, 0)
    refc = ref.copy(); refc[..., -1] = np.minimum(refc[..., -1], 0.5)
    top2 = np.sort(refc, axis=-1)[..., -2:]
    safe = valid & ((top2[..., 1] - top2[..., 0]) > 2e-4)
    full_safe = (top2[..., 1] - top2[..., 0]) > 2e-4
    for t in (mine[key + '_local'], mine[key + '_local2'], tags_s):
        assert np.array_equal(t[safe], want[safe]), key
        assert (t[~valid] == -1).all(), key
    assert np.array_equal(mine[key + '_full'][full_safe], want[full_safe]), key
    fs = safe[valid]
    assert np.array_equal(mine[key + '_flat'][fs], want[valid][fs]), key


def _stash_pads(path):
    """(the child, in the A/B build) a call at (65, 130), then one at (3, 31) on the same handle: the pad columns of the second call's stash"""
    import torch                                         # noqa: F401
    from re2nn_seq_amd import _lib
    S, SP = 71, 72
    h = _lib.create_onehot_ifst(*_model(S, '01'))
    lib = _lib.load()
    lib.farnn_debug_stash.restype = ctypes.c_int
    lib.farnn_debug_stash.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong]
    out = {}
    for B, L in ((65, 130), (3, 31)):
        x, lengths = _batch(B, L)
        tags, _, _, names = _tag(h, x, lengths, _lib.MODE_LOCAL, False)
        n = B * (L + 1) * SP
        A, Bk = np.empty(n, np.float32), np.empty(n, np.float32)
        assert lib.farnn_debug_stash(h.raw, A.ctypes.data, Bk.ctypes.data, n) == 0
        out['A_{}'.format(B)], out['Bk_{}'.format(B)] = A.reshape(B, L + 1, SP), Bk.reshape(B, L + 1, SP)
        out['tags_{}'.format(B)], out['names_{}'.format(B)] = tags, np.asarray(names)
    h.close()
    np.savez(path, **out)


def test_stash_pads_are_exact_zeros_after_a_larger_call(tmp_path):
    from re2nn_seq_amd import _lib
    assert os.path.exists(_lib.AB_LIB_PATH), 'the A/B build (csrc/build.py --probes) carries the stash read-back'
    path = str(tmp_path / 'stash.npz')
    env = dict(os.environ, FARNN_LIB=_lib.AB_LIB_PATH)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'stash', path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = dict(np.load(path))
    S = 71
    for B, L in ((65, 130), (3, 31)):
        x, lengths = _batch(B, L)
        _, ctags = _oracle(B, L, S, '01')
        assert np.array_equal(got['tags_{}'.format(B)], ctags), B
        if NO_SWITCH:
            assert got['names_{}'.format(B)][0] == HALF_NAME
        for name in ('A', 'Bk'):
            st = got['{}_{}'.format(name, B)]
            rows = np.arange(L + 1)[None, :] <= lengths[:, None]          # rows 0 .. len of every sequence are written by the call
            pads = st[..., S:][rows]
            assert pads.size and (pads.view(np.uint32) == 0).all(), (name, B)
            assert np.abs(st[..., :S][rows]).max() > 0, (name, B)
    # row 0 is the initial state
    T, W, O, h0, hT = _model(S, '01')
    assert np.array_equal(got['A_3'][:, 0, :S], np.broadcast_to(h0, (3, S)))
    assert np.array_equal(got['Bk_3'][:, 0, :S], np.broadcast_to(hT, (3, S)))


def test_one_step_in_a_graph_at_two_batch_sizes():
    import torch
    from re2nn_seq_amd import _lib
    S, L = 71, 64
    model = _model(S, '01')
    h = _lib.create_onehot_ifst(*model)
    sizes = (65, 3)
    h.reserve(max(sizes), L)
    dev = torch.device('cuda', 0)
    side = torch.cuda.Stream(dev)
    bufs = {B: dict(x=torch.zeros((B, L), dtype=torch.int64, device=dev), l=torch.ones((B,), dtype=torch.int64, device=dev),
                    tags=torch.full((B, L), -7, dtype=torch.int32, device=dev)) for B in sizes}

    def call(B, stream):
        u = bufs[B]
        h.tag(u['x'].data_ptr(), u['l'].data_ptr(), B, L, _lib.MODE_LOCAL, u['tags'].data_ptr(), None, None, stream)

    with torch.cuda.stream(side):                        # eager first (lazy attribute set-up)
        for B in sizes:
            call(B, side.cuda_stream)
    side.synchronize()
    graphs = {}
    for B in sizes:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            call(B, torch.cuda.current_stream(dev).cuda_stream)
        graphs[B] = g
    if NO_SWITCH:
        assert (h.kernel_name(_lib.KERN_CHAIN), h.kernel_name(_lib.KERN_SCORE)) == (HALF_NAME, SCORE_NAME)
    for B in (65, 3, 65, 3):
        x, lengths = _batch(B, L)
        bufs[B]['x'].copy_(torch.from_numpy(x)); bufs[B]['l'].copy_(torch.from_numpy(lengths))
        bufs[B]['tags'].fill_(-7)
        graphs[B].replay()
        torch.cuda.synchronize()
        _, ctags = _oracle(B, L, S, '01')
        assert np.array_equal(bufs[B]['tags'].cpu().numpy(), ctags), B
    h.close()


if __name__ == '__main__':                                # the children: the cases under FARNN_NOHALF=1 | the stash in the A/B build
    if sys.argv[1] == 'results':
        np.savez(sys.argv[2], **_results())
    else:
        _stash_pads(sys.argv[2])
