"""The start of the recurrence-only launch (csrc/chain_regs.hip.h, HEAD; csrc/launch_order.hip.h): the selecting wavefront finds
(sequence, length) of its launch slot with one round for the top class, a galloping descent and a bisection inside the bracket,
loads the row's first 64 token ids and hands the pair and the block offsets to the compute wavefronts through LDS (the variant
build in which every compute wavefront selects for itself runs the same search).  What can go wrong is the SELECTION: a rank
resolved otherwise than the rank the other direction's workgroup and the score launch behind it resolve, the first window's offsets
for another row or in the wrong order, a tie broken otherwise than by index, a class missed at the edges of the descent, the clamp, a register or lane
boundary of the per-lane length registers (4 / 8 / 16 a lane: B <= 256 / 512 / 1024).  Two workgroups on one sequence and none on
another leave a stash row of an earlier call or of nobody: wrong tags.

Every case is ONE tag call on a 0 / 1 automaton at V = 40 (exact in f16 and f32):
  * tags equal the C port's at every valid position;
  * tags are byte-identical to the same handle's under FARNN_NOHALF=1 (the f32 kernel: the same head; one child process);
  * tags equal the call's that also asks for scores (it scores beside the recurrence: the head that was not changed).
B in {1, 2, 3, 63, 64, 65, 255, 256, 257, 512, 513, 1024} x the eight length patterns, L in {1, 2, 64, 65} and S in {1, 71, 72} dealt
over them so that every (B, pattern), every (L, S) and every (L, pattern) occurs (L = 65: the window path with its second barrier);
every (L, S, pattern) once more at B = 257.

The host-side test restates the search in plain Python and holds it to sorted(range(B), key=lambda i: (-len[i], i))[rank] for
every rank of a few thousand seeded length vectors (B <= 65, L <= 8): no GPU.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import c_port                                # noqa: E402
from util import NO_SWITCH                               # noqa: E402

V, C = 40, 5
BS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 512, 513, 1024]
LS = [1, 2, 64, 65]
SS = [1, 71, 72]
PATTERNS = ['equal', 'all_L', 'all_0', 'descending', 'ascending', 'one_long', 'clamp', 'headline']


def _cases():
    out = []
    for i, B in enumerate(BS):
        for j, pat in enumerate(PATTERNS):
            out.append((B, LS[(i + j) % 4], SS[(i + 2 * j + (i + j) // 4) % 3], pat))
    for L in LS:
        for S in SS:
            for pat in PATTERNS:
                if (257, L, S, pat) not in out:
                    out.append((257, L, S, pat))
    return out


CASES = _cases()


def _model(S):
    from re2nn_seq_amd import synth
    rng = np.random.RandomState(77 * S + 5)
    T, W, O, h0, hT = synth.random_ifst_tensors(V, S, C, rng, edges_per_word=max(1.0, 0.5 * S), n_final=min(2, S))
    if S <= 4:
        # (T + W stays 0 / 1 and upper triangular: no doubling loop over 65 steps)
        W = np.diag(np.diag(W)).astype(np.float32)
        T = np.triu(T * (W == 0.0)[None]).astype(np.float32)
    return T, W, O, h0, hT


def _lengths(B, L, pat):
    """the `len` vector as the library gets it (the clamp pattern leaves [0, L])"""
    rng = np.random.RandomState(1000 * B + 10 * L + PATTERNS.index(pat))
    i = np.arange(B)
    if pat == 'equal':
        n = np.full(B, max(L // 2, 1))
    elif pat == 'all_L':
        n = np.full(B, L)
    elif pat == 'all_0':
        n = np.zeros(B)
    elif pat == 'descending':                            # strictly, as far as [0, L] reaches: then in runs
        n = L - (i * (L + 1)) // max(B, L + 1)
    elif pat == 'ascending':
        n = (i * (L + 1)) // max(B, L + 1)
    elif pat == 'one_long':
        n = np.ones(B)
        n[B // 2] = L
    elif pat == 'clamp':
        n = rng.randint(-3, L + 4, size=B)
        n[0] = L + 3
        n[B - 1] = -2
    else:                                                # the headline's draw
        n = rng.randint(min(5, L), L + 1, size=B)
    return n.astype(np.int64)


def _batch(B, L, pat):
    """(x, len as passed, len clamped)"""
    raw = _lengths(B, L, pat)
    n = np.clip(raw, 0, L)
    rng = np.random.RandomState(7 * B + L)
    x = np.full((B, L), V - 1, dtype=np.int64)
    for b in range(B):
        x[b, :n[b]] = rng.randint(0, V - 1, size=int(n[b]))
    return x, raw, n


def _key(B, L, S, pat):
    return 'B{}_L{}_S{}_{}'.format(B, L, S, pat)


def _results(with_scores):
    """every case under the switches of THIS process: {key: tags}, {key + '_sc': tags of the call that asks for scores}"""
    import torch
    from re2nn_seq_amd import _lib
    out = {}
    handles = {S: _lib.create_onehot_ifst(*_model(S)) for S in SS}
    for B, L, S, pat in CASES:
        h = handles[S]
        x, raw, _ = _batch(B, L, pat)
        xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(raw).cuda()
        key = _key(B, L, S, pat)
        for sc in ((False, True) if with_scores else (False,)):
            tags = torch.full((B, L), -7, dtype=torch.int32, device='cuda')
            scores = torch.empty((B, L, h.num_columns()), dtype=torch.float32, device='cuda') if sc else None
            h.tag(xd.data_ptr(), ld.data_ptr(), B, L, _lib.MODE_LOCAL, tags.data_ptr(), None, scores.data_ptr() if sc else None)
            torch.cuda.synchronize()
            out[key + ('_sc' if sc else '')] = tags.cpu().numpy()
            if not sc:
                out[key + '_name'] = np.asarray(h.kernel_name(_lib.KERN_CHAIN))
    for h in handles.values():
        h.close()
    return out


@pytest.fixture(scope='module')
def both(tmp_path_factory):
    """(this process's results, the FARNN_NOHALF=1 child's): each computed once"""
    mine = _results(True)
    path = str(tmp_path_factory.mktemp('head_select') / 'nohalf.npz')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, FARNN_NOHALF='1'),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return mine, dict(np.load(path))


@pytest.mark.gpu
@pytest.mark.parametrize('B,L,S,pat', CASES, ids=[_key(*c) for c in CASES])
def test_tags_of_one_call(B, L, S, pat, both):
    mine, child = both
    key = _key(B, L, S, pat)
    x, _, n = _batch(B, L, pat)
    T, W, O, h0, hT = _model(S)
    ctags, _, _ = c_port.onehot_ifst_tag(T + W, O, h0, hT, x, n, nthreads=4)
    valid = np.arange(L)[None, :] < n[:, None]
    if NO_SWITCH:
        assert str(mine[key + '_name']) == 'chain_regs_kernel<f16 blocks>', mine[key + '_name']
        assert str(child[key + '_name']) == 'chain_regs_kernel', child[key + '_name']
    assert np.array_equal(mine[key][valid], ctags[valid]), key + ': not the C port\'s tags'
    assert mine[key].tobytes() == child[key].tobytes(), key + ': the f16 and the f32 kernel disagree'
    assert np.array_equal(mine[key][valid], mine[key + '_sc'][valid]), key + ': not the tags of the call that asks for scores'


def test_every_combination_is_drawn():
    got = set(CASES)
    assert {(B, p) for B, _, _, p in got} == {(B, p) for B in BS for p in PATTERNS}
    assert {(L, S) for _, L, S, _ in got} == {(L, S) for L in LS for S in SS}
    assert {(L, S, p) for B, L, S, p in got if B == 257} == {(L, S, p) for L in LS for S in SS for p in PATTERNS}


# ---- the search, restated (launch_order.hip.h, select_by_length_rank_top_wave) ------------------------------------------------
def _select_top(lens, L, rank):
    """(sequence, class, count_ge rounds) of `rank`: the top class first, a galloping descent, a bisection inside the bracket"""
    v = [min(max(int(n), 0), L) for n in lens]
    rounds = [0]

    def count_ge(t):
        rounds[0] += 1
        return sum(1 for n in v if n >= t)

    lo, hi, above, gap = 0, L, 0, 0
    while lo < hi:
        t = L - gap
        if t <= lo:
            break
        c = count_ge(t)
        if c > rank:
            lo = t
            break
        hi, above = t - 1, c
        gap = 2 * gap + 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        c = count_ge(mid)
        if c > rank:
            lo = mid
        else:
            hi, above = mid - 1, c
    rem = rank - above
    members = [i for i, n in enumerate(v) if n == lo]   # index order: the kernel's register-major, then lane
    return members[rem], lo, rounds[0]


def test_search_restated_on_the_host():
    rng = np.random.RandomState(20240)
    vectors = []
    for _ in range(3000):
        B, L = int(rng.randint(1, 66)), int(rng.randint(0, 9))
        kind = rng.randint(0, 4)
        if kind == 0:
            lens = rng.randint(0, L + 1, size=B)
        elif kind == 1:
            lens = rng.randint(-2, L + 3, size=B)        # the clamp
        elif kind == 2:
            lens = np.full(B, rng.randint(0, L + 1))     # one class: ties by index
        else:
            lens = np.where(rng.rand(B) < 0.2, L, rng.randint(0, L + 1, size=B))
        vectors.append((lens, L))
    for L in range(0, 9):                                # ... and the fixed patterns
        for B in (1, 2, 3, 63, 64, 65):
            i = np.arange(B)
            vectors += [(np.full(B, L), L), (np.zeros(B, int), L), (L - i % (L + 1), L), (i % (L + 1), L),
                        (np.where(i == B // 2, L, min(1, L)), L)]
    for lens, L in vectors:
        B = len(lens)
        c = np.clip(lens, 0, L)
        order = sorted(range(B), key=lambda i: (-c[i], i))
        for rank in range(B):
            seq, cls, rounds = _select_top(lens, L, rank)
            assert (seq, cls) == (order[rank], c[order[rank]]), (list(lens), L, rank)
            if cls == L:
                assert rounds <= 1, (list(lens), L, rank)      # the rows that decide the launch's length: one round
            assert rounds <= 2 * max(L, 1).bit_length() + 1, (list(lens), L, rank)


if __name__ == '__main__':                                # the child: the cases under the parent's environment + FARNN_NOHALF=1
    np.savez(sys.argv[1], **_results(False))
