"""The label-map score + decode launch (K2l, csrc/score_decode.hip.h: `label_map_score_kernel`) behind the onehot i-FST recurrence,
at the smallest shapes where it can go wrong, against the oracle's decode of the oracle's scores at EVERY position.

The models are 0/1 automata (synth.random_ifst_tensors) whose path counts stay below 2**24 (asserted per case), so fp32 is exact
whatever the order of the additions: the comparison is bit-exact and skips nothing.

  * states 1, 2, 63, 64, 65, 71, 72 (one and two label-map entries per lane, the padded row SP == S) x labels 2, 5, 128, V = 7;
  * B = 1 and B = 3 with lengths 0, 1, 2, odd, L (an empty sequence, the lone token of a pair, len == L) at L = 1, 2, 33, 34, 65
    (the first and the second trip of a workgroup of 4, 8 or 16 wavefronts); B = 300 x 9 (many short workgroups, flat offsets
    summed in the kernel over more than 64 sequences); B = 1100 x 3 (flat offsets read from the prefix array);
  * LOCAL mode without and with flat tags, FULL mode (pads read row i + 1); pads are -1 in LOCAL mode;
  * two states of different labels with identical edges: equal non-zero top scores, decided by the first index;
  * one handle called twice with different lengths and L.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import farnn_oracle as fo                    # noqa: E402
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from util import NO_SWITCH                               # noqa: E402

pytestmark = pytest.mark.gpu

V = 7
THRESHOLD = 0.5
LOCAL, LOCAL_FLAT, FULL = 'local', 'local+flat', 'full'


def _model(S, C, seed, twins=False):
    from re2nn_seq_amd import synth
    rng = np.random.RandomState(seed)
    # dense enough that most (word, state) pairs have a successor: many states and labels are alive at a position
    # (two states: a wildcard move back to the start state closes a cycle whose path count grows like 2**L)
    T, W, O, h0, hT = synth.random_ifst_tensors(V, S, C, rng, edges_per_word=2.0 * S, n_final=min(2, S),
                                                wildcard_moves=2 if S > 2 else 0)
    loops = np.flatnonzero(np.diag(W))
    T[:, loops, loops] = 0.0                               # (a word's self loop on top of a wildcard's doubles the count per token)
    if twins:
        # two states of DIFFERENT labels with identical in / out edges carry equal values at every position: their labels'
        # scores tie wherever nothing else feeds either label
        plain = [s for s in range(1, S) if O[C - 1, s] == 0]
        a, b = plain[0], plain[1]
        for M in (T, W[None]):
            M[:, :, b] = M[:, :, a]
            M[:, b, :] = M[:, a, :]
        h0[b], hT[b] = h0[a], hT[a]
        la = int(O[:, a].argmax())
        O[:, b] = 0.0
        O[(la + 1) % (C - 1), b] = 1.0
    return T, W, O, h0, hT


def _batch(lengths, L, rng):
    lengths = np.minimum(np.asarray(lengths, np.int64), L)
    x = np.full((len(lengths), L), V - 1, dtype=np.int64)
    for b, n in enumerate(lengths):
        x[b, :n] = rng.randint(0, V - 1, size=int(n))
    return x, lengths


def _check(h, model, x, lengths, mode, o_idx, what):
    """one farnn_tag call (tags only: the label-map score launch) against the oracle at every position; returns the number of
    positions whose two best clamped scores are equal and non-zero"""
    from re2nn_seq_amd import _lib
    B, L = x.shape
    C = model[2].shape[0]
    ref = fo.onehot_ifst_scores(*model, x, lengths)
    assert np.isfinite(ref).all() and float(np.abs(ref).max()) < 2.0 ** 24, what      # the exact range: the oracle alone decides
    want = fo.decode_argmax(ref, THRESHOLD, o_idx)
    xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(lengths).cuda()
    tags = torch.full((B, L), -7, dtype=torch.int32, device='cuda')
    total = int(lengths.sum())
    with_flat = mode != LOCAL and total > 0
    flat = torch.full((max(total, 1),), -7, dtype=torch.int64, device='cuda')
    h.tag(xd.data_ptr(), ld.data_ptr(), B, L, _lib.MODE_FULL if mode == FULL else _lib.MODE_LOCAL, tags.data_ptr(),
          flat.data_ptr() if with_flat else None, None)
    torch.cuda.synchronize()
    if NO_SWITCH:                                          # (which kernels ran: the default dispatch only)
        assert h.kernel_name(_lib.KERN_SCORE) == 'label_map_score_kernel', what
        assert 'fused' not in h.kernel_name(_lib.KERN_CHAIN), what
    tg = tags.cpu().numpy().astype(np.int64)
    mask = np.arange(L)[None, :] < lengths[:, None]
    if mode == FULL:
        assert np.array_equal(tg, want), what
    else:
        assert np.array_equal(tg[mask], want[mask]), what
        assert (tg[~mask] == -1).all(), what
    if with_flat:
        assert np.array_equal(flat.cpu().numpy()[:total], fo.forward_local_tags(ref, lengths, THRESHOLD, o_idx)), what
    clamped = ref.copy()
    clamped[..., -1] = np.minimum(clamped[..., -1], THRESHOLD)
    top2 = np.sort(clamped, axis=-1)[..., -2:]
    live = np.ones_like(mask) if mode == FULL else mask
    return int(((top2[..., 0] == top2[..., 1]) & (top2[..., 1] != 0) & live).sum())


def _lengths_sets(L):
    odd = min(L, 5 if L > 5 else 3)
    return [[0, 1, L], [2, odd, L], [L, 0, 2], [0], [1], [2], [odd], [L]]


@pytest.mark.parametrize('S', [1, 2, 63, 64, 65, 71, 72])
@pytest.mark.parametrize('C', [2, 5, 128])
def test_label_map_score_small_shapes(S, C):
    from re2nn_seq_amd import _lib
    model = _model(S, C, seed=1000 * S + C)
    o_idx = 1 % C
    h = _lib.create_onehot_ifst(*model, threshold=THRESHOLD, o_idx=o_idx)
    rng = np.random.RandomState(S * 131 + C)
    try:
        for L in (1, 2, 33, 34, 65):
            for lens in _lengths_sets(L):
                x, lengths = _batch(lens, L, rng)
                for mode in (LOCAL, LOCAL_FLAT, FULL):
                    _check(h, model, x, lengths, mode, o_idx, 'S={} C={} L={} lengths={} {}'.format(S, C, L, list(lengths), mode))
    finally:
        h.close()


@pytest.mark.parametrize('B,L', [(300, 9), (1100, 3)])
def test_label_map_score_flat_offsets(B, L):
    """B = 300: the flat offset of a sequence summed in the kernel over more than 64 sequences before it; B = 1100 (beyond the
    batch the kernel sums itself): read from the prefix array"""
    from re2nn_seq_amd import _lib
    S, C = 71, 128
    model = _model(S, C, seed=77)
    h = _lib.create_onehot_ifst(*model, threshold=THRESHOLD, o_idx=1)
    rng = np.random.RandomState(B)
    try:
        x, lengths = _batch(rng.randint(0, L + 1, size=B), L, rng)
        for mode in (LOCAL, LOCAL_FLAT, FULL):
            _check(h, model, x, lengths, mode, 1, 'B={} L={} {}'.format(B, L, mode))
    finally:
        h.close()


@pytest.mark.parametrize('S,C', [(71, 128), (65, 5), (64, 5)])
def test_label_map_score_first_index_ties(S, C):
    from re2nn_seq_amd import _lib
    model = _model(S, C, seed=5 * S + C, twins=True)
    h = _lib.create_onehot_ifst(*model, threshold=THRESHOLD, o_idx=1)
    rng = np.random.RandomState(S + C)
    ties = 0
    try:
        for L in (9, 34):
            x, lengths = _batch([L, L - 1, 3, L, 7, 0, L, 2], L, rng)
            for mode in (LOCAL_FLAT, FULL):
                ties += _check(h, model, x, lengths, mode, 1, 'twins S={} C={} L={} {}'.format(S, C, L, mode))
    finally:
        h.close()
    assert ties > 0, 'no position with two equal non-zero best scores: the tie rule was not exercised'


def test_label_map_score_same_handle_twice():
    """nothing of one call (lengths, L, the flat offsets) survives into the next"""
    from re2nn_seq_amd import _lib
    S, C = 71, 128
    model = _model(S, C, seed=9)
    h = _lib.create_onehot_ifst(*model, threshold=THRESHOLD, o_idx=1)
    rng = np.random.RandomState(3)
    try:
        for L, lens in ((34, [34, 1, 0, 17, 2]), (9, [3, 9, 9, 0, 5, 1, 8]), (65, [65, 2]), (34, [1, 34, 33, 2, 0])):
            x, lengths = _batch(lens, L, rng)
            for mode in (LOCAL_FLAT, LOCAL, FULL):
                _check(h, model, x, lengths, mode, 1, 'twice L={} lengths={} {}'.format(L, lens, mode))
    finally:
        h.close()
