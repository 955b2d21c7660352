"""The drawn cases of the decomposed FST's max-semiring training step (FARNN_S_D_W, --train_mode max), shared by
tests/test_decomp0_max_train_cpu.py (every case is found within MAX_DRAWS draws and keeps the gap rule) and
tests/test_gpu_decomp0_max_train.py (the C-ABI against the float32 / float64 restatement on them).

A case is drawn from decomp0_train_ref.signed_base and redrawn until decomp0_max_train_ref.check_gap holds, every gradient is
live and well conditioned in float32 (badly_drawn) and the float32 and float64 restatements decode alike.  The shapes are the
smallest that reach each edge of the kernels:
  S     1, 2 (one candidate, two), 63 | 64 | 65 (a wavefront of chain threads), 192 (TM_MAX_S, twelve 16-row MFMA tiles)
  R, Q  3 | 4 | 5 (the MFMA k step), 15 | 16 | 17 (a block of MFMA columns), 65 (a second rank block of d0max_wgrad_kernel)
  words 15 | 16 | 17 | 33 distinct words (d0max_wgrad_kernel's chunk of 16: one chunk, a full one, two, three), one word filling
        the batch, V far above the distinct words
  B     1 and odd; lengths 0, 1 and L in one batch; K = 4 with the CRF
The large-S cases use relu and short sequences: the drawn factors are small multiples of 1/4, so the candidates of the live steps
are exact in float32 and float64 and every tie among them is exact in both (the gap rule's exact-tie clause)."""
import numpy as np
import torch

import decomp0_max_train_ref as d0m
from util import present_words

MAX_DRAWS = 20
MAX_SCORE = 64.0      # the largest |score| of a case: softmax and the CRF's forward-backward stay well inside float32


def default_trans(K, rng):
    tr = rng.uniform(-0.5, 0.5, size=(K, K)).astype(np.float32)
    tr[:, K - 2] = -10000.0
    tr[K - 1, :] = -10000.0
    return tr


def distinct_x(n, B, L):
    """[B, L] tokens with exactly n distinct words 0, 3, 6, .. at the valid positions (all lengths L)"""
    return (np.arange(B * L) % n * 3).reshape(B, L)


# name -> keywords of make_case
CASES = {
    'S1': dict(S=1, R=3, Q=3, K=2, B=1, L=3, lengths=[3]),
    'S2': dict(S=2, R=5, Q=4, K=3, B=3, L=4, lengths=[4, 1, 3]),
    'S63': dict(S=63, R=15, Q=5, K=5, B=2, L=3, lengths=[3, 2], nl='relu'),
    'S64': dict(S=64, R=16, Q=3, K=5, B=2, L=3, lengths=[3, 2], nl='relu'),
    'S65': dict(S=65, R=17, Q=4, K=5, B=3, L=3, lengths=[3, 0, 2], nl='relu'),
    'S192': dict(S=192, R=65, Q=15, K=5, B=2, L=3, lengths=[3, 2], nl='relu'),
    'RQ-16-17': dict(S=9, R=16, Q=17, K=16, B=3, L=6, lengths=[6, 5, 1]),
    'RQ-4-16': dict(S=7, R=4, Q=16, K=5, B=5, L=4, lengths=[4, 0, 1, 4, 2]),
    'crf-K4': dict(S=7, K=4, crf=True),
    'B1': dict(S=7, B=1, L=6, lengths=[6]),
    'len-0-1-L': dict(S=9, B=5, L=6, lengths=[0, 1, 6, 3, 0], farnn=2),
    'V-far': dict(S=7, V=400, B=3, L=5, lengths=[5, 2, 4], x=np.array([[390, 2, 390, 117, 2], [2, 117, 0, 0, 0], [390, 390, 2, 117, 0]])),
    'words15': dict(S=7, V=60, B=3, L=5, lengths=[5, 5, 5], x=distinct_x(15, 3, 5)),
    'words16': dict(S=7, V=60, B=4, L=4, lengths=[4, 4, 4, 4], x=distinct_x(16, 4, 4)),
    'words17': dict(S=7, V=60, B=3, L=6, lengths=[6, 6, 6], x=distinct_x(17, 3, 6), farnn=1),
    'words33': dict(S=7, V=100, B=9, L=4, lengths=[4] * 9, x=distinct_x(33, 9, 4), nl='relutanh'),
    'one-word': dict(S=7, V=5, B=4, L=5, lengths=[5, 5, 5, 5], x=np.full((4, 5), 3)),
}
for _f in (0, 1, 2):
    for _crf in (False, True):
        for _pri in (False, True):
            CASES['farnn{}-{}{}'.format(_f, 'crf' if _crf else 'ce1', '-pri' if _pri else '')] = dict(
                S=9, K=6 if _crf else 5, farnn=_f, crf=_crf, priority=_pri, nl=('tanh', 'relutanh', 'none')[_f])
# repeats: a ragged batch where words repeat across sequences and chains
REPEAT = dict(S=9, V=8, B=7, L=9, lengths=[9, 1, 4, 9, 0, 7, 3])


def seed_of(name):
    return 7000 + 100 * sorted(list(CASES) + ['repeat', 'repeat-gated', 'repeat-crf']).index(name)


def make_case(seed, V=12, S=7, R=6, Q=4, K=5, B=4, L=6, nl='tanh', farnn=0, crf=False, priority=False, lengths=None, x=None,
              draws=MAX_DRAWS):
    """(case, draws taken).  Raises AssertionError when no draw of `draws` serves."""
    for draw in range(draws):
        rng = np.random.RandomState(seed + draw)
        p = d0m.signed_base(V, S, R, Q, K, rng, farnn=farnn)
        xs = rng.randint(0, V, size=(B, L)).astype(np.int64) if x is None else np.asarray(x, np.int64)
        ln = np.asarray(lengths if lengths is not None else [L, 1] + list(rng.randint(1, L + 1, size=max(0, B - 2))), np.int64)[:B]
        lab = rng.randint(0, K - (2 if crf else 0), size=(B, L)).astype(np.int64)
        P = None
        if priority:
            P = (np.eye(K) + rng.choice([0.0, 0.25, -0.25], size=(K, K), p=[0.7, 0.15, 0.15])).astype(np.float32)
        kw = dict(p=p, P=P, x=xs, lengths=ln, nl=nl, farnn=farnn, k=5.0, trans=default_trans(K, rng) if crf else None)
        # powers of two (exact) on the label factors bring the largest score towards [4, 8), where many columns lie well apart.
        # The label factors feed the chains through Rtab and W, so the scaling is not homogeneous: a few rounds, and a draw whose
        # scores still run away (the CRF's exponentials then leave float32) is drawn again
        def top_score():
            with torch.no_grad():
                return float(d0m.forward(d0m._params(p, torch.float64), None if P is None else d0m._t(P, torch.float64), xs, ln,
                                         nl=nl, farnn=farnn, k=5.0)[0].abs().max())
        for _ in range(4 if nl in ('tanh', 'relutanh') else 1):      # (a bounded nl settles; an unbounded one would overshoot)
            top = top_score()
            if top <= 0 or 4.0 <= top < 8.0:
                break
            for n in ('C_embed', 'C_wildcard'):
                p[n] = p[n] * np.float32(2.0 ** (2 - np.floor(np.log2(top))))
        if not 1.0 <= top_score() < MAX_SCORE:
            continue
        try:
            d0m.check_gap(**kw)
        except d0m.GapError:
            continue
        l32, g32, pr32 = d0m.step(dtype=torch.float32, labels=lab, **kw)
        l64, g64, pr64 = d0m.step(dtype=torch.float64, labels=lab, **kw)
        present = present_words(xs, ln, V)
        if d0m.badly_drawn(g32, g64, present) or not np.array_equal(pr32, pr64):
            continue
        return dict(kw, labels=lab, l32=l32, l64=l64, g32=g32, g64=g64, pred=pr64, present=present), draw + 1
    raise AssertionError('no well-drawn case in {} draws'.format(draws))


_cache = {}


def get_case(name):
    """the case of that name, drawn once per process and left unchanged"""
    if name not in _cache:
        kw = {'repeat': REPEAT, 'repeat-gated': dict(REPEAT, farnn=2), 'repeat-crf': dict(REPEAT, crf=True, K=6, priority=True)}.get(name)
        _cache[name] = make_case(seed_of(name), **(CASES[name] if kw is None else kw))
    return _cache[name]


ALL_NAMES = sorted(list(CASES) + ['repeat', 'repeat-gated', 'repeat-crf'])
