"""CP decomposition of automaton tensors: the reference's ``src_seq/wfa/tensor_func.py`` with the same names and signatures,
on the library's float64 CP-ALS (include/farnn.h, farnn_cp_*) instead of ``tensorly.parafac``.

The algorithm is `parafac` as the reference calls it -- ``normalize_factors=False``, no weights, ``tol=1e-4`` -- with
``init='random'``: ``rng = numpy.random.RandomState(random_state)``, the factors ``rng.random_sample((dim_n, rank))`` in mode
order 0, 1, 2 (, 3), drawn here on the host.  The 4-way tensor of ``D.automata`` goes the same way with ``tol=1e-6``, the
reference's (row f13).  ``init='svd'`` is not built.  That seeds
and trajectories equal tensorly's at the reference's pinned commit is NOT claimed (tensorly cannot be run here); the yardstick is
the numpy restatement under tests/.

A singular normal matrix raises ``numpy.linalg.LinAlgError`` (the callers' ``except (ValueError, LinAlgError): continue``).
There is no CPU fallback: without the library or a GPU these functions raise ``FarnnError``."""
import time

import numpy as np

from .. import _lib

TOL = 1e-4
TOL4 = 1e-6         # tensor4_to_factors (ref :22)


def _refuse_init(init):
    assert init in ['random', 'svd']
    if init != 'random':
        raise NotImplementedError("init='svd' is not built: only init='random' (DESIGN.md section 9)")


def tensor3_to_factors_coo(dims, idx0, idx1, idx2, val, rank, n_iter_max=50, init='random', verbose=10, random_state=1,
                           device=0):
    """tensor3_to_factors for a tensor given by its coordinates (repeated ones add): a SNIPS-size automaton never needs its
    dense [V', S, S] tensor.  Returns (A0, A1, A2, rec_errors)."""
    _refuse_init(init)
    dims = tuple(int(d) for d in dims)
    rng = np.random.RandomState(random_state)
    factors = [rng.random_sample((d, int(rank))) for d in dims]
    ctx = _lib.CpContext(dims, idx0, idx1, idx2, val, int(rank), device=device)
    try:
        factors, rec_errors = ctx.run(int(rank), int(n_iter_max), TOL, factors)
    finally:
        ctx.close()
    if verbose:
        print('reconstruction error={} after {} sweeps'.format(rec_errors[-1], len(rec_errors)))
    return factors[0], factors[1], factors[2], rec_errors


def tensor3_to_factors(tensor, rank, n_iter_max=50, init='svd', verbose=10, random_state=1):
    """ref :7-13.  A dense numpy tensor in; its nonzeros are extracted on the host."""
    _refuse_init(init)
    tensor = np.asarray(tensor, dtype=np.float64)
    if tensor.ndim != 3:
        raise ValueError('tensor3_to_factors takes a 3-way tensor, got shape {}'.format(tensor.shape))
    idx = np.nonzero(tensor)
    return tensor3_to_factors_coo(tensor.shape, idx[0], idx[1], idx[2], tensor[idx], rank, n_iter_max=n_iter_max, init=init,
                                  verbose=verbose, random_state=random_state)


def tensor4_to_factors_coo(dims, idx, val, rank, n_iter_max=60, init='random', verbose=10, random_state=1, device=0):
    """tensor4_to_factors for a tensor given by its four coordinate arrays `idx` (repeated ones add): an ATIS-size automaton
    never needs its dense [V', C, S, S] tensor.  Returns (A0, A1, A2, A3, rec_errors)."""
    _refuse_init(init)
    dims = tuple(int(d) for d in dims)
    if len(dims) != 4 or len(idx) != 4:
        raise ValueError('tensor4_to_factors_coo takes four dimensions and four index arrays')
    rng = np.random.RandomState(random_state)
    factors = [rng.random_sample((d, int(rank))) for d in dims]
    ctx = _lib.CpContext.from_coo(dims, idx, val, int(rank), device=device)
    try:
        factors, rec_errors = ctx.run(int(rank), int(n_iter_max), TOL4, factors)
    finally:
        ctx.close()
    if verbose:
        print('reconstruction error={} after {} sweeps'.format(rec_errors[-1], len(rec_errors)))
    if rec_errors[-1] < 0:
        raise ValueError
    return factors[0], factors[1], factors[2], factors[3], rec_errors


def tensor4_to_factors(tensor, rank, n_iter_max=60, init='svd', verbose=10, random_state=1):
    """ref :16-27.  A dense numpy tensor in; its nonzeros are extracted on the host.  tol is 1e-6, as the reference's."""
    _refuse_init(init)
    tensor = np.asarray(tensor, dtype=np.float64)
    if tensor.ndim != 4:
        raise ValueError('tensor4_to_factors takes a 4-way tensor, got shape {}'.format(tensor.shape))
    idx = np.nonzero(tensor)
    return tensor4_to_factors_coo(tensor.shape, idx, tensor[idx], rank, n_iter_max=n_iter_max, init=init, verbose=verbose,
                                  random_state=random_state)


def recover_tensor_from_factors(factors):
    """ref :30-33 (tl.cp_to_tensor): `factors` is (weights or None, [A0, A1, ...]) or the list of factor matrices itself"""
    weights = None
    if isinstance(factors, tuple) and len(factors) == 2 and isinstance(factors[1], (list, tuple)):
        weights, factors = factors
    factors = [np.asarray(a, dtype=np.float64) for a in factors]
    rank = factors[0].shape[1]
    w = np.ones(rank) if weights is None else np.asarray(weights, dtype=np.float64)
    letters = 'ijkl'[:len(factors)]
    return np.einsum(','.join(c + 'r' for c in letters) + ',r->' + letters, *factors, w)


def decompose_tensor_split_slot_4d(language_tensor, language, word2idx, rank, random_state=1, n_iter_max=20, init='svd',
                                   verbose=10):
    """ref :37-61: the tensor is squashed to the rows of the `language` words; the other words' rows of V_embed_split are zero"""
    language_tensor_squashed = language_tensor[np.array([word2idx[i] for i in language])]
    print('SQUASHED TENSOR SIZE: {}'.format(language_tensor_squashed.shape))
    time_start = time.time()
    V_embed, C_embed, S1, S2, rec_error = tensor4_to_factors(language_tensor_squashed, rank=rank, n_iter_max=n_iter_max,
                                                             verbose=verbose, random_state=random_state, init=init)
    time_end = time.time()
    print('time cost', time_end - time_start, 's')
    vocab, labels, state, _ = language_tensor.shape
    V_embed_split = np.zeros((vocab, rank))
    for i in range(len(language)):
        idx = word2idx[language[i]]
        V_embed_split[idx] = V_embed[i]
    return V_embed_split, C_embed, S1, S2, rec_error


def decompose_tensor_split_slot_4d_edges(word, label, frm, to, dims, language, word2idx, rank, random_state=1, n_iter_max=20,
                                         init='svd', verbose=10):
    """decompose_tensor_split_slot_4d on the coordinates fsa_to_tensor.dfa_to_edges_slot_new gives (`word`, `label`, `frm`, `to`:
    the distinct nonzeros of language_tensor, all of value 1; `dims` = its shape [V, C, S, S]): the dense tensor is never built.
    Same squash, prints and returns."""
    vocab, labels, state, _ = (int(d) for d in dims)
    row_of = np.full(vocab, -1, dtype=np.int64)
    row_of[np.array([word2idx[w] for w in language], dtype=np.int64)] = np.arange(len(language))
    rows = row_of[np.asarray(word, dtype=np.int64)]
    if rows.size and rows.min() < 0:
        raise ValueError('an edge carries a word outside `language`')
    squashed = (len(language), labels, state, state)
    label, frm, to = (np.asarray(a, dtype=np.int32) for a in (label, frm, to))
    order = np.lexsort((to, frm, label, rows))          # the order numpy.nonzero gives the dense entry: both make the same call
    rows, label, frm, to = rows[order].astype(np.int32), label[order], frm[order], to[order]
    print('SQUASHED TENSOR SIZE: {}'.format(squashed))
    time_start = time.time()
    V_embed, C_embed, S1, S2, rec_error = tensor4_to_factors_coo(squashed, [rows, label, frm, to], np.ones(len(rows)), rank=rank,
                                                                 n_iter_max=n_iter_max, verbose=verbose,
                                                                 random_state=random_state, init=init)
    time_end = time.time()
    print('time cost', time_end - time_start, 's')
    V_embed_split = np.zeros((vocab, rank))
    for i in range(len(language)):
        V_embed_split[word2idx[language[i]]] = V_embed[i]
    return V_embed_split, C_embed, S1, S2, rec_error


def decompose_tensor_split_slot_3d(the_tensor, rank, random_state=1, n_iter_max=20, init='svd', verbose=10):
    """ref :64-76"""
    print('SQUASHED TENSOR SIZE: {}'.format(the_tensor.shape))
    time_start = time.time()
    C_embed, S1, S2, rec_error = tensor3_to_factors(the_tensor, rank=rank, n_iter_max=n_iter_max, verbose=verbose,
                                                    random_state=random_state, init=init)
    time_end = time.time()
    print('time cost', time_end - time_start, 's')
    return C_embed, S1, S2, rec_error


def decompose_tensor_split_slot_3d_language(language_tensor, language, word2idx, rank, random_state=1, n_iter_max=20, init='svd',
                                            verbose=10):
    """ref :79-101: the tensor is squashed to the rows of the `language` words; the other words' rows of V_embed_split are zero"""
    language_tensor_squashed = language_tensor[np.array([word2idx[i] for i in language])]
    print('SQUASHED TENSOR SIZE: {}'.format(language_tensor_squashed.shape))
    time_start = time.time()
    V_embed, S1, S2, rec_error = tensor3_to_factors(language_tensor_squashed, rank=rank, n_iter_max=n_iter_max, verbose=verbose,
                                                    random_state=random_state, init=init)
    time_end = time.time()
    print('time cost', time_end - time_start, 's')
    vocab, _, state = language_tensor.shape
    V_embed_split = np.zeros((vocab, rank))
    for i in range(len(language)):
        idx = word2idx[language[i]]
        V_embed_split[idx] = V_embed[i]
    return V_embed_split, S1, S2, rec_error
