"""Float64 numpy restatement of the order-N CP-ALS the library runs (include/farnn.h, farnn_cp_*_n), the
yardstick of test_cp4_als_cpu.py and test_gpu_cp4_als.py: `parafac` as the reference's tensor4_to_factors calls it (init='random',
normalize_factors=False, no weights, tol 1e-6).

    init    rng = RandomState(random_state); rng.random_sample((dim_n, rank)) in mode order 0 .. N-1
    sweep   for n = 0 .. N-1:  H = hadamard of the OTHER modes' Grams;  M = X_(n) khatri_rao(the others, ascending);
                               A_n = solve(H^T, M^T)^T
    error   sqrt(| ||X||^2 + sum(G0 o .. o G_{N-1}) - 2 sum(M o A_{N-1}) |) / ||X||, M the last mode's
    stop    from the second sweep on: |rec_errors[-2] - rec_errors[-1]| < tol, or n_iter_max

The same two forms as cp_als_ref.py: 'coo' works on the nonzeros in list order (np.add.at), 'dense' unfolds the dense tensor
against the Khatri-Rao product with every index range reversed -- a second summation order.  `mutant` plants one fault (MUTANTS);
the comparators must reject every one of them (test_cp4_als_cpu.py).  compare_solve, compare_run, _ratio and SPREAD_MAX are
cp_als_ref's own."""
import json
import os

import numpy as np

from cp_als_ref import SPREAD_MAX, U, _ratio, compare_run, compare_solve, gram, solve_stage  # noqa: F401  (shared, not copied)

MUTANTS = ('kr_drop', 'gram_all', 'gram_two', 'no_transpose', 'err_mode0', 'err_mode2', 'stop_early', 'init_order')
SEEDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cp4_als_seeds.json')
LETTERS = 'ijkl'


def others(order, mode):
    return [m for m in range(order) if m != mode]


def init_factors(dims, rank, random_state, mutant=None):
    rng = np.random.RandomState(random_state)
    order = range(len(dims))
    f = [None] * len(dims)
    for m in (reversed(order) if mutant == 'init_order' else order):
        f[m] = rng.random_sample((dims[m], rank))
    return f


def coo_of(dense):
    idx = np.nonzero(dense)
    return [np.asarray(i, np.int32) for i in idx], np.asarray(dense[idx], np.float64)


def dense_of(dims, idx, val):
    X = np.zeros(dims)
    np.add.at(X, tuple(idx), val)
    return X


def _terms(idx, val, factors, mode, mutant=None):
    """val * Fa[ia] * Fb[ib] (* Fc[ic]), the other modes ascending"""
    oth = others(len(factors), mode)
    if mutant == 'kr_drop' and mode == 1:
        oth = oth[:-1]                                 # one mode missing from this mode's Khatri-Rao product
    terms = val[:, None] * factors[oth[0]][idx[oth[0]]]
    for m in oth[1:]:
        terms = terms * factors[m][idx[m]]
    return terms


def mttkrp_coo(idx, val, factors, mode, dims, mutant=None):
    terms = _terms(idx, val, factors, mode, mutant)
    M = np.zeros((dims[mode], terms.shape[1]))
    np.add.at(M, idx[mode], terms)                     # unbuffered: the nonzeros in list order
    return M


def mttkrp_dense(X, factors, mode):
    oth = others(X.ndim, mode)
    R = factors[oth[0]].shape[1]
    kr = factors[oth[0]][::-1]                         # every index range reversed
    for m in oth[1:]:
        kr = (kr[:, None, :] * factors[m][None, ::-1, :]).reshape(-1, R)
    rev = (slice(None),) + (slice(None, None, -1),) * (X.ndim - 1)
    unf = np.moveaxis(X, mode, 0)[rev].reshape(X.shape[mode], -1)
    return unf @ kr


def normal_matrix(factors, mode, mutant=None):
    oth = others(len(factors), mode)
    if mutant == 'gram_two':
        oth = oth[:-1]                                 # only two of the three Grams
    H = gram(factors[oth[0]])
    for m in oth[1:]:
        H = H * gram(factors[m])
    if mutant == 'gram_all':
        H = H * gram(factors[mode])
    return H


def als(dims, idx, val, rank, init, n_iter_max, tol=1e-6, form='coo', mutant=None):
    """Returns (factors, rec_errors).  `init`: the initial factors, one per mode (not modified)."""
    N = len(dims)
    f = [np.array(a, dtype=np.float64) for a in init]
    X = dense_of(dims, idx, val) if form == 'dense' else None
    if form == 'coo':                                  # repeated coordinates add: the norm is the summed tensor's
        _, inv = np.unique(np.stack([np.asarray(i, np.int64) for i in idx], axis=1), axis=0, return_inverse=True)
        inv = np.asarray(inv).reshape(-1)
        merged = np.zeros(inv.max() + 1)
        np.add.at(merged, inv, val)
        normx2 = float(np.sum(merged * merged))
    else:
        normx2 = float(np.sum(X[(slice(None, None, -1),) * N] ** 2))
    errs = []
    for it in range(n_iter_max):
        before = [a.copy() for a in f]
        Ms = []
        for n in range(N):
            H = normal_matrix(f, n, mutant)
            M = mttkrp_coo(idx, val, f, n, dims, mutant) if form == 'coo' else mttkrp_dense(X, f, n)
            f[n] = solve_stage(H, M, mutant)
            Ms.append(M)
        em = {'err_mode0': 0, 'err_mode2': N - 2}.get(mutant, N - 1)
        cross = np.sum(Ms[em] * f[em])
        g = gram(f[0])
        for m in range(1, N):
            g = g * gram(f[m])
        errs.append(float(np.sqrt(abs(normx2 + np.sum(g) - 2.0 * cross)) / np.sqrt(normx2)))
        if it >= 1 and abs(errs[-2] - errs[-1]) < tol:
            if mutant == 'stop_early':
                return before, errs[:-1]
            break
    return f, errs


def direct_error(dims, idx, val, factors):
    X = dense_of(dims, idx, val)
    L = LETTERS[:len(dims)]
    rec = np.einsum(','.join(c + 'r' for c in L) + '->' + L, *factors)
    return float(np.linalg.norm(X - rec) / np.linalg.norm(X))


# ---- comparators: each returns (worst ratio of deviation to its bar, detail); <= 1 passes ------------------------------------
def mttkrp_bar(idx, val, factors, mode, dims):
    """per element: n 2^-53 sum|terms|, n = the row's term count + order - 1 (a sum of k terms, each a product of `order` numbers:
    k - 1 additions and order - 1 roundings per product act on any one term)"""
    terms = np.abs(_terms(idx, val, factors, mode))
    S = np.zeros((dims[mode], terms.shape[1]))
    np.add.at(S, idx[mode], terms)
    n = np.bincount(idx[mode], minlength=dims[mode]).astype(np.float64) + (len(dims) - 1.0)
    return n[:, None] * U * S


def compare_mttkrp(got, idx, val, factors, mode, dims):
    ref = mttkrp_coo(idx, val, factors, mode, dims)
    bar = mttkrp_bar(idx, val, factors, mode, dims)
    return _ratio(np.abs(got - ref), bar)


def normal_bar(factors, mode):
    """H = ga gb gc, each Gram entry a sum over its factor's rows held to (rows + 2) 2^-53 sum|terms|; to first order the product's
    error is the sum of each Gram's error times the other Grams' sizes plus the product's own roundings (one per multiplication):
    (sum over the other modes of (rows + 2) + (number of Grams - 1)) 2^-53 Sa Sb Sc, with S the sums of the absolute terms"""
    oth = others(len(factors), mode)
    S = np.ones((factors[oth[0]].shape[1],) * 2)
    n = len(oth) - 1
    for m in oth:
        S = S * gram(np.abs(factors[m]))
        n += factors[m].shape[0] + 2
    return n * U * S


def compare_normal(got, factors, mode):
    return _ratio(np.abs(got - normal_matrix(factors, mode)), normal_bar(factors, mode))


def cancellation_bar(dims, rank, idx, val, factors, err):
    """cp_als_ref.cancellation_bar for N Grams and the last mode's M: the squared error carries an absolute error of about
    n 2^-53 (||X||^2 + sum|G0 o .. o G_{N-1}| + 2 sum|M o A_{N-1}|) / ||X||^2, n the longest chain of additions behind any term;
    on err itself that is the bound over 2 err (or its root, near zero)."""
    N = len(dims)
    X = dense_of(dims, idx, val)
    normx2 = float(np.sum(X * X))
    g = gram(np.abs(factors[0]))
    for m in range(1, N):
        g = g * gram(np.abs(factors[m]))
    n2 = float(np.sum(g))
    cross = float(np.sum(np.abs(mttkrp_coo(idx, np.abs(val), [np.abs(a) for a in factors], N - 1, dims)) * np.abs(factors[N - 1])))
    n = rank * rank + dims[N - 1] * rank + sum(dims) + len(val) + 8
    sq = n * U * (normx2 + n2 + 2.0 * cross) / normx2
    return sq / (2.0 * err) if err * err > sq else float(np.sqrt(sq))


# ---- the case finder ----------------------------------------------------------------------------------------------------------
def make_case(dims, nnz, rank, seed):
    """a random sparse tensor (distinct coordinates, signed non-integer values) and its initial factors"""
    rng = np.random.RandomState(seed)
    flat = rng.choice(int(np.prod(dims)), size=nnz, replace=False)
    idx = [a.astype(np.int32) for a in np.unravel_index(flat, dims)]
    val = rng.uniform(0.5, 1.5, nnz) * rng.choice([-1.0, 1.0], nnz)
    return idx, val, init_factors(dims, rank, seed)


def measure_spread(dims, idx, val, rank, init, n_iter_max, tol=1e-6, draws=4, seed=0):
    """(reference errors, spread): the largest move of the error trajectory under the dense form and under a one-ulp random-sign
    perturbation of the initial factors (`draws` of them); inf if one of these five disturbed runs stops at another sweep"""
    _, ref = als(dims, idx, val, rank, init, n_iter_max, tol)
    rng = np.random.RandomState(seed + 12345)
    runs = [als(dims, idx, val, rank, init, n_iter_max, tol, form='dense')[1]]
    for _ in range(draws):
        pert = [a + np.spacing(a) * rng.choice([-1.0, 1.0], a.shape) for a in init]
        runs.append(als(dims, idx, val, rank, pert, n_iter_max, tol)[1])
    spread = 0.0
    for r in runs:
        if len(r) != len(ref):
            return ref, np.inf
        spread = max(spread, float(np.max(np.abs(np.asarray(r) - np.asarray(ref)))))
    return ref, spread


def find_cases(shapes, tries=20):
    """for each (dims, nnz, rank, n_iter_max, tol, must_stop_early): the first seed whose spread is at most SPREAD_MAX (and, where
    asked, whose run -- and so its five disturbed runs -- stops before n_iter_max)"""
    out = []
    for dims, nnz, rank, n_iter_max, tol, early in shapes:
        for seed in range(tries):
            idx, val, init = make_case(dims, nnz, rank, seed)
            try:
                errs, spread = measure_spread(dims, idx, val, rank, init, n_iter_max, tol)
            except np.linalg.LinAlgError:
                continue
            if spread <= SPREAD_MAX and (not early or len(errs) < n_iter_max):
                out.append({'dims': list(dims), 'nnz': nnz, 'rank': rank, 'seed': seed, 'n_iter_max': n_iter_max, 'tol': tol})
                break
        else:
            raise SystemExit('no seed in {} for {}: change the case, not the cap'.format(tries, (dims, nnz, rank, tol)))
    return out


def case_of(c):
    dims = tuple(c['dims'])
    idx, val, init = make_case(dims, c['nnz'], c['rank'], c['seed'])
    return dims, idx, val, init


def load_cases():
    with open(SEEDS) as f:
        return json.load(f)


SHAPES = [((10, 4, 4, 4), 60, 3, 32, 1e-6, False), ((24, 6, 5, 5), 400, 16, 10, 1e-6, False), ((20, 5, 6, 6), 300, 17, 32, 1e-6, False),
          ((30, 6, 8, 8), 900, 30, 10, 1e-6, False),
          ((24, 6, 5, 5), 400, 16, 32, 1e-3, True)]      # a looser per-case tol: this run stops on the tolerance, at order 4

if __name__ == '__main__':
    cases = find_cases(SHAPES)
    with open(SEEDS, 'w') as f:
        json.dump(cases, f, indent=1)
    print(cases)
