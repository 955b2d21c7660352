"""Float64 numpy restatement of the CP-ALS the library runs (include/farnn.h, farnn_cp_*), the yardstick of
test_cp_als_cpu.py and test_gpu_cp_als.py: `parafac` as the reference's wfa/tensor_func.py calls it (init='random',
normalize_factors=False, no weights, tol 1e-4).

    init    rng = RandomState(random_state); rng.random_sample((dim_n, rank)) in mode order 0, 1, 2
    sweep   for n = 0, 1, 2:  H = hadamard of the two other Grams;  M = X_(n) khatri_rao(the two others);
                              A_n = solve(H^T, M^T)^T
    error   sqrt(| ||X||^2 + sum(G0 o G1 o G2) - 2 sum(M o A_2) |) / ||X||, M the last mode's
    stop    from the second sweep on: |rec_errors[-2] - rec_errors[-1]| < tol, or n_iter_max

Two forms: 'coo' works on the nonzeros in their natural order, 'dense' unfolds the dense tensor against the Khatri-Rao
product with the rows and the nonzeros taken in reverse -- a second summation order.  `mutant` plants one fault (MUTANTS);
the comparators below, the ones the GPU tests use, must reject every one of them (test_cp_als_cpu.py)."""
import json
import os

import numpy as np

U = 2.0 ** -53
OTHER = {0: (1, 2), 1: (0, 2), 2: (0, 1)}
MUTANTS = ('kr_pair', 'gram_all', 'no_transpose', 'err_mode0', 'stop_early', 'init_order')
SEEDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cp_als_seeds.json')
SPREAD_MAX = 1e-9


def init_factors(dims, rank, random_state, mutant=None):
    rng = np.random.RandomState(random_state)
    order = (2, 1, 0) if mutant == 'init_order' else (0, 1, 2)
    f = [None] * 3
    for m in order:
        f[m] = rng.random_sample((dims[m], rank))
    return f


def coo_of(dense):
    idx = np.nonzero(dense)
    return [np.asarray(i, np.int32) for i in idx], np.asarray(dense[idx], np.float64)


def dense_of(dims, idx, val):
    X = np.zeros(dims)
    np.add.at(X, tuple(idx), val)
    return X


def mttkrp_coo(idx, val, factors, mode, dims, mutant=None):
    a, b = OTHER[mode]
    if mutant == 'kr_pair' and mode == 1:
        a, b = 0, 1
    terms = val[:, None] * factors[a][idx[a]] * factors[b][idx[b]]
    M = np.zeros((dims[mode], factors[a].shape[1]))
    np.add.at(M, idx[mode], terms)                     # unbuffered: the nonzeros in list order
    return M


def mttkrp_dense(X, factors, mode):
    a, b = OTHER[mode]
    R = factors[a].shape[1]
    kr = (factors[a][::-1, None, :] * factors[b][None, ::-1, :]).reshape(-1, R)       # both index ranges reversed
    unf = np.moveaxis(X, mode, 0)[:, ::-1, ::-1].reshape(X.shape[mode], -1)
    return unf @ kr


def gram(F):
    return F.T @ F


def normal_matrix(factors, mode, mutant=None):
    a, b = OTHER[mode]
    H = gram(factors[a]) * gram(factors[b])
    if mutant == 'gram_all':
        H = H * gram(factors[mode])
    return H


def solve_stage(H, M, mutant=None):
    return np.linalg.solve(H if mutant == 'no_transpose' else H.T, M.T).T


def als(dims, idx, val, rank, init, n_iter_max, tol=1e-4, form='coo', mutant=None):
    """Returns (factors, rec_errors).  `init`: the three initial factors (not modified)."""
    f = [np.array(a, dtype=np.float64) for a in init]
    X = dense_of(dims, idx, val) if form == 'dense' else None
    if form == 'coo':                                  # repeated coordinates add: the norm is the summed tensor's
        key = (idx[0].astype(np.int64) * dims[1] + idx[1]) * dims[2] + idx[2]
        _, inv = np.unique(key, return_inverse=True)
        merged = np.zeros(inv.max() + 1)
        np.add.at(merged, inv, val)
        normx2 = float(np.sum(merged * merged))
    else:
        normx2 = float(np.sum(X[::-1, ::-1, ::-1] ** 2))
    errs = []
    for it in range(n_iter_max):
        before = [a.copy() for a in f]
        M0 = None
        for n in range(3):
            H = normal_matrix(f, n, mutant)
            M = mttkrp_coo(idx, val, f, n, dims, mutant) if form == 'coo' else mttkrp_dense(X, f, n)
            f[n] = solve_stage(H, M, mutant)
            if n == 0:
                M0 = M
        cross = np.sum(M0 * f[0]) if mutant == 'err_mode0' else np.sum(M * f[2])
        n2 = np.sum(gram(f[0]) * gram(f[1]) * gram(f[2]))
        errs.append(float(np.sqrt(abs(normx2 + n2 - 2.0 * cross)) / np.sqrt(normx2)))
        if it >= 1 and abs(errs[-2] - errs[-1]) < tol:
            if mutant == 'stop_early':
                return before, errs[:-1]
            break
    return f, errs


def direct_error(dims, idx, val, factors):
    X = dense_of(dims, idx, val)
    rec = np.einsum('ir,jr,kr->ijk', *factors)
    return float(np.linalg.norm(X - rec) / np.linalg.norm(X))


# ---- comparators: each returns (worst ratio of deviation to its bar, detail); <= 1 passes ------------------------------------
def mttkrp_bar(idx, val, factors, mode, dims):
    """per element: n 2^-53 sum|terms|, n = the row's term count + 2 (a sum of k terms, each a product of three numbers: k - 1
    additions and two roundings per product act on any one term)"""
    a, b = OTHER[mode]
    terms = np.abs(val[:, None] * factors[a][idx[a]] * factors[b][idx[b]])
    S = np.zeros((dims[mode], factors[a].shape[1]))
    np.add.at(S, idx[mode], terms)
    n = np.bincount(idx[mode], minlength=dims[mode]).astype(np.float64) + 2.0
    return n[:, None] * U * S


def compare_mttkrp(got, idx, val, factors, mode, dims):
    ref = mttkrp_coo(idx, val, factors, mode, dims)
    bar = mttkrp_bar(idx, val, factors, mode, dims)
    return _ratio(np.abs(got - ref), bar)


def normal_bar(factors, mode):
    """H = ga gb, each Gram entry a sum over its factor's rows held to (rows + 2) 2^-53 sum|terms| like the MTTKRP's; to first
    order the product's error is ea |gb| + eb |ga| plus one rounding of the product: ((ra + 2) + (rb + 2) + 1) 2^-53 Sa Sb with
    Sa, Sb the sums of the absolute terms"""
    a, b = OTHER[mode]
    Sa, Sb = gram(np.abs(factors[a])), gram(np.abs(factors[b]))
    n = (factors[a].shape[0] + 2) + (factors[b].shape[0] + 2) + 1
    return n * U * Sa * Sb


def compare_normal(got, factors, mode):
    return _ratio(np.abs(got - normal_matrix(factors, mode)), normal_bar(factors, mode))


def backward_error(X, H, M):
    return float(np.linalg.norm(X @ H - M) / (np.linalg.norm(X) * np.linalg.norm(H) + np.linalg.norm(M)))


def solve_bar(H, M):
    """max(4 x numpy.linalg.solve's own backward error on the system, R 2^-52: the textbook order of Cholesky's)"""
    return max(4.0 * backward_error(solve_stage(H, M), H, M), H.shape[0] * 2.0 ** -52)


def compare_solve(X, H, M):
    if not np.all(np.isfinite(X)):
        return np.inf, 'not finite'
    eta, bar = backward_error(X, H, M), solve_bar(H, M)
    return eta / bar, 'eta {:.3e} bar {:.3e}'.format(eta, bar)


def _ratio(dev, bar):
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(dev == 0, 0.0, dev / bar)
    k = np.unravel_index(np.argmax(r), r.shape)
    return float(r[k]), 'worst at {}: dev {:.3e} bar {:.3e}'.format(k, float(dev[k]), float(bar[k]))


def cancellation_bar(dims, rank, idx, val, factors, err):
    """The error formula subtracts numbers of the size of ||X||^2 + ||[[A]]||^2: its squared value carries an absolute error of
    about n 2^-53 (||X||^2 + sum|G0 o G1 o G2| + 2 sum|M o A_2|) / ||X||^2, n the longest chain of additions behind any term (the two
    outer sums and the Gram / MTTKRP sums inside them).  On err itself that is the bound over 2 err (or its root, near zero)."""
    X = dense_of(dims, idx, val)
    normx2 = float(np.sum(X * X))
    g = [gram(np.abs(a)) for a in factors]
    n2 = float(np.sum(g[0] * g[1] * g[2]))
    cross = float(np.sum(np.abs(mttkrp_coo(idx, np.abs(val), [np.abs(a) for a in factors], 2, dims)) * np.abs(factors[2])))
    n = rank * rank + dims[2] * rank + sum(dims) + len(val) + 8
    sq = n * U * (normx2 + n2 + 2.0 * cross) / normx2
    return sq / (2.0 * err) if err * err > sq else float(np.sqrt(sq))


def compare_run(got_errs, ref_errs, spread, floor, factor=8.0):
    """the same sweep count, and every rec_error within factor x the case's measured spread (not below the cancellation floor)"""
    if len(got_errs) != len(ref_errs):
        return np.inf, 'sweeps {} != {}'.format(len(got_errs), len(ref_errs))
    bar = max(factor * spread, floor)
    dev = float(np.max(np.abs(np.asarray(got_errs) - np.asarray(ref_errs))))
    return dev / bar, 'dev {:.3e} bar {:.3e} (spread {:.3e}, floor {:.3e})'.format(dev, bar, spread, floor)


# ---- the case finder ----------------------------------------------------------------------------------------------------------
def make_case(dims, nnz, rank, seed):
    """a random sparse tensor (distinct coordinates, signed non-integer values) and its initial factors"""
    rng = np.random.RandomState(seed)
    flat = rng.choice(dims[0] * dims[1] * dims[2], size=nnz, replace=False)
    idx = [a.astype(np.int32) for a in np.unravel_index(flat, dims)]
    val = rng.uniform(0.5, 1.5, nnz) * rng.choice([-1.0, 1.0], nnz)
    return idx, val, init_factors(dims, rank, seed)


def measure_spread(dims, idx, val, rank, init, n_iter_max, draws=4, seed=0):
    """(reference errors, spread): the largest move of the error trajectory under the dense form and under a one-ulp random-sign
    perturbation of the initial factors (`draws` of them); inf if a disturbance changes the sweep count"""
    _, ref = als(dims, idx, val, rank, init, n_iter_max)
    rng = np.random.RandomState(seed + 12345)
    runs = [als(dims, idx, val, rank, init, n_iter_max, form='dense')[1]]
    for _ in range(draws):
        pert = [a + np.spacing(a) * rng.choice([-1.0, 1.0], a.shape) for a in init]
        runs.append(als(dims, idx, val, rank, pert, n_iter_max)[1])
    spread = 0.0
    for r in runs:
        if len(r) != len(ref):
            return ref, np.inf
        spread = max(spread, float(np.max(np.abs(np.asarray(r) - np.asarray(ref)))))
    return ref, spread


def find_cases(shapes, n_iter_max=32, tries=20):
    """for each (dims, nnz, rank): the first seed whose spread is at most SPREAD_MAX"""
    out = []
    for dims, nnz, rank in shapes:
        for seed in range(tries):
            idx, val, init = make_case(dims, nnz, rank, seed)
            try:
                _, spread = measure_spread(dims, idx, val, rank, init, n_iter_max)
            except np.linalg.LinAlgError:
                continue
            if spread <= SPREAD_MAX:
                out.append({'dims': list(dims), 'nnz': nnz, 'rank': rank, 'seed': seed, 'n_iter_max': n_iter_max})
                break
    return out


def load_cases():
    with open(SEEDS) as f:
        return json.load(f)


if __name__ == '__main__':
    cases = find_cases([((12, 5, 5), 60, 3), ((40, 9, 9), 400, 16), ((30, 7, 7), 300, 17), ((64, 12, 12), 900, 30)])
    with open(SEEDS, 'w') as f:
        json.dump(cases, f, indent=1)
    print(cases)
