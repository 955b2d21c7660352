"""The library's float64 CP-ALS (farnn_cp_*) against the numpy restatement (cp_als_ref.py), stage by stage and on whole runs.
Shapes are the smallest at which each kernel can go wrong: every rank class of the 16-wide matrix-core tiles, rows with 0, 1 and
chunk - 1 .. chunk + 1 nonzeros, factor rows around the Gram panel, right-hand-side rows around the solve tile.

Measured on an MI355X (CP_ALS_REPORT=<file> makes test_whole_runs append its figures; profiles/cp_als_error.txt is one such run):
the library's largest deviation from the restatement's rec_errors was below 1e-14 on every golden case, inside 8 x spread."""
import os

import numpy as np
import pytest
import torch

import cp_als_ref as ref
from re2nn_seq_amd import _lib, synth
from re2nn_seq_amd import main as cli
from re2nn_seq_amd.wfa import decompose_automata as da
from re2nn_seq_amd.wfa import tensor_func as tf

pytestmark = pytest.mark.gpu

RANKS = [1, 15, 16, 17, 64, 65, _lib.CP_MAX_RANK]
CHUNK, PANEL, TILE = _lib.CP_CHUNK, _lib.CP_PANEL, _lib.CP_TILE


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def ptrs(ts):
    return [None if t is None else t.data_ptr() for t in ts]


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def row_count_tensor(dims, counts, rng):
    """distinct coordinates with `counts[i]` nonzeros in row i of mode 0; signed non-integer values"""
    per = dims[1] * dims[2]
    i0, flat = [], []
    for row, n in enumerate(counts):
        assert n <= per
        i0 += [row] * n
        flat += list(rng.choice(per, size=n, replace=False))
    order = rng.permutation(len(i0))
    i0, flat = np.asarray(i0)[order], np.asarray(flat)[order]
    idx = [i0.astype(np.int32), (flat // dims[2]).astype(np.int32), (flat % dims[2]).astype(np.int32)]
    val = rng.uniform(0.5, 1.5, len(i0)) * rng.choice([-1.0, 1.0], len(i0))
    return idx, val


def lib_mttkrp(ctx, dims, f, mode, R):
    fd = [dev(a) for a in f]
    out = torch.full((dims[mode], R), np.nan, dtype=torch.float64, device='cuda')
    ctx.mttkrp(mode, R, ptrs(fd), out.data_ptr())
    return host(out)


@pytest.fixture(scope='module')
def mttkrp_tensors():
    rng = np.random.RandomState(11)
    dims = (40, 11, 7)
    counts = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 77] + list(rng.randint(0, 6, size=34))
    a = (dims,) + row_count_tensor(dims, counts, rng)
    small = (12, 5, 5)
    b = (small,) + row_count_tensor(small, list(rng.randint(0, 9, size=12)), rng)
    one = (dims,) + row_count_tensor(dims, [0, 0, 0, 77] + [0] * 36, rng)       # one row of mode 0 holds every nonzero
    return {'rows': a, 'small': b, 'one_row': one}


@pytest.mark.parametrize('R', RANKS)
def test_mttkrp_every_mode(mttkrp_tensors, R):
    rng = np.random.RandomState(R)
    for name, (dims, idx, val) in mttkrp_tensors.items():
        ctx = _lib.CpContext(dims, idx[0], idx[1], idx[2], val, R)
        f = [rng.uniform(-1, 1, (d, R)) for d in dims]
        for mode in range(3):
            got = lib_mttkrp(ctx, dims, f, mode, R)
            r, detail = ref.compare_mttkrp(got, idx, val, f, mode, dims)
            assert r <= 1, (name, mode, detail)
            empty = np.bincount(idx[mode], minlength=dims[mode]) == 0
            assert not got[empty].any()
            again = lib_mttkrp(ctx, dims, f, mode, R)
            assert np.array_equal(got, again)
        ctx.close()


def test_mttkrp_repeated_coordinates_and_integers():
    rng = np.random.RandomState(5)
    dims = (40, 11, 7)
    idx, _ = row_count_tensor(dims, [3, CHUNK + 1, 70] + [2] * 37, rng)
    idx = [np.concatenate([i, i[:50], i[:20]]) for i in idx]                       # coordinates given two and three times
    val = rng.randint(-3, 4, len(idx[0])).astype(np.float64)
    R = 17
    ctx = _lib.CpContext(dims, idx[0], idx[1], idx[2], val, R)
    X = ref.dense_of(dims, idx, val)
    assert ctx.norm2() == (float(np.sum(X * X)), len(np.unique((idx[0].astype(np.int64) * dims[1] + idx[1]) * dims[2] + idx[2])))
    f = [rng.randint(-4, 5, (d, R)).astype(np.float64) for d in dims]
    for mode in range(3):
        assert np.array_equal(lib_mttkrp(ctx, dims, f, mode, R), ref.mttkrp_coo(idx, val, f, mode, dims)), mode    # small integers: exact
    g = [rng.uniform(-1, 1, (d, R)) for d in dims]
    for mode in range(3):
        r, detail = ref.compare_mttkrp(lib_mttkrp(ctx, dims, g, mode, R), idx, val, g, mode, dims)
        assert r <= 1, (mode, detail)
    ctx.close()


@pytest.mark.parametrize('R', RANKS)
def test_normal_matrix(R):
    rng = np.random.RandomState(100 + R)
    for rows in (1, PANEL - 1, PANEL, PANEL + 1, 3 * PANEL - 24):
        dims = (rows, 5, 3)
        ctx = _lib.CpContext(dims, [0], [0], [0], [1.0], R)
        for ints in (True, False):
            f = [rng.randint(-3, 4, (d, R)).astype(np.float64) if ints else rng.uniform(-1, 1, (d, R)) for d in dims]
            fd = [dev(a) for a in f]
            for mode in (2, 1, 0):
                H = torch.full((R, R), np.nan, dtype=torch.float64, device='cuda')
                ctx.normal_matrix(mode, R, ptrs(fd), H.data_ptr())
                got = host(H)
                assert np.array_equal(got, got.T), (rows, mode)
                if ints:                                         # exact in float64: a wrong MFMA lane map cannot hide
                    assert np.array_equal(got, ref.normal_matrix(f, mode)), (rows, mode)
                else:
                    r, detail = ref.compare_normal(got, f, mode)
                    assert r <= 1, (rows, mode, detail)
        ctx.close()


def lib_solve(ctx, H, M):
    R = H.shape[0]
    out = torch.full(M.shape, np.nan, dtype=torch.float64, device='cuda')
    Hd, Md = dev(H), dev(M)                                      # (held until the call has waited)
    ctx.solve(R, Hd.data_ptr(), Md.data_ptr(), M.shape[0], out.data_ptr())
    return host(out)


@pytest.mark.parametrize('R,ra,rb', [(1, 3, 3), (16, 12, 9), (17, 12, 9), (65, 30, 20), (_lib.CP_MAX_RANK, 64, 48)])
def test_solve_backward_error(R, ra, rb):
    rng = np.random.RandomState(R)
    A, B = rng.random_sample((ra, R)), rng.random_sample((rb, R))
    Q = rng.randn(R, R)
    systems = {'hadamard of grams': (A.T @ A) * (B.T @ B), 'well conditioned': Q @ Q.T / R + np.eye(R)}
    ctx = _lib.CpContext((4, 3, 3), [0], [0], [0], [1.0], R)
    for name, H in systems.items():
        for rows in (1, TILE - 1, TILE, TILE + 1):
            M = rng.randn(rows, R)
            r, detail = ref.compare_solve(lib_solve(ctx, H, M), H, M)
            print(name, R, rows, detail)
            assert r <= 1, (name, rows, detail)
    ctx.close()


def test_singular_normal_matrix_is_enumeric_and_the_context_survives():
    R = 17
    rng = np.random.RandomState(3)
    A, B = rng.random_sample((12, R)), rng.random_sample((9, R))
    A[:, 5] = 0.0                                                # a zero factor column: a zero row and column of H, pivot exactly 0
    H, M = (A.T @ A) * (B.T @ B), rng.randn(5, R)
    ctx = _lib.CpContext((4, 3, 3), [0], [0], [0], [1.0], R)
    with pytest.raises(np.linalg.LinAlgError, match='-33'):
        lib_solve(ctx, H, M)
    A[:, 5] = rng.random_sample(12)
    H = (A.T @ A) * (B.T @ B)
    assert ref.compare_solve(lib_solve(ctx, H, M), H, M)[0] <= 1
    ctx.close()


@pytest.mark.parametrize('dims,nnz,R', [((12, 5, 5), 60, 3), ((40, 9, 7), 500, 17), ((64, 12, 12), 900, 65)])
def test_one_sweep_stage_by_stage(dims, nnz, R):
    idx, val, f = ref.make_case(dims, nnz, R, 2)
    if R > 17:
        f = [np.random.RandomState(9 + m).random_sample((d, R)) for m, d in enumerate(dims)]
    ctx = _lib.CpContext(dims, idx[0], idx[1], idx[2], val, R)
    fd = [dev(a) for a in f]
    for n in range(3):
        now = [host(t) for t in fd]                             # the library's own inputs of this stage
        H = torch.empty((R, R), dtype=torch.float64, device='cuda')
        M = torch.empty((dims[n], R), dtype=torch.float64, device='cuda')
        ctx.normal_matrix(n, R, ptrs(fd), H.data_ptr())
        ctx.mttkrp(n, R, ptrs(fd), M.data_ptr())
        ctx.solve(R, H.data_ptr(), M.data_ptr(), dims[n], fd[n].data_ptr())
        assert ref.compare_normal(host(H), now, n)[0] <= 1
        assert ref.compare_mttkrp(host(M), idx, val, now, n, dims)[0] <= 1
        r, detail = ref.compare_solve(host(fd[n]), ref.normal_matrix(now, n), ref.mttkrp_coo(idx, val, now, n, dims))
        assert r <= 1, (n, detail)
    ctx.close()


@pytest.fixture(scope='module')
def measured():
    out = []
    for c in ref.load_cases():
        dims = tuple(c['dims'])
        idx, val, init = ref.make_case(dims, c['nnz'], c['rank'], c['seed'])
        errs, spread = ref.measure_spread(dims, idx, val, c['rank'], init, c['n_iter_max'])
        out.append((c, dims, idx, val, init, errs, spread))
    return out


def test_whole_runs(measured):
    lines = []
    for c, dims, idx, val, init, errs, spread in measured:
        R = c['rank']
        assert spread <= ref.SPREAD_MAX
        ctx = _lib.CpContext(dims, idx[0], idx[1], idx[2], val, R)
        f, got = ctx.run(R, c['n_iter_max'], 1e-4, init)
        f2, got2 = ctx.run(R, c['n_iter_max'], 1e-4, init)
        ctx.close()
        floor = ref.cancellation_bar(dims, R, idx, val, f, got[-1])
        r, detail = ref.compare_run(got, errs, spread, floor)
        direct = ref.direct_error(dims, idx, val, f)
        lines.append('dims {} R {} sweeps {} / {}  spread {:.3e}  floor {:.3e}  {}  |last - direct| {:.3e}'.format(
            dims, R, len(got), len(errs), spread, floor, detail, abs(direct - got[-1])))
        print(lines[-1])
        if os.environ.get('CP_ALS_REPORT'):
            with open(os.environ['CP_ALS_REPORT'], 'a') as fh:
                fh.write(lines[-1] + '\n')
        assert r <= 1, detail
        assert abs(direct - got[-1]) <= floor
        assert all(b <= a + floor for a, b in zip(got, got[1:]))
        assert got == got2 and all(np.array_equal(a, b) for a, b in zip(f, f2))          # bit-identical repeats on one context


def test_two_ranks_through_one_context_equal_fresh_contexts(measured):
    c, dims, idx, val, init, errs, spread = measured[2]
    runs = {}
    for R in (17, 5):
        start = ref.init_factors(dims, R, 1)
        ctx = _lib.CpContext(dims, idx[0], idx[1], idx[2], val, R)
        runs[R] = (start, ctx.run(R, 6, 1e-4, start))
        ctx.close()
    ctx = _lib.CpContext(dims, idx[0], idx[1], idx[2], val, 17)
    for R in (17, 5):
        f, e = ctx.run(R, 6, 1e-4, runs[R][0])
        assert e == runs[R][1][1] and all(np.array_equal(a, b) for a, b in zip(f, runs[R][1][0]))
    ctx.close()


def test_rank_limits():
    dims = (64, 30, 30)
    cap = _lib.CP_MAX_RANK
    idx, val, init = ref.make_case(dims, 2000, cap, 0)
    ctx = _lib.CpContext(dims, idx[0], idx[1], idx[2], val, cap + 40)
    small = _lib.CpContext(dims, idx[0], idx[1], idx[2], val, 8)
    out = torch.full((dims[0], cap + 1), 7.0, dtype=torch.float64, device='cuda')
    fd = [dev(np.ones((d, cap + 1))) for d in dims]
    for c, R in ((ctx, cap + 1), (small, 9)):
        for call in (lambda: c.mttkrp(0, R, ptrs(fd), out.data_ptr()), lambda: c.normal_matrix(0, R, ptrs(fd), out.data_ptr()),
                     lambda: c.solve(R, out.data_ptr(), out.data_ptr(), 1, out.data_ptr()),
                     lambda: c.run(R, 2, 1e-4, [np.ones((d, R)) for d in dims])):
            with pytest.raises(_lib.FarnnError) as e:
                call()
            assert e.value.code == _lib.ERANGE
    assert bool((host(out) == 7.0).all())                       # nothing was launched
    with pytest.raises(_lib.FarnnError) as e:
        _lib.CpContext(dims, [], [], [], [], 4)
    assert e.value.code == _lib.EINVAL
    with pytest.raises(_lib.FarnnError) as e:
        _lib.CpContext(dims, [0], [30], [0], [1.0], 4)             # a coordinate outside its dimension
    assert e.value.code == _lib.EINVAL
    f, errs = ctx.run(cap, 2, 1e-4, init)                        # the largest accepted rank runs
    _, want = ref.als(dims, idx, val, cap, init, 2)
    assert len(errs) == 2 and np.allclose(errs, want, rtol=0, atol=1e-9)
    ctx.close(); small.close()


def test_mirror_on_a_dense_tensor_and_on_coordinates():
    c = ref.load_cases()[1]
    dims = tuple(c['dims'])
    idx, val, _ = ref.make_case(dims, c['nnz'], c['rank'], c['seed'])
    X = ref.dense_of(dims, idx, val)
    a = tf.tensor3_to_factors(X, c['rank'], n_iter_max=8, init='random', verbose=0, random_state=4)
    b = tf.tensor3_to_factors_coo(dims, idx[0], idx[1], idx[2], val, c['rank'], n_iter_max=8, init='random', verbose=0, random_state=4)
    _, want = ref.als(dims, idx, val, c['rank'], ref.init_factors(dims, c['rank'], 4), 8)
    assert a[3] == b[3] and all(np.array_equal(p, q) for p, q in zip(a[:3], b[:3]))
    assert np.allclose(a[3], want, rtol=0, atol=1e-9) and a[0].shape == (dims[0], c['rank'])


def test_end_to_end_decompose_then_tag(tmp_path):
    tree = synth.write_dataset_tree(str(tmp_path / 'data'))
    path = da.main(['--dataset', 'ATIS-BIO', '--automata_path', tree['paths']['ID2'], '--independent', '2', '--ranks', '30',
                    '--k_best', '2', '--data_dir', tree['paths']['data_dir'], '--out_dir', str(tmp_path / 'out')])
    assert os.path.basename(path).startswith('IIID.automata.')
    argv = ['--dataset', 'ATIS-BIO', '--method', 'decompose', '--independent', '2', '--automata_path', path, '--rank', '30',
            '--seed', '3', '--beta', '1.0', '--embed_dim', '16', '--normalize_automata', 'none', '--rand_constant', '0',
            '--update_nonlinear', 'none', '--bz', '9', '--seq_max_len', '12', '--epoch', '0', '--train_portion', '0',
            '--data_dir', tree['paths']['data_dir'], '--model_dir', str(tmp_path)]
    results, stats, _ = cli.main(argv)
    assert stats['test']['tokens'] > 0 and len(results['test']['token-level']) >= 4
    # the error the file name records for the last outer seed (3; restarts at rands 3 and 11), rounded to 4 digits there
    recorded = float(os.path.basename(path).split('.1splits.30-')[1].split('..pkl')[0])
    from re2nn_seq_amd.wfa.fsa_to_tensor import dfa_to_tensor_slot_single_wildcard
    T, _, _, _, _, _, _, language = dfa_to_tensor_slot_single_wildcard(tree['automaton'], tree['dset']['t2i'], tree['dset']['s2i'],
                                                                       dataset='ATIS-BIO')
    X = T[np.array([tree['dset']['t2i'][w] for w in language])]
    idx, val = ref.coo_of(X)
    best, bar = np.inf, 0.0
    for r in (3, 11):
        init = ref.init_factors(X.shape, 30, r)
        errs, spread = ref.measure_spread(X.shape, idx, val, 30, init, 32)
        f, _ = ref.als(X.shape, idx, val, 30, init, 32)
        best = min(best, errs[-1])
        bar = max(bar, 8 * spread, ref.cancellation_bar(X.shape, 30, idx, val, f, errs[-1]))
    print('recorded', recorded, 'restatement', best, 'bar', bar)
    assert recorded <= best + bar + 5e-5
