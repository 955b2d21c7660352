"""The library's float64 CP-ALS of order 4 (farnn_cp_*_n) against the numpy restatement (cp4_als_ref.py), stage by
stage and on whole runs, and the D.automata writer on it end to end.  Shapes are the smallest at which each kernel can go wrong:
every rank class of the 16-wide matrix-core tiles, rows with 0, 1 and chunk - 1 .. chunk + 1 nonzeros in mode 0, one row that owns
every nonzero (in mode 0 and in mode 3, the automaton's "state 0 owns the edges"), factor rows around the Gram panel.

CP_ALS_REPORT=<file> makes test_whole_runs append its figures; profiles/cp4_als_error.txt is one such run on an MI355X."""
import os

import numpy as np
import pytest
import torch

import cp4_als_ref as ref
import cp_als_ref as ref3
from re2nn_seq_amd import _lib, synth
from re2nn_seq_amd import main as cli
from re2nn_seq_amd.wfa import decompose_automata as da
from re2nn_seq_amd.wfa import fsa_to_tensor as f2t
from re2nn_seq_amd.wfa import tensor_func as tf

pytestmark = pytest.mark.gpu

RANKS = [1, 15, 16, 17, 64, 65, _lib.CP_MAX_RANK]
CHUNK, PANEL = _lib.CP_CHUNK, _lib.CP_PANEL


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def ptrs(ts):
    return [None if t is None else t.data_ptr() for t in ts]


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def row_count_tensor(dims, counts, rng, mode=0):
    """distinct coordinates with `counts[i]` nonzeros in row i of `mode`; signed non-integer values"""
    oth = [m for m in range(len(dims)) if m != mode]
    odims = tuple(dims[m] for m in oth)
    per = int(np.prod(odims))
    rows, flat = [], []
    for row, n in enumerate(counts):
        assert n <= per
        rows += [row] * n
        flat += list(rng.choice(per, size=n, replace=False))
    order = rng.permutation(len(rows))
    rows, flat = np.asarray(rows)[order], np.asarray(flat)[order]
    idx = [None] * len(dims)
    idx[mode] = rows.astype(np.int32)
    for m, a in zip(oth, np.unravel_index(flat, odims)):
        idx[m] = a.astype(np.int32)
    val = rng.uniform(0.5, 1.5, len(rows)) * rng.choice([-1.0, 1.0], len(rows))
    return idx, val


def lib_mttkrp(ctx, dims, f, mode, R):
    fd = [dev(a) for a in f]
    out = torch.full((dims[mode], R), np.nan, dtype=torch.float64, device='cuda')
    ctx.mttkrp(mode, R, ptrs(fd), out.data_ptr())
    return host(out)


@pytest.fixture(scope='module')
def mttkrp_tensors():
    rng = np.random.RandomState(11)
    dims = (40, 6, 5, 5)
    counts = [0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 77] + list(rng.randint(0, 6, size=34))
    a = (dims,) + row_count_tensor(dims, counts, rng)
    one0 = (dims,) + row_count_tensor(dims, [0, 0, 0, 77] + [0] * 36, rng)              # one row of mode 0 holds every nonzero
    one3 = (dims,) + row_count_tensor(dims, [0, 0, 3 * CHUNK + 8, 0, 0], rng, mode=3)   # one row of mode 3 does: a row of 4 chunks
    small = (12, 3, 4, 4)
    b = (small,) + row_count_tensor(small, list(rng.randint(0, 9, size=12)), rng)
    return {'rows': a, 'one_row_mode0': one0, 'one_row_mode3': one3, 'small': b}


@pytest.mark.parametrize('R', RANKS)
def test_mttkrp_every_mode(mttkrp_tensors, R):
    rng = np.random.RandomState(R)
    for name, (dims, idx, val) in mttkrp_tensors.items():
        ctx = _lib.CpContext.from_coo(dims, idx, val, R)
        assert ctx.order == 4
        f = [rng.uniform(-1, 1, (d, R)) for d in dims]
        for mode in range(4):
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
    dims = (40, 6, 5, 5)
    idx, _ = row_count_tensor(dims, [3, CHUNK + 1, 70] + [2] * 37, rng)
    idx = [np.concatenate([i, i[:50], i[:20]]) for i in idx]                       # coordinates given two and three times
    val = rng.randint(-3, 4, len(idx[0])).astype(np.float64)
    R = 17
    ctx = _lib.CpContext.from_coo(dims, idx, val, R)
    X = ref.dense_of(dims, idx, val)
    assert ctx.norm2() == (float(np.sum(X * X)), len(np.unique(np.stack(idx, axis=1), axis=0)))
    f = [rng.randint(-4, 5, (d, R)).astype(np.float64) for d in dims]
    for mode in range(4):
        assert np.array_equal(lib_mttkrp(ctx, dims, f, mode, R), ref.mttkrp_coo(idx, val, f, mode, dims)), mode    # small integers: exact
    g = [rng.uniform(-1, 1, (d, R)) for d in dims]
    for mode in range(4):
        r, detail = ref.compare_mttkrp(lib_mttkrp(ctx, dims, g, mode, R), idx, val, g, mode, dims)
        assert r <= 1, (mode, detail)
    ctx.close()


@pytest.mark.parametrize('R', RANKS)
def test_normal_matrix(R):
    rng = np.random.RandomState(100 + R)
    shapes = [(rows, 3, 2, 2) for rows in (1, PANEL - 1, PANEL, PANEL + 1, 3 * PANEL - 24)] + [(3, 2, 2, PANEL + 1)]
    for dims in shapes:
        ctx = _lib.CpContext.from_coo(dims, [[0]] * 4, [1.0], R)
        for ints in (True, False):
            f = [rng.randint(-3, 4, (d, R)).astype(np.float64) if ints else rng.uniform(-1, 1, (d, R)) for d in dims]
            fd = [dev(a) for a in f]
            for mode in (3, 2, 1, 0):
                H = torch.full((R, R), np.nan, dtype=torch.float64, device='cuda')
                ctx.normal_matrix(mode, R, ptrs(fd), H.data_ptr())
                got = host(H)
                assert np.array_equal(got, got.T), (dims, mode)
                if ints:                        # exact in float64: a Gram dropped from or doubled in the product cannot hide
                    assert np.array_equal(got, ref.normal_matrix(f, mode)), (dims, mode)
                else:
                    r, detail = ref.compare_normal(got, f, mode)
                    assert r <= 1, (dims, mode, detail)
        ctx.close()


@pytest.mark.parametrize('dims,nnz,R', [((10, 4, 4, 4), 60, 3), ((24, 6, 5, 5), 400, 17), ((30, 6, 8, 8), 900, 65)])
def test_one_sweep_stage_by_stage(dims, nnz, R):
    idx, val, f = ref.make_case(dims, nnz, R, 2)
    if R > 17:
        f = [np.random.RandomState(9 + m).random_sample((d, R)) for m, d in enumerate(dims)]
    ctx = _lib.CpContext.from_coo(dims, idx, val, R)
    fd = [dev(a) for a in f]
    for n in range(4):
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
        dims, idx, val, init = ref.case_of(c)
        errs, spread = ref.measure_spread(dims, idx, val, c['rank'], init, c['n_iter_max'], c['tol'])
        out.append((c, dims, idx, val, init, errs, spread))
    return out


def test_whole_runs(measured):
    lines = []
    for c, dims, idx, val, init, errs, spread in measured:
        R = c['rank']
        assert spread <= ref.SPREAD_MAX
        ctx = _lib.CpContext.from_coo(dims, idx, val, R)
        f, got = ctx.run(R, c['n_iter_max'], c['tol'], init)
        f2, got2 = ctx.run(R, c['n_iter_max'], c['tol'], init)
        ctx.close()
        floor = ref.cancellation_bar(dims, R, idx, val, f, got[-1])
        r, detail = ref.compare_run(got, errs, spread, floor)
        direct = ref.direct_error(dims, idx, val, f)
        lines.append('dims {} R {} tol {:g} sweeps {} / {}  spread {:.3e}  floor {:.3e}  {}  |last - direct| {:.3e}'.format(
            dims, R, c['tol'], len(got), len(errs), spread, floor, detail, abs(direct - got[-1])))
        print(lines[-1])
        if os.environ.get('CP_ALS_REPORT'):
            with open(os.environ['CP_ALS_REPORT'], 'a') as fh:
                fh.write(lines[-1] + '\n')
        assert r <= 1, detail
        assert abs(direct - got[-1]) <= floor
        assert all(b <= a + floor for a, b in zip(got, got[1:]))
        assert got == got2 and all(np.array_equal(a, b) for a, b in zip(f, f2))          # bit-identical repeats on one context
    assert any(len(m[5]) < m[0]['n_iter_max'] for m in measured)                         # the stop rule was exercised at order 4


def test_two_ranks_through_one_context_equal_fresh_contexts(measured):
    c, dims, idx, val, init, errs, spread = measured[2]
    runs = {}
    for R in (17, 5):
        start = ref.init_factors(dims, R, 1)
        ctx = _lib.CpContext.from_coo(dims, idx, val, R)
        runs[R] = (start, ctx.run(R, 6, 1e-6, start))
        ctx.close()
    ctx = _lib.CpContext.from_coo(dims, idx, val, 17)
    for R in (17, 5):
        f, e = ctx.run(R, 6, 1e-6, runs[R][0])
        assert e == runs[R][1][1] and all(np.array_equal(a, b) for a, b in zip(f, runs[R][1][0]))
    ctx.close()


def test_order_3_through_the_n_entries_is_bit_identical_to_the_3_way_entries():
    c = ref3.load_cases()[2]
    dims = tuple(c['dims'])
    idx, val, init = ref3.make_case(dims, c['nnz'], c['rank'], c['seed'])
    R = c['rank']
    old = _lib.CpContext(dims, idx[0], idx[1], idx[2], val, R)
    new = _lib.CpContext.from_coo(dims, idx, val, R)
    assert old.order == new.order == 3 and old.norm2() == new.norm2()
    a, b = old.run(R, 8, 1e-4, init), new.run(R, 8, 1e-4, init)
    assert a[1] == b[1] and all(np.array_equal(p, q) for p, q in zip(a[0], b[0]))
    f = [np.random.RandomState(m).uniform(-1, 1, (d, R)) for m, d in enumerate(dims)]
    fd = [dev(x) for x in f]
    for mode in range(3):
        assert np.array_equal(lib_mttkrp(old, dims, f, mode, R), lib_mttkrp(new, dims, f, mode, R))
        Ha, Hb = (torch.full((R, R), np.nan, dtype=torch.float64, device='cuda') for _ in range(2))
        old.normal_matrix(mode, R, ptrs(fd), Ha.data_ptr())
        new.normal_matrix(mode, R, ptrs(fd), Hb.data_ptr())
        assert np.array_equal(host(Ha), host(Hb))
    with pytest.raises(_lib.FarnnError) as e:                     # mode 3 of a 3-way tensor
        new.mttkrp(3, R, ptrs(fd) , Ha.data_ptr())
    assert e.value.code == _lib.EINVAL
    old.close(); new.close()


def test_refusals_leave_the_outputs_untouched():
    dims = (12, 3, 4, 4)
    idx, val, init = ref.make_case(dims, 80, 8, 0)
    cap = _lib.CP_MAX_RANK
    lib = _lib.load()
    for bad_dims, bad_idx in (((12, 3), idx[:2]), ((12, 3, 4, 4, 2), idx + [idx[0] % 2])):          # order 2 and order 5
        with pytest.raises(_lib.FarnnError) as e:
            _lib.CpContext.from_coo(bad_dims, bad_idx, val, 4)
        assert e.value.code == _lib.EINVAL
    with pytest.raises(_lib.FarnnError) as e:
        _lib.CpContext.from_coo(dims, [[], [], [], []], [], 4)                                      # empty coordinate lists
    assert e.value.code == _lib.EINVAL
    with pytest.raises(_lib.FarnnError) as e:
        _lib.CpContext.from_coo(dims, [[0], [0], [0], [4]], [1.0], 4)                               # a coordinate outside its dimension
    assert e.value.code == _lib.EINVAL
    ctx = _lib.CpContext.from_coo(dims, idx, val, cap + 40)
    small = _lib.CpContext.from_coo(dims, idx, val, 8)
    out = torch.full((dims[0], cap + 1), 7.0, dtype=torch.float64, device='cuda')
    fd = [dev(np.ones((d, cap + 1))) for d in dims]
    for c, R in ((ctx, cap + 1), (small, 9)):                                                       # rank above the cap
        for call in (lambda: c.mttkrp(0, R, ptrs(fd), out.data_ptr()), lambda: c.normal_matrix(0, R, ptrs(fd), out.data_ptr()),
                     lambda: c.solve(R, out.data_ptr(), out.data_ptr(), 1, out.data_ptr()),
                     lambda: c.run(R, 2, 1e-6, [np.ones((d, R)) for d in dims])):
            with pytest.raises(_lib.FarnnError) as e:
                call()
            assert e.value.code == _lib.ERANGE
    for call in (lambda: small.mttkrp(4, 8, ptrs(fd), out.data_ptr()), lambda: small.normal_matrix(4, 8, ptrs(fd), out.data_ptr()),
                 lambda: small.mttkrp(-1, 8, ptrs(fd), out.data_ptr())):                            # mode 4
        with pytest.raises(_lib.FarnnError) as e:
            call()
        assert e.value.code == _lib.EINVAL
    # a 3-way entry on an order-4 context
    p = ptrs(fd)
    assert lib.farnn_cp_mttkrp(small._raw, 0, 8, p[0], p[1], p[2], out.data_ptr(), None) == _lib.EINVAL
    assert lib.farnn_cp_normal_matrix(small._raw, 0, 8, p[0], p[1], p[2], out.data_ptr(), None) == _lib.EINVAL
    h = [np.full((d, 8), 3.0) for d in dims[:3]]
    errs, n = np.full(2, 5.0), _lib.C.c_int32(9)
    dp = lambda a: a.ctypes.data_as(_lib.C.POINTER(_lib.C.c_double))      # noqa: E731
    assert lib.farnn_cp_run(small._raw, 8, 2, 1e-6, dp(h[0]), dp(h[1]), dp(h[2]), dp(errs), _lib.C.byref(n), None) == _lib.EINVAL
    assert n.value == 0 and (errs == 5.0).all() and all((a == 3.0).all() for a in h)
    assert bool((host(out) == 7.0).all())                       # nothing was launched
    f, errs = small.run(8, 2, 1e-6, init)                       # the contexts still run
    _, want = ref.als(dims, idx, val, 8, init, 2)
    assert len(errs) == 2 and np.allclose(errs, want, rtol=0, atol=1e-9)
    ctx.close(); small.close()


def test_a_singular_normal_matrix_in_a_run_is_enumeric_and_the_context_survives():
    c = ref.load_cases()[0]
    dims, idx, val, init = ref.case_of(c)
    R = c['rank']
    ctx = _lib.CpContext.from_coo(dims, idx, val, R)
    bad = [a.copy() for a in init]
    bad[1][:, 1] = 0.0                                            # a zero factor column: a zero row and column of H, pivot exactly 0
    with pytest.raises(np.linalg.LinAlgError, match='-33'):
        ctx.run(R, 4, c['tol'], bad)
    f, errs = ctx.run(R, c['n_iter_max'], c['tol'], init)
    _, want = ref.als(dims, idx, val, R, init, c['n_iter_max'], c['tol'])
    assert len(errs) == len(want) and np.allclose(errs, want, rtol=0, atol=1e-9)
    ctx.close()


def test_mirror_on_a_dense_tensor_and_on_coordinates():
    c = ref.load_cases()[1]
    dims, idx, val, _ = ref.case_of(c)
    X = ref.dense_of(dims, idx, val)
    a = tf.tensor4_to_factors(X, c['rank'], n_iter_max=8, init='random', verbose=0, random_state=4)
    b = tf.tensor4_to_factors_coo(dims, idx, val, c['rank'], n_iter_max=8, init='random', verbose=0, random_state=4)
    _, want = ref.als(dims, idx, val, c['rank'], ref.init_factors(dims, c['rank'], 4), 8, 1e-6)
    assert a[4] == b[4] and all(np.array_equal(p, q) for p, q in zip(a[:4], b[:4]))
    assert np.allclose(a[4], want, rtol=0, atol=1e-9) and [m.shape for m in a[:4]] == [(d, c['rank']) for d in dims]


def test_end_to_end_decompose_then_tag(tmp_path):
    from oracle import farnn_oracle as fo
    from re2nn_seq_amd.farnn.model_decompose import FARNN_S_D_W
    from re2nn_seq_amd.init_params import get_init_params_seq
    # an automaton whose '$' edges carry 4 slots between 6 and 5 states: its wildcard tensor [C, S, S] has a rank-10 normal matrix
    # that is not singular (the default tree's has two such edges, and every restart at rank 10 ends in FARNN_ENUMERIC)
    tree = synth.write_dataset_tree(str(tmp_path / 'data'), n_entity_types=8, n_states=60, ranks=(300,), output_ranks=(300,))
    data_dir = tree['paths']['data_dir']
    path = da.main(['--dataset', 'ATIS-BIO', '--automata_path', tree['paths']['ID0'], '--independent', '0', '--ranks', '30',
                    '--wildcard_ranks', '10', '--k_best', '2', '--data_dir', data_dir, '--out_dir', str(tmp_path / 'out')])
    assert os.path.basename(path).startswith('D.automata.')
    args, _ = cli.parse_args(['--dataset', 'ATIS-BIO', '--method', 'decompose', '--independent', '0', '--automata_path', path,
                              '--rank', '30', '--rank_wildcard', '10', '--seed', '3', '--beta', '1.0', '--embed_dim', '16',
                              '--normalize_automata', 'none', '--rand_constant', '0', '--update_nonlinear', 'none',
                              '--local_loss_func', 'CE'])       # (the loader's CE1 check wants an `oo` row no D pickle has)
    s2i = tree['dset']['s2i']
    (V, C, S1, S2, E, _, WW, final, start, prio, Cw, S1w, S2w) = get_init_params_seq(args, s2i, data_dir=data_dir)
    args.local_loss_func = 'CE1'                                 # the model itself is built as the tagging tests build it
    m = FARNN_S_D_W(V=V, C=C, S1=S1, S2=S2, C_wildcard=Cw, S1_wildcard=S1w, S2_wildcard=S2w, wildcard_wildcard=WW,
                    final_vector=final, start_vector=start, pretrained_word_embed=E, priority_mat=prio, args=args, o_idx=s2i['o'])
    rng = np.random.RandomState(3)
    x, lengths = synth.random_batch(V.shape[0] - 1, 6, 9, rng, min_len=1)
    p = {'Vgen': m.generalized_vocab_table().numpy(), 'C': m.C_embed.numpy(), 'S1': m.S1.numpy(), 'S2': m.S2.numpy(),
         'Cw': m.C_wildcard.numpy(), 'S1w': m.S1_wildcard.numpy(), 'S2w': m.S2_wildcard.numpy(), 'WW': m.wildcard_wildcard.numpy(),
         'h0': m.h0.numpy(), 'hT': m.hT.numpy(), 'farnn': 0, 'nl': fo.NL_CODES['none'], 'semiring': fo.SEMIRING_SUM, 'sig_k': 5}
    want = fo.decomp_fst_scores(p, x, lengths)
    xt, lt = torch.from_numpy(x), torch.from_numpy(lengths)
    Lmax = int(lengths.max())
    r = m.run(xt[:, :Lmax], lt, _lib.MODE_FULL, want_scores=True)
    mask = np.arange(Lmax)[None, :] < lengths[:, None]
    np.testing.assert_allclose(r['scores'].cpu().numpy()[mask], want[mask], rtol=1e-4, atol=1e-4)
    _, pred, _ = m.forward_local(xt, torch.zeros_like(xt), lt, train=False)
    assert np.array_equal(pred.numpy(), fo.forward_local_tags(want, lengths, args.threshold, s2i['o']))
    # the error the file name records for the last outer seed: 3, whose running value is 3, 11 at the wildcard rank and 11, 19 here
    recorded = float(os.path.basename(path).split('.1splits.30:')[1].split(',..pkl')[0])
    T, _, _, _, _, _, language = f2t.dfa_to_tensor_slot_new(tree['automaton'], tree['dset']['t2i'], s2i, dataset='ATIS-BIO')
    X = T[np.array([tree['dset']['t2i'][w] for w in language])]
    idx, val = ref.coo_of(X)
    best, bar = np.inf, 0.0
    for rs in (11, 19):
        init = ref.init_factors(X.shape, 30, rs)
        errs, spread = ref.measure_spread(X.shape, idx, val, 30, init, 10, 1e-6)
        f, _ = ref.als(X.shape, idx, val, 30, init, 10, 1e-6)
        best = min(best, errs[-1])
        bar = max(bar, 8 * spread, ref.cancellation_bar(X.shape, 30, idx, val, f, errs[-1]))
    print('recorded', recorded, 'restatement', best, 'bar', bar)
    assert recorded <= best + bar + 5e-5
