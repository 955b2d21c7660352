"""The CP-ALS yardstick and the mirrors' plumbing, without a GPU: the two forms of the numpy restatement (cp_als_ref.py) agree,
the comparators the GPU tests use reject every planted fault, the golden cases are as stable as the case finder promised, and
wfa/decompose_automata.py -- with tensor_func.tensor3_to_factors replaced by the restatement -- squashes, restarts, selects and
writes what the reference's does, in pickles init_params loads."""
import os
import pickle

import numpy as np
import pytest

import cp_als_ref as ref
from re2nn_seq_amd import _lib, synth
from re2nn_seq_amd import main as cli
from re2nn_seq_amd.wfa import decompose_automata as da
from re2nn_seq_amd.wfa import tensor_func as tf

CASES = ref.load_cases()


def _case(c):
    dims = tuple(c['dims'])
    idx, val, init = ref.make_case(dims, c['nnz'], c['rank'], c['seed'])
    return dims, idx, val, init


@pytest.fixture(scope='module')
def measured():
    out = []
    for c in CASES:
        dims, idx, val, init = _case(c)
        errs, spread = ref.measure_spread(dims, idx, val, c['rank'], init, c['n_iter_max'])
        f, _ = ref.als(dims, idx, val, c['rank'], init, c['n_iter_max'])
        out.append((c, dims, idx, val, init, errs, spread, ref.cancellation_bar(dims, c['rank'], idx, val, f, errs[-1])))
    return out


def test_golden_cases_cover_the_issue_shapes_and_are_stable(measured):
    assert [(tuple(c['dims']), c['rank']) for c in CASES] == [((12, 5, 5), 3), ((40, 9, 9), 16), ((30, 7, 7), 17), ((64, 12, 12), 30)]
    for c, dims, idx, val, init, errs, spread, floor in measured:
        assert spread <= ref.SPREAD_MAX, (c, spread)
        assert len(errs) >= 3
    assert len(measured[0][5]) < CASES[0]['n_iter_max']            # one case stops on the tolerance, not on the sweep limit


def test_the_two_forms_agree_stage_by_stage():
    dims = (40, 9, 7)
    idx, val, f = ref.make_case(dims, 500, 17, 3)
    X = ref.dense_of(dims, idx, val)
    for mode in range(3):
        r, detail = ref.compare_mttkrp(ref.mttkrp_dense(X, f, mode), idx, val, f, mode, dims)
        assert r <= 1, (mode, detail)


def test_the_two_forms_agree_on_whole_runs(measured):
    for c, dims, idx, val, init, errs, spread, floor in measured:
        f, dense = ref.als(dims, idx, val, c['rank'], init, c['n_iter_max'], form='dense')
        r, detail = ref.compare_run(dense, errs, spread, floor)
        assert r <= 1, (c, detail)
        assert abs(ref.direct_error(dims, idx, val, f) - dense[-1]) <= floor
        assert all(b <= a + floor for a, b in zip(errs, errs[1:]))


def test_repeated_coordinates_add():
    dims = (6, 4, 4)
    idx, val, init = ref.make_case(dims, 30, 3, 5)
    idx2 = [np.concatenate([i, i[:7]]) for i in idx]
    val2 = np.concatenate([val, val[:7]])
    merged = val.copy(); merged[:7] *= 2
    _, a = ref.als(dims, idx2, val2, 3, init, 6)
    _, b = ref.als(dims, idx, merged, 3, init, 6)
    assert np.allclose(a, b, rtol=0, atol=1e-12)


@pytest.mark.parametrize('mutant', ref.MUTANTS)
def test_each_planted_fault_is_rejected(mutant, measured):
    dims = (40, 9, 7)
    idx, val, f = ref.make_case(dims, 500, 17, 3)
    if mutant == 'kr_pair':
        assert ref.compare_mttkrp(ref.mttkrp_coo(idx, val, f, 1, dims), idx, val, f, 1, dims)[0] <= 1
        assert ref.compare_mttkrp(ref.mttkrp_coo(idx, val, f, 1, dims, mutant), idx, val, f, 1, dims)[0] > 1
    elif mutant == 'gram_all':
        for mode in range(3):
            assert ref.compare_normal(ref.normal_matrix(f, mode), f, mode)[0] <= 1
            assert ref.compare_normal(ref.normal_matrix(f, mode, mutant), f, mode)[0] > 1
    elif mutant == 'no_transpose':
        rng = np.random.RandomState(0)
        H = rng.randn(17, 17) + 17 * np.eye(17)                     # asymmetric, well conditioned
        M = rng.randn(23, 17)
        assert ref.compare_solve(ref.solve_stage(H, M), H, M)[0] <= 1
        assert ref.compare_solve(ref.solve_stage(H, M, mutant), H, M)[0] > 1
    else:
        rejected = 0
        for c, dims, idx, val, init, errs, spread, floor in measured:
            start = ref.init_factors(dims, c['rank'], c['seed'], mutant)
            _, got = ref.als(dims, idx, val, c['rank'], start, c['n_iter_max'], mutant=mutant)
            rejected += ref.compare_run(got, errs, spread, floor)[0] > 1
        # the early stop shows only where the run stops on the tolerance (the first case); the other two faults show everywhere
        assert rejected == (1 if mutant == 'stop_early' else len(measured)), rejected


# ---- the mirrors' plumbing ------------------------------------------------------------------------------------------------------
def _restatement(calls):
    def tensor3_to_factors(tensor, rank, n_iter_max=50, init='svd', verbose=10, random_state=1):
        assert init == 'random'
        calls.append({'shape': tensor.shape, 'rank': rank, 'n_iter_max': n_iter_max, 'random_state': random_state})
        idx, val = ref.coo_of(np.asarray(tensor, np.float64))
        f, errs = ref.als(tensor.shape, idx, val, rank, ref.init_factors(tensor.shape, rank, random_state), n_iter_max)
        return f[0], f[1], f[2], errs
    return tensor3_to_factors


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return synth.write_dataset_tree(str(tmp_path_factory.mktemp('cpdata')), dataset='ATIS-BIO', seed=4)


def test_squash_and_unsquash_of_the_language_rows(monkeypatch):
    calls = []
    monkeypatch.setattr(tf, 'tensor3_to_factors', _restatement(calls))
    rng = np.random.RandomState(1)
    T = (rng.rand(9, 4, 4) < 0.3).astype(np.float64)
    word2idx = {'w%d' % i: i for i in range(9)}
    language = ['w7', 'w2', 'w5']
    V, S1, S2, errs = tf.decompose_tensor_split_slot_3d_language(T, language, word2idx, 3, random_state=2, n_iter_max=5, init='random')
    assert calls[0]['shape'] == (3, 4, 4) and calls[0]['random_state'] == 2 and calls[0]['n_iter_max'] == 5
    idx, val = ref.coo_of(T[[7, 2, 5]])
    f, e = ref.als((3, 4, 4), idx, val, 3, ref.init_factors((3, 4, 4), 3, 2), 5)
    assert V.shape == (9, 3) and np.array_equal(V[[7, 2, 5]], f[0]) and not V[[0, 1, 3, 4, 6, 8]].any()
    assert np.array_equal(S1, f[1]) and np.array_equal(S2, f[2]) and errs == e
    rec = tf.recover_tensor_from_factors([f[0], f[1], f[2]])
    assert np.allclose(rec, np.einsum('ir,jr,kr->ijk', *f)) and np.allclose(tf.recover_tensor_from_factors((None, f)), rec)


def test_iiid_writer_seeds_selection_schema_and_loader(tree, tmp_path, monkeypatch):
    calls = []
    fake = _restatement(calls)

    def flaky(tensor, rank, **kw):                                   # the restart at rands = 8 (outer seed 0 only) raises
        if kw['random_state'] == 8:
            calls.append({'random_state': 8, 'raised': True})
            raise np.linalg.LinAlgError('singular')
        return fake(tensor, rank, **kw)
    monkeypatch.setattr(tf, 'tensor3_to_factors', flaky)
    path = da.decompose_automata_single(tree['automaton'], 'ATIS-BIO', 'synthetic', 1, k_best=3, rule_name='r',
                                        data_dir=tree['paths']['data_dir'], out_dir=str(tmp_path), ranks=[4, 6])
    name = os.path.basename(path)
    assert name.startswith('IIID.automata.') and '.random.3best.{}states.synthetic.1splits.'.format(len(tree['automaton']['states'])) in name
    assert name.endswith('.r.pkl')
    # rands = seed, then + k * 8 before every restart, carried from one rank to the next (ref :383-391): 0, 8, 24 for k = 0, 1, 2
    expect = []
    for seed in range(4):
        rands = seed
        for rank in (4, 6):
            for k in range(3):
                rands += k * 8
                expect.append((rank, rands))
    got = [(c.get('rank'), c['random_state']) for c in calls]
    assert [g[1] for g in got] == [e[1] for e in expect]
    assert all(g[0] in (None, e[0]) for g, e in zip(got, expect)) and all(c.get('n_iter_max', 32) == 32 for c in calls)
    with open(path, 'rb') as f:
        d = pickle.load(f)
    assert sorted(k for k in d if k != 'automata') == [0, 1, 2, 3] and d['automata'] == tree['automaton']
    ref_dict = synth.make_iiid_pickle_dict(tree['automaton'], tree['dset']['t2i'], tree['dset']['s2i'], [100], np.random.RandomState(0), noise=0)
    for seed in range(4):
        per_rank, out1, out2 = d[seed]
        assert sorted(per_rank) == [4, 6]
        for R, fd in per_rank.items():
            assert sorted(fd) == ['S1', 'S2', 'V', 'wildcard_mat']
            assert fd['V'].shape == (len(tree['dset']['t2i']), R) and fd['V'].dtype == np.float64
            assert fd['S1'].shape == fd['S2'].shape == (ref_dict[0][0][100]['S1'].shape[0], R)
            assert np.array_equal(fd['wildcard_mat'], ref_dict[0][0][100]['wildcard_mat'])
        assert np.array_equal(out1['output_mat'], ref_dict[0][1]['output_mat']) and np.array_equal(out2['output_mat'], ref_dict[0][2]['output_mat'])
        assert out1['output_wildcard_vector'].shape == out2['output_wildcard_vector'].shape == (out1['output_mat'].shape[1],)
    # k-best: the stored factors are those of the restart with the lowest last error among the restarts that did not raise
    from re2nn_seq_amd.wfa.fsa_to_tensor import dfa_to_tensor_slot_single_wildcard
    T, _, _, _, _, _, _, language = dfa_to_tensor_slot_single_wildcard(tree['automaton'], tree['dset']['t2i'], tree['dset']['s2i'],
                                                                       dataset='ATIS-BIO')
    rows = np.array([tree['dset']['t2i'][w] for w in language])
    idx, val = ref.coo_of(T[rows])
    dims = T[rows].shape
    tried = {0: [0, 24], 1: [1, 9, 25]}                             # seed 0: the restart at rands = 8 raised and was skipped
    for seed, rs in tried.items():
        runs = [ref.als(dims, idx, val, 4, ref.init_factors(dims, 4, r), 32) for r in rs]
        best = min(runs, key=lambda fe: fe[1][-1])
        assert np.array_equal(d[seed][0][4]['V'][rows], best[0][0]) and np.array_equal(d[seed][0][4]['S1'], best[0][1])
    assert '4-{}'.format(round(min(ref.als(dims, idx, val, 4, ref.init_factors(dims, 4, r), 32)[1][-1] for r in (3, 11, 27)), 4)) in name
    # the pickle loads through the decomposed model's loader
    args, _ = cli.parse_args(['--dataset', 'ATIS-BIO', '--method', 'decompose', '--independent', '2', '--automata_path', path,
                              '--rank', '6', '--seed', '1', '--embed_dim', '16', '--normalize_automata', 'none'])
    from re2nn_seq_amd.init_params import get_init_params_seq_independent_single
    t2i = dict(tree['dset']['t2i']); t2i['<pad>'] = len(t2i)
    out = get_init_params_seq_independent_single(args, tree['dset']['s2i'], t2i, data_dir=tree['paths']['data_dir'])
    assert out[0].shape == (len(t2i), 6) and np.array_equal(out[0][:-1], d[1][0][6]['V']) and not out[0][-1].any()


def test_iid_writer_schema_and_loader(tree, tmp_path, monkeypatch):
    calls = []
    monkeypatch.setattr(tf, 'tensor3_to_factors', _restatement(calls))
    path = da.decompose_automata_independent(tree['automaton'], 'ATIS-BIO', 'synthetic', 1, k_best=2, data_dir=tree['paths']['data_dir'],
                                             out_dir=str(tmp_path), ranks=[5], output_tensor_ranks=[3])
    assert os.path.basename(path).startswith('IID.automata.') and '.random.2best.' in path
    # per outer seed: rands = seed; C tensor k = 0, 1, then C+1 tensor k = 0, 1 (carried on), then rands = 0 for the language tensor
    expect = []
    for seed in range(4):
        expect += [seed, seed + 8, seed + 8, seed + 16, 0, 8]
    assert [c['random_state'] for c in calls] == expect and all(c['n_iter_max'] == 40 for c in calls)
    with open(path, 'rb') as f:
        d = pickle.load(f)
    C = len(tree['dset']['s2i'])
    for seed in range(4):
        per_rank, out1, out2 = d[seed]
        assert sorted(per_rank[5]) == ['S1', 'S2', 'V', 'wildcard_mat']
        assert out1[3]['C_output'].shape == (C, 3) and out2[3]['C_output'].shape == (C + 1, 3)
        assert out1[3]['wildcard_output'].shape == out1[3]['S1_output'].shape[:1] * 2 and out2[3]['wildcard_output'] is None
    args, _ = cli.parse_args(['--dataset', 'ATIS-BIO', '--method', 'decompose', '--independent', '1', '--automata_path', path,
                              '--rank', '5', '--rank_wildcard', '3', '--seed', '2', '--embed_dim', '16', '--normalize_automata', 'none'])
    from re2nn_seq_amd.init_params import get_init_params_seq_independent
    t2i = dict(tree['dset']['t2i']); t2i['<pad>'] = len(t2i)
    out = get_init_params_seq_independent(args, tree['dset']['s2i'], t2i, data_dir=tree['paths']['data_dir'])
    assert out[0].shape == (len(t2i), 5)


def test_refusals():
    T4 = np.zeros((3, 2, 2, 2))
    with pytest.raises(NotImplementedError, match='DESIGN.md'):
        tf.tensor4_to_factors(T4, 2)
    with pytest.raises(NotImplementedError, match='DESIGN.md'):
        tf.decompose_tensor_split_slot_4d(T4, ['a'], {'a': 0}, 2)
    with pytest.raises(NotImplementedError, match='DESIGN.md'):
        da.decompose_automata({'states': {0}}, 'ATIS-BIO', 'x', 1)
    with pytest.raises(NotImplementedError, match='svd'):
        tf.tensor3_to_factors(np.ones((3, 2, 2)), 2)                 # the reference's default init
    with pytest.raises(NotImplementedError, match='svd'):
        tf.tensor3_to_factors_coo((3, 2, 2), [0], [0], [0], [1.0], 2, init='svd')
    with pytest.raises(AssertionError):
        tf.tensor3_to_factors(np.ones((3, 2, 2)), 2, init='zeros')


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    with pytest.raises(_lib.FarnnError):
        tf.tensor3_to_factors(np.ones((3, 2, 2)), 2, init='random')
    with pytest.raises(_lib.FarnnError):
        tf.tensor3_to_factors_coo((3, 2, 2), [0, 1], [0, 1], [1, 0], [1.0, 2.0], 2, init='random')
