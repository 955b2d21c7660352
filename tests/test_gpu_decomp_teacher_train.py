"""The KD / PR teacher step of the decomposed i-FST (--marryup_type kd | pr) on the GPU: the reference's
captures through the model mirror, the float64 / float32 restatement (tests/decomp_teacher_train_ref.py) through the C-ABI at
the sizes where the new code takes another path, repeatability, the plain step around a teacher step, the refusals, and one
epoch through the command line."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import decomp_teacher_train_ref as dtr  # noqa: E402
from test_decomp_teacher_train_cpu import BASE, G, META, N_CONFIGS, mirror as cpu_mirror, names_of  # noqa: E402
from test_gpu_train_max import GATES, OUT_NAMES, close, draw, run_library  # noqa: E402
from util import _grad_figures, assert_float_path, check_grad  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def opted_in(monkeypatch):
    monkeypatch.setenv('RE2NN_DECOMP_TEACHER_TRAIN', '1')


# ---- 1. the reference's captures through the mirror -------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(N_CONFIGS))
def test_teacher_step_matches_reference_captures(k):
    """forward_local(train=True, re_tags=...) -> loss.backward() -> .grad of every parameter and the flat predictions; the
    step's tags equal forward_local(train=False) on the same weights."""
    cfg = {kk: v for kk, v in META['configs'][k].items() if kk != 'seed'}
    m = cpu_mirror(**dict(META['train_flags'], **cfg))
    pre = 'c{}.'.format(k)
    names = names_of(k)
    sd = {n: G[pre + 'w.' + n] for n in names}
    sd['priority_layer.priority_mat'] = G[pre + 'w.priority_mat']
    m.load_state_dict(sd)
    x, lengths, labels = torch.from_numpy(BASE['x']), torch.from_numpy(BASE['lengths']), torch.from_numpy(G['labels'])
    m.train()
    loss, pred, _ = m.forward_local(x, labels, lengths, train=True, re_tags=torch.from_numpy(G['re_tags']))
    loss.backward()
    ref_loss = float(G[pre + 'loss'])
    print('config', k, 'loss', float(loss.detach()), 'ref', ref_loss)
    assert abs(float(loss.detach()) - ref_loss) < 2e-5 * max(1.0, abs(ref_loss))
    assert np.array_equal(pred.cpu().numpy(), G[pre + 'flat_pred'])
    named = dict(m.named_parameters())
    assert set(named) == set(names)
    for n in names:
        close(named[n].grad.cpu().numpy(), G[pre + 'g.' + n], n)
    m.eval()
    _, pred_eval, _ = m.forward_local(x, labels, lengths, train=False)
    assert np.array_equal(pred.cpu().numpy(), pred_eval.cpu().numpy())


# ---- 2. the restatement through the C-ABI -------------------------------------------------------------------------------------
def teacher_case(S, R, K, V, B, L, nl, farnn, crf, prio, seed, full=False):
    w, x, _, labels = draw(S, R, K, V, B, L, nl, farnn, crf, prio, seed=seed)
    rng = np.random.RandomState(seed + 1)
    lengths = np.array(([0, 1, max(L - 1, 1), L] + list(rng.randint(0, L + 1, size=B)))[:B], np.int64)
    if full:
        lengths[:] = L
    re = (rng.rand(B, L, K) * 0.1).astype(np.float32)
    hot = rng.rand(B, L, K) < 0.15
    re[hot] = 0.9 + 0.1 * rng.rand(int(hot.sum())).astype(np.float32)
    re[..., K - (3 if crf else 1):] = 0.0                     # the zero columns the caller appends
    return w, x, lengths, labels, re


def run_teacher(w, x, lengths, labels, re, mode, c1, pi, nl, farnn, crf, tc=None, semiring='sum'):
    from re2nn_seq_amd import _lib
    V, R = w['Vgen'].shape
    S, K = w['S1'].shape[0], w['C'].shape[0]
    B, L = x.shape
    dev = torch.device('cuda')
    if tc is None:
        tc = _lib.TrainContext(V, S, R, K, nl=nl, threshold=0.5, o_idx=1, use_crf=crf, farnn=farnn, semiring=semiring)
    wd = {n: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for n, v in w.items()}
    weights = {n: wd[n].data_ptr() for n in OUT_NAMES}
    weights['P'] = wd['P'].data_ptr() if 'P' in wd else None
    weights['crf_trans'] = wd['trans'].data_ptr() if 'trans' in wd else None
    out = {'d' + n: torch.full_like(wd[n], 7.0) for n in OUT_NAMES}          # the library must zero them itself
    for n in GATES[:3 * farnn]:
        weights[n] = wd[n].data_ptr()
        out['d' + n] = torch.full_like(wd[n], 7.0)
    if crf:
        out['dtrans'] = torch.full_like(wd['trans'], 7.0)
    loss = torch.full((1,), 3.0, device=dev)
    tags = torch.full((B, L), -7, dtype=torch.int32, device=dev)
    xd, ld, labd, red = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, lengths, labels, re))
    try:
        tc.teacher_step(weights, xd.data_ptr(), ld.data_ptr(), labd.data_ptr(), red.data_ptr(), mode, c1, pi, B, L,
                        max(int(lengths.sum()), 1), dict({n: t.data_ptr() for n, t in out.items()}, loss=loss.data_ptr(),
                                                         tags=tags.data_ptr()))
    finally:
        torch.cuda.synchronize()
        res = {n: t.cpu().numpy() for n, t in out.items()}
        res['loss'] = float(loss)
        res['tags'] = tags.cpu().numpy()
        run_teacher.last = res
    return res, tc


def check_teacher(res, ref32, ref64, farnn, crf, x, case):
    l32, g32, _ = ref32
    l64, g64, sc = ref64
    print(case, 'loss', res['loss'], 'f64', l64)
    assert_float_path([res['loss']], [l32], [l64], 1e-4, 'loss')
    present = np.zeros(g64['Vgen'].shape[0], bool)
    present[np.asarray(x).ravel()] = True                     # the words present at ANY position, pads included
    for n in list(OUT_NAMES) + list(GATES[:3 * farnn]) + (['trans'] if crf else []):
        got = res['d' + n].reshape(g64[n].shape)
        assert_float_path(got, g32[n], g64[n], 1e-4, 'd' + n)
        check_grad(case, 'd' + n, got, g32[n], g64[n], slices=0 if n == 'Vgen' else None, present=present if n == 'Vgen' else None)
    return sc


def well_drawn(ref32, ref64, x, tol=1e-4):
    """check_grad's conditions on the inputs, from the two references alone: the float32 restatement within tol / 10 of every
    tensor's scale, and at most 1 % of the present words ill-conditioned in it"""
    present = np.zeros(ref64[1]['Vgen'].shape[0], bool)
    present[np.asarray(x).ravel()] = True
    for n, b in ref64[1].items():
        a = ref32[1][n]
        if float(np.abs(a - b).max()) > tol / 10 * float(np.abs(b).max()):
            return False
        if n == 'Vgen':
            r, _ = _grad_figures(b, a, b, tol, 0, present)
            if r['fallback'] > 0.01 * r['present']:
                return False
    return True


def drawn_refs(S, R, K, V, B, L, nl, farnn, crf, prio, mode, c1, pi, seed0):
    """the first draw from seed0 on that is well drawn (a long chain can leave one word's gradient to cancellation)"""
    for seed in range(seed0, seed0 + 10):
        w, x, lengths, labels, re = teacher_case(S, R, K, V, B, L, nl, farnn, crf, prio, seed=seed)
        ref64 = dtr.step_on_table(w, x, lengths, labels, re, mode, c1, pi, nl=nl, farnn=farnn, dtype=torch.float64)
        ref32 = dtr.step_on_table(w, x, lengths, labels, re, mode, c1, pi, nl=nl, farnn=farnn, dtype=torch.float32)
        if well_drawn(ref32, ref64, x):
            return w, x, lengths, labels, re, ref32, ref64
    pytest.fail('no well-drawn case')


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


FULL = -1
TEACHER_CASES = [   # S, R, K, V, B, L, nl, farnn, crf, prio, mode, c1, pi
    pytest.param(7, 5, 3, 9, 3, 1, 'tanh', 0, False, False, 'kd', 2.0, 0.3, id='K3-L1'),                  # one position per sequence
    pytest.param(12, 8, 4, 30, 5, 2, 'none', 0, True, False, 'pr', 2.0, 0.3, id='K4-crf-L2'),             # smallest CRF
    pytest.param(23, 70, 63, 50, 5, 33, 'relutanh', 2, False, True, 'kd', 4.0, 0.5, id='K63-L33-g2-prio'),
    pytest.param(40, 30, 64, 50, 6, 9, 'tanh', 1, False, False, 'pr', 1.0, 0.0, id='K64-g1-pi0'),
    pytest.param(64, 64, 65, 40, 5, 7, 'tanh', 0, True, True, 'pr', 4.0, 0.3, id='K65-crf-prio'),
    pytest.param(134, 250, 130, 60, 5, 8, 'tanh', 2, True, False, 'kd', 2.0, 0.1, id='K130-shipped-g2-crf'),
    pytest.param(256, 64, 140, 50, 5, 6, 'tanh', 0, False, True, 'kd', 2.0, 0.3, id='K140-S256-C-through-L2'),    # teacher_loss<false, 0>
    pytest.param(232, 30, 150, 50, 3, 4, 'tanh', 0, True, False, 'pr', 2.0, 0.05, id='K150-crf-C-through-L2'),    # <false, 1|2>, crf<true>
    pytest.param(257, 40, 12, 50, 5, 6, 'tanh', 1, False, False, 'pr', 2.0, 0.3, id='S257-g1'),                   # chains through L2, 2 slots
    pytest.param(64, 200, 12, 50, 5, 6, 'tanh', 1, True, False, 'kd', 2.0, 0.1, id='R200-g1-crf'),               # forward LDS, backward L2
    pytest.param(40, 257, 12, 50, 5, 6, 'none', 0, False, False, 'kd', 1.0, 0.0, id='R257-pi0'),
    pytest.param(129, 100, 12, 100, FULL, 4, 'none', 0, False, False, 'kd', 2.0, 0.3, id='S129-full-4seq'),       # 4 sequences per workgroup
]


@pytest.mark.parametrize('S,R,K,V,B,L,nl,farnn,crf,prio,mode,c1,pi', TEACHER_CASES)
def test_c_abi_vs_restatement(S, R, K, V, B, L, nl, farnn, crf, prio, mode, c1, pi):
    if B == FULL:
        B = 2 * n_cu() + 1
    w, x, lengths, labels, re, ref32, ref64 = drawn_refs(S, R, K, V, B, L, nl, farnn, crf, prio, mode, c1, pi, S + R + K + farnn)
    res, _ = run_teacher(w, x, lengths, labels, re, mode, c1, pi, nl, farnn, crf)
    check_teacher(res, ref32, ref64, farnn, crf, x, 'teacher {} S{} R{} K{} farnn{} crf{}'.format(mode, S, R, K, farnn, int(crf)))
    mask = np.arange(L)[None, :] < lengths[:, None]
    assert (res['tags'][~mask] == -1).all() and (res['tags'][mask] >= 0).all()


@pytest.mark.parametrize('mode', ['kd', 'pr'])
@pytest.mark.parametrize('farnn,crf,prio', [(0, False, False), (2, True, True), (1, False, True)])
def test_pi_one_is_the_plain_step(mode, farnn, crf, prio):
    """pi = 1: loss, gradients and tags equal the plain entry's (the chains still run L steps, their adjoints are zero)"""
    S, R, K, V, B, L = 40, 30, 10, 50, 7, 9
    w, x, lengths, labels, re = teacher_case(S, R, K, V, B, L, 'tanh', farnn, crf, prio, seed=21)
    plain, _ = run_library(w, x, lengths, labels, 'tanh', farnn, crf, semiring='sum')
    res, _ = run_teacher(w, x, lengths, labels, re, mode, 2.0, 1.0, 'tanh', farnn, crf)
    assert np.array_equal(res['tags'], plain['tags'])
    assert abs(res['loss'] - plain['loss']) < 2e-5 * max(1.0, abs(plain['loss']))
    for n in plain:
        if n not in ('tags', 'loss'):
            close(res[n], plain[n], n)


@pytest.mark.parametrize('farnn,crf', [(0, False), (2, True)])
def test_full_length_batch_runs_the_plain_chains_bit_for_bit(farnn, crf):
    """No pads: the teacher step's chains are the plain step's.  With pi = 1 the adjoints are the plain step's too, so every
    output free of multi-way float atomics (tags, dS1, dS2, dW: one product per chain, two commutative adds) is bit-identical."""
    S, R, K, V, B, L = 40, 30, 10, 50, 5, 9
    w, x, lengths, labels, re = teacher_case(S, R, K, V, B, L, 'tanh', farnn, crf, False, seed=22, full=True)
    plain, _ = run_library(w, x, lengths, labels, 'tanh', farnn, crf, semiring='sum')
    res, _ = run_teacher(w, x, lengths, labels, re, 'kd', 2.0, 1.0, 'tanh', farnn, crf)
    for n in ('tags', 'dS1', 'dS2', 'dW'):
        assert np.array_equal(res[n], plain[n]), n


# ---- 3. / 4. repeatability and the plain step around a teacher step ------------------------------------------------------------
EXACT = ('tags', 'dS1', 'dS2', 'dW')       # outputs no multi-way float atomic of the chain kernels reaches (train.hip.h)


def same(a, b, exact):
    """bit-identical where the step's design gives it; elsewhere the rule tests/test_gpu_train_handles.py holds the decomposed
    step to, whose chain kernels add dVgen, dh0, dhT and dOsum with float atomics in arrival order"""
    for n in a:
        if n in exact:
            assert np.array_equal(a[n], b[n]), n
        else:
            ref = np.asarray(b[n], np.float64)
            assert (np.abs(np.asarray(a[n]) - ref) <= 1e-4 * (1 + np.abs(ref))).all(), n


@pytest.mark.parametrize('mode,crf', [('kd', False), ('pr', False), ('kd', True)])
def test_two_teacher_steps_repeat(mode, crf):
    """The teacher's own terms use no float atomic: without the CRF the loss (per-wavefront partials in index order) repeats
    bit for bit, as do the tags and the products of the stashed rows."""
    S, R, K, V, B, L = 40, 30, 10, 50, 7, 9
    w, x, lengths, labels, re = teacher_case(S, R, K, V, B, L, 'tanh', 1, crf, True, seed=23)
    a, tc = run_teacher(w, x, lengths, labels, re, mode, 2.0, 0.3, 'tanh', 1, crf)
    b, _ = run_teacher(w, x, lengths, labels, re, mode, 2.0, 0.3, 'tanh', 1, crf, tc=tc)
    same(a, b, EXACT + (() if crf else ('loss',)))


def test_plain_steps_around_a_teacher_step_are_the_same():
    """the teacher leaves no state behind on the context"""
    S, R, K, V, B, L = 40, 30, 10, 50, 7, 9
    w, x, lengths, labels, re = teacher_case(S, R, K, V, B, L, 'tanh', 2, True, False, seed=24)
    before, tc = run_library(w, x, lengths, labels, 'tanh', 2, True, semiring='sum')
    run_teacher(w, x, lengths, labels, re, 'pr', 2.0, 0.3, 'tanh', 2, True, tc=tc)
    after, _ = run_library(w, x, lengths, labels, 'tanh', 2, True, tc=tc)
    same(after, before, EXACT)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,c1,pi,semiring,big,code', [
    (3, 2.0, 0.3, 'sum', False, -22), ('kd', 0.5, 0.3, 'sum', False, -22), ('pr', 2.0, 1.5, 'sum', False, -22),
    ('pr', 2.0, -0.1, 'sum', False, -22), ('kd', 2.0, float('nan'), 'sum', False, -22), ('kd', 2.0, 0.3, 'max', False, -22),
    ('kd', 2.0, 0.3, 'sum', True, -34)])
def test_refusals_leave_the_outputs_untouched(mode, c1, pi, semiring, big, code):
    from re2nn_seq_amd import _lib
    S, R, K, V, B, L = 12, 8, 5, 20, 4, 6
    w, x, lengths, labels, re = teacher_case(S, R, K, V, B, L, 'tanh', 0, False, False, seed=25)
    tc = _lib.TrainContext(V, S, R, K, nl='tanh', semiring=semiring)
    if big:                                                   # B (L + 1) >= 2^30 on the small batch's real pointers: refused by the plan
        x = np.broadcast_to(x[:1, :1], (1 << 15, 1 << 15))
    with pytest.raises(_lib.FarnnError) as e:
        if big:
            _teacher_raw(tc, w, x, lengths, labels, re, mode, c1, pi)
        else:
            run_teacher(w, x, lengths, labels, re, mode, c1, pi, 'tanh', 0, False, tc=tc)
    assert 'code {}'.format(code) in str(e.value), str(e.value)
    if not big:
        res = run_teacher.last
        assert res['loss'] == 3.0 and (res['tags'] == -7).all()
        assert all((res['d' + n] == 7.0).all() for n in OUT_NAMES)


def _teacher_raw(tc, w, x, lengths, labels, re, mode, c1, pi):
    """the entry with B, L far beyond the buffers it is handed: legal only because the plan refuses before anything runs"""
    dev = torch.device('cuda')
    wd = {n: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for n, v in w.items()}
    out = {'d' + n: torch.full_like(wd[n], 7.0) for n in OUT_NAMES}
    small = {n: torch.zeros(8, dtype=torch.int64, device=dev) for n in ('x', 'len', 'lab')}
    red = torch.zeros(8, device=dev)
    loss, tags = torch.full((1,), 3.0, device=dev), torch.full((8,), -7, dtype=torch.int32, device=dev)
    try:
        tc.teacher_step({n: wd[n].data_ptr() for n in OUT_NAMES}, small['x'].data_ptr(), small['len'].data_ptr(),
                        small['lab'].data_ptr(), red.data_ptr(), mode, c1, pi, x.shape[0], x.shape[1], 10,
                        dict({n: t.data_ptr() for n, t in out.items()}, loss=loss.data_ptr(), tags=tags.data_ptr()))
    finally:
        torch.cuda.synchronize()
        assert float(loss) == 3.0 and all(bool((t == 7.0).all()) for t in out.values())


# ---- 6. one epoch through the command line ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    from re2nn_seq_amd import synth
    root = str(tmp_path_factory.mktemp('data'))
    return synth.write_dataset_tree(root, dataset='ATIS-BIO', seed=4)


def epoch_loss(tree, out_dir, extra):
    from re2nn_seq_amd import main as cli
    argv = ['--dataset', 'ATIS-BIO', '--method', 'decompose', '--independent', '2',
            '--automata_path', tree['paths']['IIID'], '--rank', '100', '--seed', '1', '--beta', '0.9',
            '--embed_dim', '16', '--normalize_automata', 'none', '--rand_constant', '0',
            '--update_nonlinear', 'tanh', '--bz', '64', '--seq_max_len', '12', '--epoch', '1', '--lr', '0.01',
            '--train_portion', '1.0', '--data_dir', tree['paths']['data_dir'], '--model_dir', str(out_dir)] + extra
    _, stats, res_path = cli.main(argv)
    assert len(stats['train_step']) == 1 and stats['train_step'][0]['tokens'] > 0
    losses = [float(line.split('LOSS:')[1]) for line in cli.load_res(res_path)['logger'].record if 'LOSS:' in line]
    assert len(losses) == 1 and np.isfinite(losses[0])
    return losses[0]


@pytest.fixture(scope='module')
def plain_loss(tree, tmp_path_factory):
    return epoch_loss(tree, tmp_path_factory.mktemp('plain'), [])


@pytest.mark.parametrize('mode', ['kd', 'pr'])
def test_one_epoch_through_the_command_line(tree, tmp_path, plain_loss, mode, monkeypatch):
    """--marryup_type kd | pr: with the original loss's weight 1 the epoch's loss is the plain run's; with 0.5 it is not"""
    from re2nn_seq_amd import RE
    monkeypatch.setitem(RE.DEFAULT_RE_AUTOMATA, 'ATIS-BIO', tree['paths']['ID2'])      # the RE teacher's automaton: the tiny tree's
    # The reference appends ONE zero column to the teacher's scores (model_decompose_single.py:213-218), so it expects them one
    # column narrower than the model's; the tiny tree's RE automaton scores every label of the model, and the reference itself
    # would stop at KLDivLoss on it.  The teacher's last column is cut here, where the zero column goes.
    full = RE.predict_by_RE
    monkeypatch.setattr(RE, 'predict_by_RE', lambda *a, **k: tuple(t[..., :-1] if i >= 3 else t for i, t in enumerate(full(*a, **k))))
    extra = ['--marryup_type', mode, '--c1_kdpr', '2', '--c3_pr', '0.2']
    bar = 2e-5 * max(1.0, abs(plain_loss))
    one = epoch_loss(tree, tmp_path / 'one', extra + ['--c2_kdpr', '1'])
    half = epoch_loss(tree, tmp_path / 'half', extra + ['--c2_kdpr', '0.5'])
    print(mode, 'plain', plain_loss, 'c2=1', one, 'c2=0.5', half)
    assert abs(one - plain_loss) <= bar
    assert abs(half - plain_loss) > bar
