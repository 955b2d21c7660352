"""The KD / PR teacher step of the decomposed i-FST in the MAX semiring (--train_mode max --marryup_type kd | pr; DESIGN.md,
row f3) on the GPU: the reference's captures through the model mirror, the float64 / float32 restatement
(tests/decomp_teacher_max_train_ref.py) through the C-ABI at the sizes where the tmax_* kernels take another path, pi = 1
against the plain max step, the plain steps after a teacher step, repeatability, the refusals, and one epoch through the
command line.

Drawn cases keep the arg-max gap rule (2e-5 relative, float32 and float64, or an exact tie in both) at ALL L steps of every
sequence, since with a teacher every step reaches a score; a draw that misses it is drawn again with the next seed."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import decomp_teacher_max_train_ref as dxr  # noqa: E402
from test_decomp_teacher_max_train_cpu import BASE, G, META, N_CONFIGS, TODAY_MAX, mirror as cpu_mirror, names_of  # noqa: E402
from test_gpu_decomp_teacher_train import check_teacher, epoch_loss, run_teacher, same, well_drawn  # noqa: E402
from test_gpu_train_max import MIN_GAP, OUT_NAMES, close, draw, run_library  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def opted_in(monkeypatch):
    monkeypatch.setenv('RE2NN_DECOMP_TEACHER_TRAIN', '1')
    monkeypatch.setenv('RE2NN_DECOMP_TEACHER_MAX_TRAIN', '1')


def context(w, nl, farnn, crf, semiring='max', teacher_max=True):
    from re2nn_seq_amd import _lib
    V, R = w['Vgen'].shape
    return _lib.TrainContext(V, w['S1'].shape[0], R, w['C'].shape[0], nl=nl, threshold=0.5, o_idx=1, use_crf=crf, farnn=farnn,
                             semiring=semiring, teacher_max=teacher_max)


def run_teacher_max(w, x, lengths, labels, re, mode, c1, pi, nl, farnn, crf, tc=None):
    tc = tc or context(w, nl, farnn, crf)
    return run_teacher(w, x, lengths, labels, re, mode, c1, pi, nl, farnn, crf, tc=tc)


# ---- 1. the reference's captures through the mirror -------------------------------------------------------------------------
@pytest.mark.parametrize('k', range(N_CONFIGS))
def test_teacher_max_step_matches_reference_captures(k):
    """forward_local(train=True, re_tags=...) -> loss.backward() -> .grad of every parameter and the flat predictions"""
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


# ---- 2. the restatement through the C-ABI -------------------------------------------------------------------------------------
def teacher_case(S, R, K, V, B, L, nl, farnn, crf, prio, seed, full=False):
    """lengths [0, 1, L-1, L, ...] in one batch (or all L); with prio a SIGNED priority matrix; the words of the pad positions
    are random, so with a small V some occur at pads only"""
    w, x, _, labels = draw(S, R, K, V, B, L, nl, farnn, crf, prio, seed=seed)
    rng = np.random.RandomState(seed + 1)
    lengths = np.array(([0, 1, max(L - 1, 1), L] + list(rng.randint(0, L + 1, size=B)))[:B], np.int64)
    if full:
        lengths[:] = L
    if prio:
        w['P'] = (np.eye(K) + (rng.rand(K, K) < 0.3) * rng.randn(K, K) * 0.5).astype(np.float32)
    re = (rng.rand(B, L, K) * 0.1).astype(np.float32)
    hot = rng.rand(B, L, K) < 0.15
    re[hot] = 0.9 + 0.1 * rng.rand(int(hot.sum())).astype(np.float32)
    re[..., K - (3 if crf else 1):] = 0.0                     # the zero columns the caller appends
    return w, x, lengths, labels, re


def pad_only_words(x, lengths):
    valid = np.arange(x.shape[1])[None, :] < lengths[:, None]
    return sorted(set(x[~valid]) - set(x[valid]))


def drawn_refs(S, R, K, V, B, L, nl, farnn, crf, prio, mode, c1, pi, seed0, full=False):
    """the first draw from seed0 on that keeps the gap rule over all L steps and is well drawn; a small batch with pads must
    also have a word that occurs at pad positions only"""
    for seed in range(seed0, seed0 + 40):
        w, x, lengths, labels, re = teacher_case(S, R, K, V, B, L, nl, farnn, crf, prio, seed=seed, full=full)
        if not full and B * L < 256 and not pad_only_words(x, lengths):
            continue
        try:
            dxr.check_gap(w, x, lengths, nl=nl, farnn=farnn, min_gap=MIN_GAP)
        except dxr.GapError:
            continue
        ref64 = dxr.step_on_table(w, x, lengths, labels, re, mode, c1, pi, nl=nl, farnn=farnn, dtype=torch.float64)
        ref32 = dxr.step_on_table(w, x, lengths, labels, re, mode, c1, pi, nl=nl, farnn=farnn, dtype=torch.float32)
        if well_drawn(ref32, ref64, x):
            return w, x, lengths, labels, re, ref32, ref64
    pytest.fail('no draw keeps the gap rule and is well drawn')


TEACHER_MAX_CASES = [   # S, R, K, V, B, L, nl, farnn, crf, prio, mode, c1, pi, full
    pytest.param(1, 7, 5, 9, 4, 3, 'tanh', 0, False, False, 'kd', 2.0, 0.3, False, id='S1'),
    pytest.param(16, 64, 5, 12, 5, 6, 'none', 1, False, True, 'pr', 2.0, 0.3, False, id='S16-R64-g1-prio'),     # unroll: tail only
    pytest.param(17, 65, 5, 12, 6, 8, 'tanh', 2, True, False, 'kd', 4.0, 0.1, False, id='S17-R65-g2-crf'),      # one round of 16
    pytest.param(18, 7, 5, 200, 4, 5, 'relu', 0, False, True, 'pr', 1.0, 0.0, False, id='S18-V200-pi0'),        # V > B L
    pytest.param(33, 64, 5, 20, 6, 7, 'relutanh', 2, False, False, 'kd', 2.0, 0.5, True, id='S33-full-g2'),     # two rounds; no pads
    pytest.param(192, 65, 5, 30, 5, 4, 'tanh', 1, True, True, 'pr', 2.0, 0.3, False, id='S192-g1-crf-prio'),    # a thread per state
    pytest.param(9, 7, 5, 40, 33, 8, 'tanh', 0, False, False, 'kd', 2.0, 0.3, False, id='BL264-two-chunks'),    # B L > OT_CH
]


@pytest.mark.parametrize('S,R,K,V,B,L,nl,farnn,crf,prio,mode,c1,pi,full', TEACHER_MAX_CASES)
def test_c_abi_vs_restatement(S, R, K, V, B, L, nl, farnn, crf, prio, mode, c1, pi, full):
    w, x, lengths, labels, re, ref32, ref64 = drawn_refs(S, R, K, V, B, L, nl, farnn, crf, prio, mode, c1, pi, S + R + K + farnn, full)
    valid = np.arange(L)[None, :] < lengths[:, None]
    only_pad = pad_only_words(x, lengths)
    res, _ = run_teacher_max(w, x, lengths, labels, re, mode, c1, pi, nl, farnn, crf)
    check_teacher(res, ref32, ref64, farnn, crf, x, 'teacher-max {} S{} R{} V{} farnn{} crf{}'.format(mode, S, R, V, farnn, int(crf)))
    assert (res['tags'][~valid] == -1).all() and (res['tags'][valid] >= 0).all()
    g = ref64[1]['Vgen']
    for t in only_pad:                                         # a word of the pads only: its row is the oracle's, not zero
        if np.abs(g[t]).max() > 0:
            assert np.abs(res['dVgen'][t]).max() > 0, t


# ---- 3. pi = 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['kd', 'pr'])
@pytest.mark.parametrize('farnn,crf,prio', [(0, False, False), (2, True, True), (1, False, True)])
def test_pi_one_is_the_plain_max_step(mode, farnn, crf, prio):
    """pi = 1: the tags are the plain max step's exactly, loss and gradients at the bars the sum test uses for the same
    statement (the chains still run L steps, their pad adjoints are zero; a pad-only word's row of dVgen is zero)"""
    S, R, K, V, B, L = 40, 30, 10, 50, 7, 9
    w, x, lengths, labels, re = teacher_case(S, R, K, V, B, L, 'tanh', farnn, crf, prio, seed=21)
    plain, _ = run_library(w, x, lengths, labels, 'tanh', farnn, crf, semiring='max')
    res, _ = run_teacher_max(w, x, lengths, labels, re, mode, 2.0, 1.0, 'tanh', farnn, crf)
    assert np.array_equal(res['tags'], plain['tags'])
    assert abs(res['loss'] - plain['loss']) < 2e-5 * max(1.0, abs(plain['loss']))
    for n in plain:
        if n not in ('tags', 'loss'):
            close(res[n], plain[n], n)
    valid = np.arange(L)[None, :] < lengths[:, None]
    for t in sorted(set(x[~valid]) - set(x[valid])):
        assert not res['dVgen'][t].any(), t


# ---- 4. / 5. the plain steps after a teacher step, and two teacher steps -----------------------------------------------------------
def test_plain_max_and_sum_steps_after_a_teacher_max_step_are_a_fresh_contexts():
    S, R, K, V, B, L = 40, 30, 10, 50, 7, 9
    w, x, lengths, labels, re = teacher_case(S, R, K, V, B, L, 'tanh', 2, True, False, seed=24)
    fresh_max, _ = run_library(w, x, lengths, labels, 'tanh', 2, True, semiring='max')
    fresh_sum, _ = run_library(w, x, lengths, labels, 'tanh', 2, True, semiring='sum')
    _, tc = run_teacher_max(w, x, lengths, labels, re, 'pr', 2.0, 0.3, 'tanh', 2, True)
    after_max, _ = run_library(w, x, lengths, labels, 'tanh', 2, True, tc=tc)
    tc.set_semiring('sum')
    after_sum, _ = run_library(w, x, lengths, labels, 'tanh', 2, True, tc=tc)
    same(after_max, fresh_max, ('tags',))
    same(after_sum, fresh_sum, ('tags', 'dS1', 'dS2', 'dW'))


@pytest.mark.parametrize('mode,crf', [('kd', False), ('pr', True)])
def test_two_teacher_max_steps_repeat(mode, crf):
    """within the decomposed step's own repeatability: its float atomics on dGV, dh0, dOsum and the products' sums stay, so
    only the tags are held to bit identity (as for the parent's plain max step)"""
    S, R, K, V, B, L = 40, 30, 10, 50, 7, 9
    w, x, lengths, labels, re = teacher_case(S, R, K, V, B, L, 'tanh', 1, crf, True, seed=23)
    a, tc = run_teacher_max(w, x, lengths, labels, re, mode, 2.0, 0.3, 'tanh', 1, crf)
    b, _ = run_teacher_max(w, x, lengths, labels, re, mode, 2.0, 0.3, 'tanh', 1, crf, tc=tc)
    same(a, b, ('tags',))


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def _refused(tc, w, x, lengths, labels, re, mode, c1, pi, max_entry):
    """one call of the named entry that must raise code -22 and leave every output as it was"""
    from re2nn_seq_amd import _lib
    dev = torch.device('cuda')
    wd = {n: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for n, v in w.items()}
    out = {'d' + n: torch.full_like(wd[n], 7.0) for n in OUT_NAMES}
    loss = torch.full((1,), 3.0, device=dev)
    tags = torch.full(x.shape, -7, dtype=torch.int32, device=dev)
    xd, ld, labd, red = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, lengths, labels, re))
    with pytest.raises(_lib.FarnnError) as e:
        tc.teacher_step({n: wd[n].data_ptr() for n in OUT_NAMES}, xd.data_ptr(), ld.data_ptr(), labd.data_ptr(), red.data_ptr(),
                        mode, c1, pi, x.shape[0], x.shape[1], max(int(lengths.sum()), 1),
                        dict({n: t.data_ptr() for n, t in out.items()}, loss=loss.data_ptr(), tags=tags.data_ptr()),
                        max_entry=max_entry)
    torch.cuda.synchronize()
    assert 'code -22' in str(e.value), str(e.value)
    assert float(loss) == 3.0 and bool((tags == -7).all()) and all(bool((t == 7.0).all()) for t in out.values())
    return str(e.value)


@pytest.mark.parametrize('mode,c1,pi,semiring,max_entry', [
    ('kd', 2.0, 0.3, 'sum', True),                            # the new entry on a sum context
    ('kd', 0.5, 0.3, 'max', True), ('pr', 2.0, 1.5, 'max', True), ('kd', 2.0, float('nan'), 'max', True), (3, 2.0, 0.3, 'max', True),
    ('kd', 2.0, 0.3, 'max', False),                           # the old entry on a max context: as before
])
def test_refusals_leave_the_outputs_untouched(mode, c1, pi, semiring, max_entry):
    S, R, K, V, B, L = 12, 8, 5, 20, 4, 6
    w, x, lengths, labels, re = teacher_case(S, R, K, V, B, L, 'tanh', 0, False, False, seed=25)
    tc = context(w, 'tanh', 0, False, semiring=semiring)
    msg = _refused(tc, w, x, lengths, labels, re, mode, c1, pi, max_entry)
    if semiring == 'max' and not max_entry:
        assert 'the max semiring has no KD / PR teacher (its kernels walk the valid positions only)' in msg
    # the context is still good for the step it is set to
    if semiring == 'max':
        run_teacher_max(w, x, lengths, labels, re, 'kd', 2.0, 0.3, 'tanh', 0, False, tc=tc)


def test_a_max_context_without_the_opt_in_goes_to_the_old_entry():
    from re2nn_seq_amd import _lib
    S, R, K, V, B, L = 12, 8, 5, 20, 4, 6
    w, x, lengths, labels, re = teacher_case(S, R, K, V, B, L, 'tanh', 0, False, False, seed=25)
    with pytest.raises(_lib.FarnnError, match='code -22'):
        run_teacher(w, x, lengths, labels, re, 'kd', 2.0, 0.3, 'tanh', 0, False, tc=context(w, 'tanh', 0, False, teacher_max=False))


# ---- 7. one epoch through the command line ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    from re2nn_seq_amd import synth
    root = str(tmp_path_factory.mktemp('data'))
    return synth.write_dataset_tree(root, dataset='ATIS-BIO', seed=4)


def test_one_epoch_through_the_command_line(tree, tmp_path, monkeypatch):
    """--train_mode max --marryup_type kd: the loss is finite; with the original loss's weight 1 it is the plain max run's;
    without the new switch the run is refused with today's text"""
    from re2nn_seq_amd import RE
    monkeypatch.setitem(RE.DEFAULT_RE_AUTOMATA, 'ATIS-BIO', tree['paths']['ID2'])      # the RE teacher's automaton: the tiny tree's
    # (the teacher's last column is cut where the reference's zero column goes: tests/test_gpu_decomp_teacher_train.py)
    full = RE.predict_by_RE
    monkeypatch.setattr(RE, 'predict_by_RE', lambda *a, **k: tuple(t[..., :-1] if i >= 3 else t for i, t in enumerate(full(*a, **k))))
    mx = ['--train_mode', 'max']
    extra = mx + ['--marryup_type', 'kd', '--c1_kdpr', '2']
    plain = epoch_loss(tree, tmp_path / 'plain', mx)
    bar = 2e-5 * max(1.0, abs(plain))
    one = epoch_loss(tree, tmp_path / 'one', extra + ['--c2_kdpr', '1'])
    half = epoch_loss(tree, tmp_path / 'half', extra + ['--c2_kdpr', '0.5'])
    print('plain max', plain, 'c2=1', one, 'c2=0.5', half)
    assert np.isfinite(half)
    assert abs(one - plain) <= bar
    assert abs(half - plain) > bar
    monkeypatch.delenv('RE2NN_DECOMP_TEACHER_MAX_TRAIN')
    with pytest.raises(NotImplementedError) as e:
        epoch_loss(tree, tmp_path / 'refused', extra + ['--c2_kdpr', '0.5'])
    assert str(e.value) == TODAY_MAX
