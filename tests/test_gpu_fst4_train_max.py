"""The HIP training step of the onehot FST in the MAX semiring (FARNN_S_O, --train_mode max): the C-ABI
after farnn_fst4_train_set_semiring(MAX) against the float64 restatement (tests/fst4_max_train_ref.py) under the arg-max gap
rule at the shape edges of the max kernels, the captured configurations, exact ties, all-negative candidates, repeatability,
switching semirings, Adam steps, and the command line."""
import numpy as np
import pytest
import torch

import fst4_max_train_ref as fmr
from test_fst4_max_train_cpu import N_CASES, case
from test_gpu_fst4_train import _cli_argv, run_step_c_abi
from util import assert_float_path, check_grad, ns, present_words

pytestmark = pytest.mark.gpu
KEYS = ('T4', 'W4', 'h0', 'hT', 'P', 'x', 'lengths', 'labels')


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    monkeypatch.setenv('RE2NN_ONEHOT_FST_TRAIN', '1')
    monkeypatch.setenv('RE2NN_BUCKETED_MAX_TRAIN', '1')


def _ctx(c, semiring='max', threshold=0.5, o_idx=0):
    from re2nn_seq_amd import _lib
    V, C, S, _ = c['T4'].shape
    return _lib.Fst4TrainContext(V, S, C, threshold=threshold, o_idx=o_idx, semiring=semiring)


def _model(inp, cfg):
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O
    V, C, S, _ = inp['T4'].shape
    pri = inp['P'][:-1, :-1] if cfg['use_priority'] else np.eye(C - 1)
    a = ns(independent=0, use_priority=cfg['use_priority'], train_wildcard=cfg['train_wildcard'], threshold=inp['threshold'],
           train_mode='max')
    return FARNN_S_O(inp['T4'], inp['W4'], np.zeros((S, S)), inp['hT'], inp['h0'], pri, a, o_idx=inp['o_idx'])


@pytest.mark.parametrize('k', range(N_CASES))
def test_c_abi_and_model_mirror_match_the_reference_capture(k):
    cfg, inp, ref = case(k)
    l64, g64, w64, _ = fmr.step(dtype=torch.float64, **inp)
    present = present_words(inp['x'], inp['lengths'], inp['T4'].shape[0])
    c = {n: inp[n] for n in KEYS}
    tc = _ctx(c, threshold=inp['threshold'], o_idx=inp['o_idx'])
    loss, dT4, dW4, tags = run_step_c_abi(c, tc=tc)
    tc.close()
    name = 'fst4 max capture c{}'.format(k)
    assert_float_path(loss, ref['loss'], l64, err_msg='loss')
    check_grad(name, 'dT4', dT4, ref['dT4'], g64, slices=0, present=present)
    if cfg['train_wildcard']:
        check_grad(name, 'dW4', dW4, ref['dW4'], w64)
    valid = np.arange(inp['x'].shape[1])[None, :] < inp['lengths'][:, None]
    assert np.array_equal(tags[valid], ref['flat_pred'])
    m = _model(inp, cfg)
    x, lt, lab = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths']), torch.from_numpy(inp['labels'])
    m.train()
    mloss, pred, _ = m.forward_local(x, lab, lt, train=True)
    mloss.backward()
    named = dict(m.named_parameters())
    assert set(named) == {'language_tensor'} | ({'wildcard_tensor'} if cfg['train_wildcard'] else set())
    assert_float_path(float(mloss.detach()), ref['loss'], l64, err_msg='loss')
    check_grad(name + ' mirror', 'dT4', named['language_tensor'].grad.cpu().numpy(), ref['dT4'], g64, slices=0, present=present)
    if cfg['train_wildcard']:
        check_grad(name + ' mirror', 'dW4', named['wildcard_tensor'].grad.cpu().numpy(), ref['dW4'], w64)
    assert np.array_equal(pred.cpu().numpy(), ref['flat_pred'])


def make_case(V, S, C, B, L, seed, lengths=None, priority=False, x=None):
    """a signed real-valued case that keeps the gap rule (fst4_max_train_ref.check_gap); drawn again (next seed) while the rule
    fails, while the float64 restatement's gradient is below 1e-3, or while the float32 restatement leaves a present word's
    block beyond a tenth of the bar from float64 -- conditions read off the restatement alone"""
    why = None
    for attempt in range(50):
        try:
            c = _draw(V, S, C, B, L, seed + 1000 * attempt, lengths, priority, x)
        except fmr.GapError as e:
            why = str(e)
            continue
        r32, r64 = fmr.step(dtype=torch.float32, **c), fmr.step(dtype=torch.float64, **c)
        sw = np.abs(r64[1]).reshape(V, -1).max(1)
        if np.abs(r64[1]).max() >= 1e-3 and (np.abs(r32[1] - r64[1]).reshape(V, -1).max(1) <= 1e-5 * sw).all() \
                and np.array_equal(r32[3], r64[3]):
            c['_ref'] = (r32, r64)
            return c
        why = 'dead or ill-conditioned'
    raise AssertionError('no live case in 50 draws: ' + str(why))


def _draw(V, S, C, B, L, seed, lengths, priority, x):
    rng = np.random.RandomState(seed)
    T4, W4, h0, hT = fmr.signed_base(V, S, C, rng)
    if lengths is None:
        lengths = rng.randint(1, L + 1, size=B)
        lengths[0] = L
    lengths = np.asarray(lengths, np.int64)
    x = rng.randint(0, V, size=(B, L)).astype(np.int64) if x is None else x
    labels = rng.randint(0, C, size=(B, L)).astype(np.int64)
    P = None
    if priority:
        P = np.eye(C, dtype=np.float32)
        P[rng.randint(0, C, 4), rng.randint(0, C, 4)] = -1.0
    fmr.check_gap(T4, W4, h0, hT, x, lengths)
    return dict(T4=T4, W4=W4, h0=h0, hT=hT, P=P, x=x, lengths=lengths, labels=labels)


def check_case(name, c, tc=None):
    kw = {k: c[k] for k in KEYS}
    if '_ref' not in c:
        c['_ref'] = (fmr.step(dtype=torch.float32, **kw), fmr.step(dtype=torch.float64, **kw))
    (l32, g32, w32, p32), (l64, g64, w64, p64) = c['_ref']
    own = tc is None
    tc = _ctx(c) if own else tc
    try:
        loss, dT4, dW4, tags = run_step_c_abi(kw, tc=tc)
    finally:
        if own:
            tc.close()
    assert_float_path(loss, l32, l64, err_msg=name + ' loss')
    present = present_words(c['x'], c['lengths'], dT4.shape[0])
    check_grad(name, 'dT4', dT4, g32, g64, slices=0, present=present)
    check_grad(name, 'dW4', dW4, w32, w64)
    assert not dT4[~present].any(), 'the block of an absent word is not zero'
    B, L = c['x'].shape
    valid = np.arange(L)[None, :] < np.clip(c['lengths'], 0, L)[:, None]
    assert (tags[~valid] == -1).all()
    assert np.array_equal(p32, p64), 'badly drawn: the restatement decodes differently in float32 and float64'
    assert np.array_equal(tags[valid], p64)
    return loss, dT4, dW4, tags


# 64 | 65, 72 | 73, 96 | 97: where with_chain_slots changes the register-slot form of the chain kernels (8, 18, 24, 32 slots)
@pytest.mark.parametrize('S', [1, 3, 4, 5, 63, 64, 65, 71, 72, 73, 95, 96, 97, 127, 128])
def test_state_counts_at_the_register_slot_edges(S):
    C, V = (3, 6) if S <= 73 else (2, 5)
    c = make_case(V, S, C, 4, 3, seed=100 + S, lengths=[3, 0, 2, 1], priority=S % 2 == 0)
    check_case('fst4 max S{}'.format(S), c)


@pytest.mark.parametrize('C', [2, 65])
def test_label_counts(C):
    c = make_case(7, 5, C, 3, 4, seed=200 + C, priority=C == 2)
    check_case('fst4 max C{}'.format(C), c)


@pytest.mark.parametrize('V,B,L,lengths', [(1, 3, 3, [3, 1, 2]), (9, 2, 2, [2, 1]), (5, 4, 5, [0, 5, 2, 0]), (4, 3, 3, [0, 1, 0])])
def test_vocabulary_and_batch_edges(V, B, L, lengths):
    """one word only; absent words; an empty sequence beside full ones; a batch whose only valid sequence has length 1"""
    c = make_case(V, 6, 3, B, L, seed=300 + V, lengths=lengths)
    check_case('fst4 max V{} B{} L{}'.format(V, B, L), c)


@pytest.mark.parametrize('n', [31, 32, 33, 65])
def test_a_word_at_the_edges_of_a_run_of_32_positions(n):
    """the OT_G run edges of onehot_max_dT_kernel: one run, a full run, two runs (partial tiles), three"""
    B, L, V = 35, 2, 3
    rng = np.random.RandomState(n)
    lengths = np.full(B, 2, np.int64)
    lengths[:4] = [1, 2, 1, 2]
    x = rng.randint(1, V, size=(B, L)).astype(np.int64)
    valid = np.arange(L)[None, :] < lengths[:, None]
    flat = np.flatnonzero(valid.reshape(-1))
    x.reshape(-1)[flat[::len(flat) // n][:n] if len(flat) // n > 1 else flat[:n]] = 0
    assert int((x[valid] == 0).sum()) == n
    c = make_case(V, 7, 3, B, L, seed=400 + n, lengths=lengths, x=x)
    check_case('fst4 max run{}'.format(n), c)


def _positive_case(V, S, C, B, L, seed, values):
    rng = np.random.RandomState(seed)
    T4 = rng.choice(np.asarray(values, np.float32), size=(V, C, S, S))
    W4 = np.zeros((C, S, S), np.float32)
    h0, hT = np.full(S, 0.5, np.float32), np.full(S, 0.5, np.float32)
    lengths = rng.randint(2, L + 1, size=B).astype(np.int64)
    x = rng.randint(0, V, size=(B, L)).astype(np.int64)
    labels = rng.randint(0, C, size=(B, L)).astype(np.int64)
    return dict(T4=T4, W4=W4, h0=h0, hT=hT, P=None, x=x, lengths=lengths, labels=labels)


def test_planted_exact_ties_go_to_the_first_index():
    """two values per label and constant initial vectors: M's entries take few values, most maxima are exact ties of several
    candidates (exact in both dtypes: the gap rule holds), and the restatement with the LAST maximal index gives another gradient"""
    c = _positive_case(5, 9, 2, 6, 4, 7, [0.25, 0.5])
    fmr.check_gap(*(c[k] for k in ('T4', 'W4', 'h0', 'hT', 'x', 'lengths')))
    g = fmr.step(dtype=torch.float64, **c)[1]
    last = fmr.step(dtype=torch.float64, fault='last', **c)[1]
    assert np.abs(g - last).max() > 1e-2 * np.abs(g).max(), 'badly drawn: no tie decides anything'
    check_case('fst4 max ties', c)


def test_all_negative_candidates_keep_a_real_index():
    """every entry of one word's blocks is negative and the states before it are positive: every candidate of every state is
    negative, the zero of a padded row or register slot must not win (S = 5: three of eight slots are padding)"""
    c = _positive_case(4, 5, 2, 5, 3, 11, [0.25, 0.5, 1.0])
    c['T4'][2] = -c['T4'][2]
    c['x'][c['x'] == 2] = 0
    c['x'][::2, 1] = 2                                      # every other sequence meets the negative word; the rest stay live
    c['lengths'][:] = 3
    fmr.check_gap(*(c[k] for k in ('T4', 'W4', 'h0', 'hT', 'x', 'lengths')))
    check_case('fst4 max negative', c)


def test_two_max_steps_are_bit_identical_and_sum_after_max_is_the_fresh_sum_step():
    c = make_case(6, 71, 3, 6, 4, seed=21, priority=True)
    kw = {k: c[k] for k in KEYS}
    tc = _ctx(c)
    a = run_step_c_abi(kw, tc=tc)
    b = run_step_c_abi(kw, tc=tc)
    assert a[0] == b[0] and all(np.array_equal(p, q) for p, q in zip(a[1:], b[1:]))
    check_case('fst4 max bitwise', c, tc=tc)
    tc.set_semiring('sum')
    s = run_step_c_abi(kw, tc=tc)
    tc.close()
    fresh = run_step_c_abi(kw)                                # a context that never left the sum semiring
    assert s[0] == fresh[0] and all(np.array_equal(p, q) for p, q in zip(s[1:], fresh[1:]))
    assert not np.array_equal(s[1], a[1]), 'badly drawn: the semiring changes nothing'


def test_set_semiring_refuses_other_values():
    from re2nn_seq_amd import _lib
    tc = _lib.Fst4TrainContext(3, 4, 2)
    with pytest.raises(_lib.FarnnError) as e:
        _lib.check(_lib.load().farnn_fst4_train_set_semiring(tc._raw, 7), 'farnn_fst4_train_set_semiring')
    assert 'FARNN_SEMIRING_SUM or FARNN_SEMIRING_MAX' in str(e.value)
    tc.close()
    with pytest.raises(ValueError):
        _lib.Fst4TrainContext(3, 4, 2, semiring='min')


@pytest.mark.parametrize('native', [False, True])
def test_three_adam_steps_match_the_restatement(native):
    """strictly positive, all distinct weights: every step keeps the gap rule, asserted on the float64 restatement's weights of
    every step.  torch.optim without, the library's optimizer with train_wildcard"""
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O
    V, S, C = 7, 5, 3
    rng = np.random.RandomState(33)
    T4 = (rng.permutation(V * C * S * S).reshape(V, C, S, S) + 1).astype(np.float32) / 1024
    W4 = (rng.permutation(C * S * S).reshape(C, S, S) + 1).astype(np.float32) / 2048 + 0.125   # three steps of at most lr leave it positive
    h0, hT = (np.arange(S) + 1).astype(np.float32) / 8, (np.arange(S)[::-1] + 1).astype(np.float32) / 8
    batches = []
    for _ in range(3):
        batches.append((rng.randint(0, V, size=(6, 4)).astype(np.int64), rng.randint(1, 5, size=6).astype(np.int64),
                        rng.randint(0, C, size=(6, 4)).astype(np.int64)))
    kw = dict(P=None, batches=batches, train_wildcard=native, lr=0.01)
    T64, W64 = fmr.adam_steps(T4, W4, h0, hT, dtype=torch.float64, min_gap=2e-5, **kw)
    T32, W32 = fmr.adam_steps(T4, W4, h0, hT, dtype=torch.float32, **kw)
    m = FARNN_S_O(T4, W4, np.zeros((S, S)), hT, h0, np.eye(C - 1), ns(independent=0, train_wildcard=int(native), train_mode='max'),
                  o_idx=0)
    m.enable_training()
    optim = torch.optim
    if native:
        from re2nn_seq_amd.farnn import optim
    opt = optim.Adam(list(m.parameters()), lr=0.01, weight_decay=0)
    for x, lengths, labels in batches:
        opt.zero_grad()
        loss, _, _ = m.forward_local(torch.from_numpy(x), torch.from_numpy(labels), torch.from_numpy(lengths))
        loss.backward()
        opt.step()
    sd = m.state_dict()
    assert_float_path(sd['language_tensor'], T32, T64, err_msg='language_tensor after 3 Adam steps')
    assert_float_path(sd['wildcard_tensor'], W32, W64, err_msg='wildcard_tensor after 3 Adam steps')
    assert np.abs(sd['language_tensor'] - T4).max() > 0


def test_fst_cli_trains_in_the_max_semiring(tmp_path):
    """--method onehot --independent 0 --train_mode max --epoch 2 through train_epochs"""
    from re2nn_seq_amd import main as cli
    results, stats, res_path = cli.main(_cli_argv(tmp_path) + ['--train_mode', 'max'])
    steps = stats['train_step']
    assert len(steps) == 2 and all(s['tokens'] > 0 for s in steps)
    saved = cli.load_res(res_path)
    losses = [float(line.split('LOSS:')[1]) for line in saved['logger'].record if 'TRAIN' in line and 'LOSS:' in line]
    assert len(losses) == 2 and all(np.isfinite(losses))


def test_tagging_after_max_training_reads_the_trained_weights_in_the_max_semiring():
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O
    c = _positive_case(6, 7, 3, 8, 5, 5, [0.125, 0.25, 0.5, 1.0])
    S = 7
    a = ns(independent=0, train_mode='max')
    m = FARNN_S_O(c['T4'], c['W4'], np.zeros((S, S)), c['hT'], c['h0'], np.eye(2), a, o_idx=0)
    x, lt, lab = torch.from_numpy(c['x']), torch.from_numpy(c['lengths']), torch.from_numpy(c['labels'])
    opt = torch.optim.Adam(list(m.enable_training().parameters()), lr=0.05, weight_decay=0)
    for _ in range(3):
        opt.zero_grad()
        loss, _, _ = m.forward_local(x, lab, lt, train=True)
        loss.backward()
        opt.step()
    _, after, _ = m.forward_local(x, lab, lt, train=False)
    sd = m.state_dict()
    assert np.abs(sd['language_tensor'] - c['T4']).max() > 0
    fresh = FARNN_S_O(sd['language_tensor'], sd['wildcard_tensor'], np.zeros((S, S)), c['hT'], c['h0'], np.eye(2), a, o_idx=0)
    _, want, _ = fresh.forward_local(x, lab, lt, train=False)
    assert np.array_equal(after.numpy(), want.numpy())
