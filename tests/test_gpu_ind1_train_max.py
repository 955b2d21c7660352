"""The HIP training step of the onehot independent=1 model in the MAX semiring (FARNN_S_O_I, --train_mode max; DESIGN.md, row
f8): the C-ABI after farnn_ind1_train_set_semiring(MAX) against the float64 restatement (tests/ind1_max_train_ref.py) under
the arg-max gap rule at the shape edges of the max kernels, the captured configurations, exact ties, all-negative candidates,
repeatability, switching semirings, Adam steps, and the command line."""
import numpy as np
import pytest
import torch

import ind1_max_train_ref as imr
from test_gpu_ind1_train import _cli_argv, run_step_c_abi
from test_ind1_max_train_cpu import N_CASES, case
from util import assert_float_path, check_grad, ns, present_words

pytestmark = pytest.mark.gpu
KEYS = ('T', 'W', 'O', 'h0', 'hT', 'P', 'x', 'lengths', 'labels', 'mask')


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    monkeypatch.setenv('RE2NN_ONEHOT_IND1_TRAIN', '1')
    monkeypatch.setenv('RE2NN_BUCKETED_MAX_TRAIN', '1')


def _ctx(c, semiring='max', threshold=0.5, o_idx=0):
    from re2nn_seq_amd import _lib
    V, S, _ = c['T'].shape
    return _lib.Ind1TrainContext(V, S, c['O'].shape[0], mask_by_output=c['mask'], threshold=threshold, o_idx=o_idx,
                                 semiring=semiring)


def _model(inp, cfg):
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I
    C = inp['O'].shape[0]
    pri = inp['P'][:-1, :-1] if cfg['use_priority'] else np.eye(C - 1)
    a = ns(independent=cfg['independent'], use_priority=cfg['use_priority'], threshold=inp['threshold'], train_mode='max')
    return FARNN_S_O_I(inp['T'], inp['O'], inp['W'], None, inp['hT'], inp['h0'], pri, a, o_idx=inp['o_idx'])


@pytest.mark.parametrize('k', range(N_CASES))
def test_c_abi_and_model_mirror_match_the_reference_capture(k):
    cfg, inp, ref = case(k)
    l64, g64, _ = imr.step(dtype=torch.float64, **inp)
    present = present_words(inp['x'], inp['lengths'], inp['T'].shape[0])
    c = {n: inp[n] for n in KEYS}
    tc = _ctx(c, threshold=inp['threshold'], o_idx=inp['o_idx'])
    loss, dT, tags = run_step_c_abi(c, tc=tc)
    tc.close()
    assert_float_path(loss, ref['loss'], l64, err_msg='loss')
    check_grad('ind1 max capture c{}'.format(k), 'dT', dT, ref['dT'], g64, slices=0, present=present)
    valid = np.arange(inp['x'].shape[1])[None, :] < inp['lengths'][:, None]
    assert np.array_equal(tags[valid], ref['flat_pred'])
    m = _model(inp, cfg)
    x, lt, lab = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths']), torch.from_numpy(inp['labels'])
    m.train()
    mloss, pred, _ = m.forward_local(x, lab, lt, train=True)
    mloss.backward()
    assert_float_path(float(mloss.detach()), ref['loss'], l64, err_msg='loss')
    check_grad('ind1 max mirror c{}'.format(k), 'dT', dict(m.named_parameters())['language_tensor'].grad.cpu().numpy(), ref['dT'],
               g64, slices=0, present=present)
    assert np.array_equal(pred.cpu().numpy(), ref['flat_pred'])


def make_case(V, S, C, B, L, seed, lengths=None, priority=False, x=None, mask=False):
    """a signed real-valued case that keeps the gap rule (ind1_max_train_ref.check_gap); drawn again (next seed) while the rule
    fails, while the float64 restatement's gradient is below 1e-3, or while the float32 restatement leaves a present word's
    block beyond a tenth of the bar from float64 -- conditions read off the restatement alone"""
    why = None
    for attempt in range(50):
        try:
            c = _draw(V, S, C, B, L, seed + 1000 * attempt, lengths, priority, x, mask)
        except imr.GapError as e:
            why = str(e)
            continue
        r32, r64 = imr.step(dtype=torch.float32, **c), imr.step(dtype=torch.float64, **c)
        sw = np.abs(r64[1]).reshape(V, -1).max(1)
        if np.abs(r64[1]).max() >= 1e-3 and (np.abs(r32[1] - r64[1]).reshape(V, -1).max(1) <= 1e-5 * sw).all() \
                and np.array_equal(r32[2], r64[2]):
            c['_ref'] = (r32, r64)
            return c
        why = 'dead or ill-conditioned'
    raise AssertionError('no live case in 50 draws: ' + str(why))


def _draw(V, S, C, B, L, seed, lengths, priority, x, mask):
    rng = np.random.RandomState(seed)
    T, W, O, h0, hT = imr.signed_base(V, S, C, rng)
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
    imr.check_gap(T, W, O, h0, hT, x, lengths, mask=mask)
    return dict(T=T, W=W, O=O, h0=h0, hT=hT, P=P, x=x, lengths=lengths, labels=labels, mask=mask)


def check_case(name, c, tc=None):
    if '_ref' not in c:
        c['_ref'] = (imr.step(dtype=torch.float32, **{k: c[k] for k in KEYS}), imr.step(dtype=torch.float64, **{k: c[k] for k in KEYS}))
    (l32, g32, p32), (l64, g64, p64) = c['_ref']
    own = tc is None
    tc = _ctx(c) if own else tc
    try:
        loss, dT, tags = run_step_c_abi({k: c[k] for k in KEYS}, tc=tc)
    finally:
        if own:
            tc.close()
    assert_float_path(loss, l32, l64, err_msg=name + ' loss')
    present = present_words(c['x'], c['lengths'], dT.shape[0])
    check_grad(name, 'dT', dT, g32, g64, slices=0, present=present)
    assert not dT[~present].any(), 'the block of an absent word is not zero'
    B, L = c['x'].shape
    valid = np.arange(L)[None, :] < np.clip(c['lengths'], 0, L)[:, None]
    assert (tags[~valid] == -1).all()
    assert np.array_equal(p32, p64), 'badly drawn: the restatement decodes differently in float32 and float64'
    assert np.array_equal(tags[valid], p64)
    return loss, dT, tags


# 64 | 65, 72 | 73, 96 | 97: where with_chain_slots changes the register-slot form of the chain kernels (8, 18, 24, 32 slots)
@pytest.mark.parametrize('k,S', list(enumerate([1, 3, 4, 5, 63, 64, 65, 71, 72, 73, 95, 96, 97, 127, 128])))
def test_state_counts_at_the_register_slot_edges(k, S):
    C, V = (5, 6) if S <= 73 else (2, 5)
    c = make_case(V, S, C, 4, 3, seed=100 + S, lengths=[3, 0, 2, 1], priority=k % 2 == 0, mask=(k // 2) % 2 == 1)
    check_case('ind1 max S{}'.format(S), c)


@pytest.mark.parametrize('C', [2, 65])
def test_label_counts(C):
    c = make_case(7, 5, C, 3, 4, seed=200 + C, priority=C == 2, mask=C == 65)
    check_case('ind1 max C{}'.format(C), c)


@pytest.mark.parametrize('V,B,L,lengths', [(1, 3, 3, [3, 1, 2]), (9, 2, 2, [2, 1]), (5, 4, 5, [0, 5, 2, 0]), (4, 3, 3, [0, 1, 0])])
def test_vocabulary_and_batch_edges(V, B, L, lengths):
    """one word only; absent words; an empty sequence beside full ones; a batch whose only valid sequence has length 1"""
    c = make_case(V, 6, 3, B, L, seed=300 + V, lengths=lengths, mask=V == 9)
    check_case('ind1 max V{} B{} L{}'.format(V, B, L), c)


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
    c = make_case(V, 7, 3, B, L, seed=400 + n, lengths=lengths, x=x, mask=n == 33)
    check_case('ind1 max run{}'.format(n), c)


def _positive_case(V, S, C, B, L, seed, values, mask=False):
    rng = np.random.RandomState(seed)
    T = rng.choice(np.asarray(values, np.float32), size=(V, S, S))
    W = np.zeros((S, S), np.float32)
    O = rng.choice(np.array([0.5, 1.0], np.float32), size=(C, S, S))
    h0, hT = np.full(S, 0.5, np.float32), np.full(S, 0.5, np.float32)
    lengths = rng.randint(2, L + 1, size=B).astype(np.int64)
    x = rng.randint(0, V, size=(B, L)).astype(np.int64)
    labels = rng.randint(0, C, size=(B, L)).astype(np.int64)
    return dict(T=T, W=W, O=O, h0=h0, hT=hT, P=None, x=x, lengths=lengths, labels=labels, mask=mask)


def test_planted_exact_ties_go_to_the_first_index():
    """two values only and constant initial vectors: most maxima are exact ties of several candidates (exact in both dtypes: the
    gap rule holds), and the restatement with the LAST maximal index gives another gradient"""
    c = _positive_case(5, 9, 3, 6, 4, 7, [0.5, 1.0])
    imr.check_gap(*(c[k] for k in ('T', 'W', 'O', 'h0', 'hT', 'x', 'lengths')))
    g = imr.step(dtype=torch.float64, **c)[1]
    last = imr.step(dtype=torch.float64, fault='last', **c)[1]
    assert np.abs(g - last).max() > 1e-2 * np.abs(g).max(), 'badly drawn: no tie decides anything'
    check_case('ind1 max ties', c)


def test_all_negative_candidates_keep_a_real_index():
    """every entry of one word's block is negative and the states before it are positive: every candidate of every state is
    negative, the zero of a padded row or register slot must not win (S = 5: three of eight slots are padding)"""
    c = _positive_case(4, 5, 3, 5, 3, 11, [0.25, 0.5, 1.0])
    c['T'][2] = -c['T'][2]
    c['x'][c['x'] == 2] = 0
    c['x'][::2, 1] = 2                                      # every other sequence meets the negative word; the rest stay live
    c['lengths'][:] = 3
    imr.check_gap(*(c[k] for k in ('T', 'W', 'O', 'h0', 'hT', 'x', 'lengths')))
    check_case('ind1 max negative', c)


def test_two_max_steps_are_bit_identical_and_sum_after_max_is_the_fresh_sum_step():
    c = make_case(6, 71, 5, 6, 4, seed=21, priority=True, mask=True)
    kw = {k: c[k] for k in KEYS}
    tc = _ctx(c)
    a = run_step_c_abi(kw, tc=tc)
    b = run_step_c_abi(kw, tc=tc)
    assert a[0] == b[0] and all(np.array_equal(p, q) for p, q in zip(a[1:], b[1:]))
    check_case('ind1 max bitwise', c, tc=tc)
    tc.set_semiring('sum')
    s = run_step_c_abi(kw, tc=tc)
    tc.close()
    fresh = run_step_c_abi(kw)                                # a context that never left the sum semiring
    assert s[0] == fresh[0] and all(np.array_equal(p, q) for p, q in zip(s[1:], fresh[1:]))
    assert not np.array_equal(s[1], a[1]), 'badly drawn: the semiring changes nothing'


def test_set_semiring_refuses_other_values():
    from re2nn_seq_amd import _lib
    tc = _lib.Ind1TrainContext(3, 4, 2)
    with pytest.raises(_lib.FarnnError) as e:
        _lib.check(_lib.load().farnn_ind1_train_set_semiring(tc._raw, 7), 'farnn_ind1_train_set_semiring')
    assert 'FARNN_SEMIRING_SUM or FARNN_SEMIRING_MAX' in str(e.value)
    tc.close()
    with pytest.raises(ValueError):
        _lib.Ind1TrainContext(3, 4, 2, semiring='min')


@pytest.mark.parametrize('native', [False, True])
def test_three_adam_steps_match_the_restatement(native):
    """strictly positive weights (no relu near its kink after a step), distinct enough that every step keeps the gap rule: asserted
    on the float64 restatement's weights of every step.  torch.optim with independent = 1, the library's with independent = 2"""
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I
    V, S, C = 9, 5, 4
    mask = native
    rng = np.random.RandomState(31)
    T = (rng.permutation(V * S * S).reshape(V, S, S) + 1).astype(np.float32) / 256          # all distinct
    W = np.zeros((S, S), np.float32)
    O = rng.choice(np.array([0.25, 0.5, 1.0], np.float32), size=(C, S, S))
    h0, hT = (np.arange(S) + 1).astype(np.float32) / 8, (np.arange(S)[::-1] + 1).astype(np.float32) / 8
    batches = []
    for _ in range(3):
        batches.append((rng.randint(0, V, size=(6, 4)).astype(np.int64), rng.randint(1, 5, size=6).astype(np.int64),
                        rng.randint(0, C, size=(6, 4)).astype(np.int64)))
    kw = dict(P=None, batches=batches, mask=mask, lr=0.01)
    T64 = imr.adam_steps(T, W, O, h0, hT, dtype=torch.float64, min_gap=2e-5, **kw)
    T32 = imr.adam_steps(T, W, O, h0, hT, dtype=torch.float32, **kw)
    m = FARNN_S_O_I(T, O, W, None, hT, h0, np.eye(C - 1), ns(independent=2 if mask else 1, train_mode='max'), o_idx=0)
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
    assert np.abs(sd['language_tensor'] - T).max() > 0


def test_ind1_cli_trains_in_the_max_semiring_and_tags_with_the_trained_weights(tmp_path):
    """--method onehot --independent 1 --train_mode max --epoch 2 through train_epochs; then forward_local(train=False) on the
    trained model equals a max-semiring handle created from the synced tensors"""
    from re2nn_seq_amd import main as cli
    results, stats, res_path = cli.main(_cli_argv(tmp_path) + ['--train_mode', 'max'])
    steps = stats['train_step']
    assert len(steps) == 2 and all(s['tokens'] > 0 for s in steps)
    saved = cli.load_res(res_path)
    losses = [float(line.split('LOSS:')[1]) for line in saved['logger'].record if 'TRAIN' in line and 'LOSS:' in line]
    assert len(losses) == 2 and all(np.isfinite(losses))


def test_tagging_after_max_training_reads_the_trained_weights_in_the_max_semiring():
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I
    c = _positive_case(6, 7, 4, 8, 5, 5, [0.125, 0.25, 0.5, 1.0])
    a = ns(independent=1, train_mode='max')
    m = FARNN_S_O_I(c['T'], c['O'], c['W'], None, c['hT'], c['h0'], np.eye(3), a, o_idx=0)
    x, lt, lab = torch.from_numpy(c['x']), torch.from_numpy(c['lengths']), torch.from_numpy(c['labels'])
    opt = torch.optim.Adam(list(m.enable_training().parameters()), lr=0.05, weight_decay=0)
    for _ in range(3):
        opt.zero_grad()
        loss, _, _ = m.forward_local(x, lab, lt, train=True)
        loss.backward()
        opt.step()
    _, after, _ = m.forward_local(x, lab, lt, train=False)
    sd = m.state_dict()
    assert np.abs(sd['language_tensor'] - c['T']).max() > 0
    fresh = FARNN_S_O_I(sd['language_tensor'], sd['output_tensor'], sd['wildcard_mat'], None, c['hT'], c['h0'], np.eye(3), a, o_idx=0)
    _, want, _ = fresh.forward_local(x, lab, lt, train=False)
    assert np.array_equal(after.numpy(), want.numpy())
