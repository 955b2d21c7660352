"""The HIP training step of the decomposed independent=1 model in the MAX semiring (FARNN_S_D_W_I, --train_mode max;
DESIGN.md, row f9): the model mirror against the captured configurations, the C-ABI after
farnn_decomp_ind1_train_set_semiring(MAX) against the float64 restatement (tests/decomp1_max_train_ref.py) under the arg-max
gap rule at the shape edges of the max kernels -- dh0 / dhT through the row-0 carry of onehot_max_bptt_carry_kernel among the
gradients of every case -- all-negative candidates, repeatability, switching semirings, Adam steps, tagging with the trained
weights, and the command line."""
import numpy as np
import pytest
import torch

import decomp1_max_train_ref as dmr
from decomp1_train_ref import badly_drawn
from test_decomp1_max_train_cpu import case, model
from test_decomp1_train_cpu import N_CASES, PARAMS, check_all_grads
from test_gpu_decomp1_train import _cli_argv, run_step_c_abi
from util import assert_float_path, present_words

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    monkeypatch.setenv('RE2NN_DECOMP_IND1_TRAIN', '1')
    monkeypatch.setenv('RE2NN_BUCKETED_MAX_TRAIN', '1')


def _ctx(c, semiring='max'):
    from re2nn_seq_amd import _lib
    p = c['p']
    V, R = p['Vgen'].shape
    C, RO = p['C_output'].shape
    return _lib.Decomp1TrainContext(V, p['S1'].shape[0], R, RO, C, nl=c['nl'], semiring=semiring)


@pytest.mark.parametrize('k', range(N_CASES))
def test_model_mirror_matches_the_reference_capture(k):
    cfg, inp, ref = case(k)
    m = model(k)
    x, lt, lab = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths']), torch.from_numpy(inp['labels'])
    m.train()
    loss, pred, true = m.forward_local(x, lab, lt, train=True)
    loss.backward()
    named = dict(m.named_parameters())
    assert set(named) == set(PARAMS)
    l64, g64, _ = dmr.step(dtype=torch.float64, **inp)
    assert_float_path(float(loss.detach()), ref['loss'], l64, err_msg='loss')
    present = present_words(inp['x'], inp['lengths'], inp['p']['V_embed'].shape[0])
    check_all_grads('decomp1 max capture c{}'.format(k), {n: t.grad.cpu().numpy() for n, t in named.items()}, ref['grads'], g64,
                    present)
    assert np.array_equal(pred.cpu().numpy(), ref['flat_pred'])


def make_case(V, S, R, RO, C, B, L, seed, lengths=None, priority=False, x=None, nl='relu'):
    """a signed real-valued case that keeps the gap rule (decomp1_max_train_ref.check_gap), drawn again (next seed) until the
    float64 restatement's gradients are live and the float32 restatement sits within a tenth of the bar
    (decomp1_train_ref.badly_drawn) -- conditions read off the restatement alone"""
    why = None
    for attempt in range(60):
        try:
            c = _draw(V, S, R, RO, C, B, L, seed + 1000 * attempt, lengths, priority, x, nl)
        except dmr.GapError as e:
            why = str(e)
            continue
        present = present_words(c['x'], c['lengths'], V)
        r32, r64 = dmr.step(dtype=torch.float32, **c), dmr.step(dtype=torch.float64, **c)
        why = badly_drawn(r32[1], r64[1], present)
        if why is None and not np.array_equal(r32[2], r64[2]):
            why = 'float32 and float64 decode differently'
        if why is None:
            c['_ref'] = (r32, r64)
            return c
    raise AssertionError('no live case in 60 draws: ' + str(why))


def _draw(V, S, R, RO, C, B, L, seed, lengths, priority, x, nl):
    rng = np.random.RandomState(seed)
    p = dmr.signed_base(V, S, R, RO, C, rng)
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
    dmr.check_gap(p, P, x, lengths, nl=nl)
    return dict(p=p, P=P, x=x, lengths=lengths, labels=labels, nl=nl)


def check_case(name, c, tc=None):
    (l32, g32, p32), (l64, g64, p64) = c['_ref']
    own = tc is None
    tc = _ctx(c) if own else tc
    try:
        loss, grads, tags = run_step_c_abi(c, tc=tc)
    finally:
        if own:
            tc.close()
    assert_float_path(loss, l32, l64, err_msg=name + ' loss')
    present = present_words(c['x'], c['lengths'], grads['Vgen'].shape[0])
    check_all_grads(name, grads, g32, g64, present)          # h0 and hT among them: the row-0 carry
    assert not grads['Vgen'][~present].any(), 'the row of an absent word is not zero'
    B, L = c['x'].shape
    valid = np.arange(L)[None, :] < np.clip(c['lengths'], 0, L)[:, None]
    assert (tags[~valid] == -1).all()
    assert np.array_equal(tags[valid], p64)
    return loss, grads, tags


# 64 | 65, 72 | 73, 96 | 97: where with_chain_slots changes the register-slot form of the chain kernels (8, 18, 24, 32 slots)
@pytest.mark.parametrize('k,S', list(enumerate([1, 3, 4, 5, 63, 64, 65, 71, 72, 73, 95, 96, 97, 127, 128])))
def test_state_counts_at_the_register_slot_edges(k, S):
    C, V = (5, 6) if S <= 73 else (2, 5)
    c = make_case(V, S, 6, 4, C, 4, 3, seed=100 + S, lengths=[3, 0, 2, 1], priority=k % 2 == 0,
                  nl=('relu', 'tanh', 'none', 'relutanh')[k % 4])
    check_case('decomp1 max S{}'.format(S), c)


@pytest.mark.parametrize('C,RO', [(2, 4), (65, 4), (5, 64), (5, 65)])
def test_label_counts_and_output_ranks_at_a_group_edge(C, RO):
    c = make_case(7, 5, 6, RO, C, 3, 4, seed=200 + C + RO, priority=C == 2, nl='tanh')
    check_case('decomp1 max C{} RO{}'.format(C, RO), c)


@pytest.mark.parametrize('V,B,L,lengths', [(1, 3, 3, [3, 1, 2]), (9, 2, 2, [2, 1]), (5, 4, 5, [0, 5, 2, 0]), (4, 3, 3, [0, 1, 0])])
def test_vocabulary_and_batch_edges(V, B, L, lengths):
    """one word only; absent words; an empty sequence beside full ones; a batch whose only valid sequence has length 1 (dhT is
    then the score adjoint alone: the backward chain has no step)"""
    c = make_case(V, 6, 5, 4, 3, B, L, seed=300 + V, lengths=lengths, nl='tanh')
    check_case('decomp1 max V{} B{} L{}'.format(V, B, L), c)


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
    c = make_case(V, 7, 5, 4, 3, B, L, seed=400 + n, lengths=lengths, x=x, nl='tanh')
    check_case('decomp1 max run{}'.format(n), c)


def test_all_negative_candidates_keep_a_real_index():
    """update_nonlinear none: a negative maximum stays a live state (under relu it would be cut to zero whichever candidate
    won).  Every factor positive but one word's row of Vgen negative: every candidate of every state at that word is negative,
    the zero of a padded row or register slot must not win (S = 5: three of eight slots are padding)"""
    rng = np.random.RandomState(17)
    V, S, R, RO, C, B, L = 4, 5, 3, 2, 3, 5, 3
    pos = lambda *sh: rng.choice(np.array([0.25, 0.5, 1.0], np.float32), size=sh)      # noqa: E731
    p = {'Vgen': pos(V, R), 'S1': pos(S, R), 'S2': pos(S, R), 'wildcard_mat': np.zeros((S, S), np.float32), 'C_output': pos(C, RO),
         'S1_output': pos(S, RO), 'S2_output': pos(S, RO), 'h0': np.full(S, 0.5, np.float32), 'hT': np.full(S, 0.5, np.float32)}
    p['Vgen'][2] = -p['Vgen'][2]
    x = rng.randint(0, V, size=(B, L)).astype(np.int64)
    x[:, 1] = 2
    c = dict(p=p, P=None, x=x, lengths=np.full(B, 3, np.int64), labels=rng.randint(0, C, size=(B, L)).astype(np.int64), nl='none')
    dmr.check_gap(p, None, x, c['lengths'], nl='none')
    c['_ref'] = (dmr.step(dtype=torch.float32, **c), dmr.step(dtype=torch.float64, **c))
    assert np.abs(c['_ref'][1][1]['h0']).max() > 0
    check_case('decomp1 max negative', c)


def test_two_max_steps_are_bit_identical_and_sum_after_max_is_the_fresh_sum_step():
    c = make_case(6, 71, 9, 5, 5, 6, 4, seed=21, priority=True, nl='relu')
    tc = _ctx(c)
    a = run_step_c_abi(c, tc=tc)
    b = run_step_c_abi(c, tc=tc)
    assert a[0] == b[0] and np.array_equal(a[2], b[2]) and all(np.array_equal(a[1][n], b[1][n]) for n in a[1])
    check_case('decomp1 max bitwise', c, tc=tc)
    tc.set_semiring('sum')
    s = run_step_c_abi(c, tc=tc)
    tc.close()
    fresh = run_step_c_abi(c)                                 # a context that never left the sum semiring
    assert s[0] == fresh[0] and np.array_equal(s[2], fresh[2]) and all(np.array_equal(s[1][n], fresh[1][n]) for n in s[1])
    assert not np.array_equal(s[1]['S1'], a[1]['S1']), 'badly drawn: the semiring changes nothing'


def test_set_semiring_refuses_other_values():
    from re2nn_seq_amd import _lib
    tc = _lib.Decomp1TrainContext(3, 4, 3, 2, 2, nl='relu')
    with pytest.raises(_lib.FarnnError) as e:
        _lib.check(_lib.load().farnn_decomp_ind1_train_set_semiring(tc._raw, 7), 'farnn_decomp_ind1_train_set_semiring')
    assert 'FARNN_SEMIRING_SUM or FARNN_SEMIRING_MAX' in str(e.value)
    tc.close()


def test_decompose_independent1_cli_trains_in_the_max_semiring_and_tags_with_the_trained_weights(tmp_path):
    """--method decompose --independent 1 --train_mode max --epoch 2 through train_epochs"""
    from re2nn_seq_amd import main as cli
    results, stats, res_path = cli.main(_cli_argv(tmp_path) + ['--train_mode', 'max'])
    steps = stats['train_step']
    assert len(steps) == 2 and all(s['tokens'] > 0 for s in steps)
    saved = cli.load_res(res_path)
    losses = [float(line.split('LOSS:')[1]) for line in saved['logger'].record if 'TRAIN' in line and 'LOSS:' in line]
    assert len(losses) == 2 and all(np.isfinite(losses))


def _adam_setup():
    """strictly positive, generic (all distinct) weights and tanh chains: no kink, and the maxima stay apart by far more than
    the gap after every optimizer step -- asserted on the float64 restatement's weights of every step"""
    from re2nn_seq_amd.farnn.model_decompose_independent import FARNN_S_D_W_I
    from test_decomp1_train_cpu import FLAGS
    from util import ns
    V, S, R, RO, C, D = 9, 5, 4, 3, 4, 3
    rng = np.random.RandomState(41)
    pos = lambda *s: (0.2 + 0.8 * rng.rand(*s)).astype(np.float32)      # noqa: E731
    Vm, S1, S2, W, Co, S1o, S2o = pos(V, R), pos(S, R), pos(S, R), pos(S, S) / 4, pos(C, RO), pos(S, RO), pos(S, RO)
    a = ns(independent=1, update_nonlinear='tanh', train_mode='max', **FLAGS)
    m = FARNN_S_D_W_I(V=Vm, S1=S1, S2=S2, C_output=Co, S1_output=S1o, S2_output=S2o, wildcard_mat=W,
                      wildcard_output=np.zeros((S, S), np.float32), final_vector=pos(S), start_vector=pos(S),
                      pretrained_word_embed=pos(V, D), priority_mat=None, args=a, o_idx=0)
    p0 = {n: np.ascontiguousarray(t.numpy(), dtype=np.float32) for n, t in m.state_dict().items() if n in PARAMS}
    batches = [(rng.randint(0, V, size=(6, 4)).astype(np.int64), rng.randint(1, 5, size=6).astype(np.int64),
                rng.randint(0, C, size=(6, 4)).astype(np.int64)) for _ in range(3)]
    return m, p0, batches


@pytest.mark.parametrize('native', [False, True])
def test_three_adam_steps_match_the_restatement(native):
    m, p0, batches = _adam_setup()
    kw = dict(P=None, batches=batches, trainable=set(PARAMS), nl='tanh', lr=0.01)
    p64 = dmr.adam_steps(p0, dtype=torch.float64, min_gap=2e-5, **kw)
    p32 = dmr.adam_steps(p0, dtype=torch.float32, **kw)
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
    m.eval()                                                  # the trained tensors return to the host attributes
    sd = m.state_dict()
    for n in PARAMS:
        assert_float_path(sd[n].numpy(), p32[n], p64[n], err_msg=n + ' after 3 Adam steps')
        assert np.abs(sd[n].numpy() - p0[n]).max() > 0, n


def test_tagging_after_max_training_reads_the_trained_weights_in_the_max_semiring():
    _, inp, _ = case(12)
    m = model(12)
    x, lt, lab = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths']), torch.from_numpy(inp['labels'])
    opt = torch.optim.Adam(list(m.enable_training().parameters()), lr=0.02, weight_decay=0)
    for _ in range(3):
        opt.zero_grad()
        loss, _, _ = m.forward_local(x, lab, lt, train=True)
        loss.backward()
        opt.step()
    _, after, _ = m.forward_local(x, lab, lt, train=False)
    sd = m.state_dict()
    assert np.abs(sd['S1'].numpy() - inp['p']['S1']).max() > 0
    fresh = model(12)                                         # --train_mode max: its handle is created with semiring='max'
    fresh.load_state_dict(sd)
    _, want, _ = fresh.forward_local(x, lab, lt, train=False)
    assert np.array_equal(after.numpy(), want.numpy())
