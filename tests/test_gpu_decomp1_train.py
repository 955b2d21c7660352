"""The HIP training step of the decomposed independent=1 model (FARNN_S_D_W_I): the model mirror against
the loss / gradients / predictions captured from the reference, the C-ABI against the torch restatement
(tests/decomp1_train_ref.py) at the shape edges of its kernels, its refusals, Adam steps on the device, and the command
line."""
import numpy as np
import pytest
import torch

import decomp1_train_ref as dtr
from test_decomp1_train_cpu import N_CASES, PARAMS, REFUSAL, case, check_all_grads, model
from util import assert_float_path, present_words

pytestmark = pytest.mark.gpu
GUARD = 64
NAMES = ('Vgen', 'S1', 'S2', 'wildcard_mat', 'C_output', 'S1_output', 'S2_output', 'h0', 'hT')     # the C-ABI's order
ABI = dict(zip(NAMES, ('Vgen', 'S1', 'S2', 'W', 'C', 'S1o', 'S2o', 'h0', 'hT')))


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    monkeypatch.setenv('RE2NN_DECOMP_IND1_TRAIN', '1')


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
    l64, g64, _ = dtr.step(dtype=torch.float64, **inp)
    assert_float_path(float(loss.detach()), ref['loss'], l64, err_msg='loss')
    present = present_words(inp['x'], inp['lengths'], inp['p']['V_embed'].shape[0])
    check_all_grads('decomp1 capture c{}'.format(k), {n: t.grad.cpu().numpy() for n, t in named.items()}, ref['grads'], g64, present)
    assert np.array_equal(pred.cpu().numpy(), ref['flat_pred'])
    assert true.shape == pred.shape


@pytest.mark.parametrize('flags', [dict(), dict(train_wildcard=0), dict(train_wildcard_wildcard=0, train_h0=0),
                                   dict(train_hT=0, train_V_embed=0, train_word_embed=0, train_beta=0)])
def test_named_parameters_follow_the_train_flags(flags):
    """the tensors without the flag get no gradient and are not parameters; the others' gradients do not change"""
    _, inp, _ = case(12)
    m, full = model(12, **flags), model(12)
    x, lt, lab = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths']), torch.from_numpy(inp['labels'])
    grads = []
    for mm in (m, full):
        loss, _, _ = mm.forward_local(x, lab, lt, train=True)
        loss.backward()
        grads.append({n: t.grad.cpu().numpy() for n, t in mm.named_parameters()})
    off = {'train_wildcard': ('C_output', 'S1_output', 'S2_output'), 'train_wildcard_wildcard': ('wildcard_mat',),
           'train_h0': ('h0',), 'train_hT': ('hT',), 'train_V_embed': ('V_embed',), 'train_word_embed': ('embedding.weight',),
           'train_beta': ('beta_vec',)}
    want = set(PARAMS) - {n for f in flags for n in off[f]}
    assert set(grads[0]) == want and 'wildcard_output' not in grads[1]
    for n in want:
        assert np.array_equal(grads[0][n], grads[1][n]), n


def make_case(V, S, R, RO, C, B, L, seed, lengths=None, priority=False, x=None, nl='relu', need_osum_paths=False):
    """a signed real-valued case that keeps the gap rule, drawn again (next seed) until the float64 restatement's gradients
    are live and the float32 restatement sits within a tenth of the bar (decomp1_train_ref.badly_drawn) -- conditions read off
    the restatement alone"""
    why = None
    for attempt in range(60):
        try:
            c = _draw(V, S, R, RO, C, B, L, seed + 1000 * attempt, lengths, priority, x, nl)
        except dtr.GapError as e:
            why = str(e)
            continue
        present = present_words(c['x'], c['lengths'], V)
        r32, r64 = dtr.step(dtype=torch.float32, **c), dtr.step(dtype=torch.float64, **c)
        why = dtr.badly_drawn(r32[1], r64[1], present)
        if why is None and not np.array_equal(r32[2], r64[2]):
            why = 'float32 and float64 decode differently'
        if why is None and need_osum_paths:
            cut = dtr.step(dtype=torch.float64, detach_chains=True, **c)[1]
            if any(np.abs(r64[1][n] - cut[n]).max() <= 1e-3 * np.abs(r64[1][n]).max() for n in ('C_output', 'S1_output', 'S2_output')):
                why = 'the chains carry nothing into the output factors'
        if why is None:
            c['_ref'] = (r32, r64)
            return c
    raise AssertionError('no live case in 60 draws: ' + str(why))


def _draw(V, S, R, RO, C, B, L, seed, lengths, priority, x, nl):
    rng = np.random.RandomState(seed)
    p = dtr.signed_base(V, S, R, RO, C, rng)
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
    dtr.check_gap(p, P, x, lengths, nl=nl)
    return dict(p=p, P=P, x=x, lengths=lengths, labels=labels, nl=nl)


def run_step_c_abi(c, tc=None, threshold=0.5, o_idx=0):
    """farnn_decomp_ind1_train_step on pre-filled outputs with guard elements around every output; returns (loss, grads, tags)
    and asserts that the guards are untouched"""
    from re2nn_seq_amd import _lib
    dev = torch.device('cuda', 0)
    p = c['p']
    V, R = p['Vgen'].shape
    S = p['S1'].shape[0]
    C, RO = p['C_output'].shape
    own = tc is None
    if own:
        tc = _lib.Decomp1TrainContext(V, S, R, RO, C, nl=c['nl'], threshold=threshold, o_idx=o_idx, device=0)
    try:
        w = {n: torch.from_numpy(np.ascontiguousarray(p[n], dtype=np.float32)).to(dev) for n in NAMES}
        P = None if c['P'] is None else torch.from_numpy(np.ascontiguousarray(c['P'], dtype=np.float32)).to(dev)
        x, lengths, labels = (torch.from_numpy(np.ascontiguousarray(c[n])).to(dev) for n in ('x', 'lengths', 'labels'))
        B, L = c['x'].shape
        bufs = {n: torch.full((w[n].numel() + 2 * GUARD,), 7.0, device=dev) for n in NAMES}
        tags = torch.full((B * L + 2 * GUARD,), 77, dtype=torch.int32, device=dev)
        loss = torch.full((1 + 2 * GUARD,), 3.0, device=dev)
        out = {'d' + ABI[n]: t.data_ptr() + GUARD * 4 for n, t in bufs.items()}
        out.update(loss=loss.data_ptr() + GUARD * 4, tags=tags.data_ptr() + GUARD * 4)
        tc.step(dict({ABI[n]: t.data_ptr() for n, t in w.items()}, P=None if P is None else P.data_ptr()), x.data_ptr(),
                lengths.data_ptr(), labels.data_ptr(), B, L, int(np.clip(c['lengths'], 0, L).sum()), out)
        torch.cuda.synchronize()
        h = {n: t.cpu().numpy() for n, t in bufs.items()}
        ht, hl = tags.cpu().numpy(), loss.cpu().numpy()
        for n in NAMES:
            assert (h[n][:GUARD] == 7.0).all() and (h[n][-GUARD:] == 7.0).all(), 'guard elements around d{} overwritten'.format(n)
        assert (ht[:GUARD] == 77).all() and (ht[-GUARD:] == 77).all(), 'guard elements around tags overwritten'
        assert (hl[:GUARD] == 3.0).all() and (hl[-GUARD:] == 3.0).all(), 'guard elements around loss overwritten'
        return float(hl[GUARD]), {n: h[n][GUARD:-GUARD].reshape(p[n].shape) for n in NAMES}, ht[GUARD:-GUARD].reshape(B, L)
    finally:
        if own:
            tc.close()


def check_case(name, c):
    (l32, g32, p32), (l64, g64, p64) = c['_ref']
    loss, grads, tags = run_step_c_abi(c)
    assert_float_path(loss, l32, l64, err_msg=name + ' loss')
    present = present_words(c['x'], c['lengths'], grads['Vgen'].shape[0])
    check_all_grads(name, grads, g32, g64, present)
    assert not grads['Vgen'][~present].any(), 'the row of an absent word is not zero'
    B, L = c['x'].shape
    valid = np.arange(L)[None, :] < np.clip(c['lengths'], 0, L)[:, None]
    assert (tags[~valid] == -1).all()
    assert np.array_equal(tags[valid], p64)
    return loss, grads, tags


@pytest.mark.parametrize('k,S', list(enumerate([1, 3, 4, 5, 63, 64, 65, 71, 104, 127, 128])))
def test_state_counts_at_the_chunk_and_row_share_edges(k, S):
    C, V = (5, 6) if S <= 71 else (2, 5)
    c = make_case(V, S, 6, 4, C, 4, 3, seed=100 + S, lengths=[3, 0, 2, 1], priority=k % 2 == 0,
                  nl=('relu', 'none', 'tanh', 'relutanh')[k % 4])
    check_case('decomp1 S{}'.format(S), c)


@pytest.mark.parametrize('R', [1, 3, 4, 5, 31, 32, 33, 64, 65, 250])
def test_ranks_at_the_tile_edges(R):
    c = make_case(7, 5, R, 4, 4, 3, 4, seed=200 + R, priority=R % 2 == 0, nl='relu' if R % 3 else 'tanh')
    check_case('decomp1 R{}'.format(R), c)


@pytest.mark.parametrize('RO', [1, 4, 5, 64, 65, 80])
def test_output_ranks(RO):
    c = make_case(7, 5, 6, RO, 4, 3, 4, seed=300 + RO, priority=RO % 2 == 0, nl='relu' if RO % 3 else 'none')
    check_case('decomp1 RO{}'.format(RO), c)


@pytest.mark.parametrize('C', [2, 5, 64, 65])
def test_label_counts(C):
    c = make_case(7, 5, 6, 5, C, 3, 4, seed=400 + C, priority=C == 5)
    check_case('decomp1 C{}'.format(C), c)


def test_the_largest_label_count_and_the_refused_sizes():
    from re2nn_seq_amd import _lib
    c = make_case(2, 1, 2, 2, 2400, 2, 2, seed=5, nl='none')
    check_case('decomp1 C2400', c)
    for dims, word in (((2, 1, 2, 2, 2401), 'score columns'), ((4, 129, 3, 3, 3), '128 states'),
                       ((2, 128, 1 << 17, 2, 2), 'rank R'), ((2, 128, 2, 1 << 17, 2), 'output rank R_O')):
        with pytest.raises(_lib.FarnnError) as e:
            _lib.Decomp1TrainContext(*dims)
        assert word in str(e.value)
    _lib.Decomp1TrainContext(2, 128, (1 << 17) - 1, (1 << 17) - 1, 2).close()      # the largest ranks create accepts at S = 128


@pytest.mark.parametrize('nl', ['none', 'relu', 'tanh', 'relutanh'])
def test_every_nonlinearity_and_both_osum_paths(nl):
    c = make_case(6, 71, 8, 5, 5, 5, 4, seed=500, priority=True, nl=nl, need_osum_paths=True)
    check_case('decomp1 nl {}'.format(nl), c)


@pytest.mark.parametrize('V,B,L,lengths', [(1, 3, 3, [3, 1, 2]), (9, 2, 2, [2, 1]), (4, 1, 1, [1]), (5, 4, 5, [0, 5, 2, 0])])
def test_vocabulary_and_batch_edges(V, B, L, lengths):
    """one word only; absent words (dVgen rows exactly zero over the pre-filled buffer); a single position; zero-length
    beside full-length sequences"""
    c = make_case(V, 6, 5, 4, 3, B, L, seed=600 + V, lengths=lengths)
    _, grads, _ = check_case('decomp1 V{} B{} L{}'.format(V, B, L), c)
    present = present_words(c['x'], c['lengths'], V)
    assert not grads['Vgen'][~present].any()
    if V == 9:
        assert (~present).any()


@pytest.mark.parametrize('n', [31, 32, 33, 65])
def test_a_word_at_the_edges_of_a_run_of_32_positions(n):
    B, L, V = 35, 2, 3
    rng = np.random.RandomState(n)
    lengths = np.full(B, 2, np.int64)
    lengths[:4] = [1, 2, 1, 2]
    x = rng.randint(1, V, size=(B, L)).astype(np.int64)
    valid = np.arange(L)[None, :] < lengths[:, None]
    flat = np.flatnonzero(valid.reshape(-1))
    assert len(flat) >= n
    x.reshape(-1)[flat[::len(flat) // n][:n] if len(flat) // n > 1 else flat[:n]] = 0
    assert int((x[valid] == 0).sum()) == n
    c = make_case(V, 7, 5, 6, 3, B, L, seed=700 + n, lengths=lengths, x=x)
    check_case('decomp1 run{}'.format(n), c)


def test_two_steps_on_one_context_are_bit_identical():
    from re2nn_seq_amd import _lib
    c = make_case(6, 71, 9, 5, 5, 6, 4, seed=21, priority=True)
    tc = _lib.Decomp1TrainContext(6, 71, 9, 5, 5, nl='relu')
    a = run_step_c_abi(c, tc=tc)
    b = run_step_c_abi(c, tc=tc)
    tc.close()
    assert a[0] == b[0] and np.array_equal(a[2], b[2]) and all(np.array_equal(a[1][n], b[1][n]) for n in NAMES)


def test_a_refused_step_leaves_the_outputs_untouched():
    """B (L + 1) >= 2^30 is refused by the plan: FARNN_ERANGE, nothing enqueued, nothing written (x / lengths / labels are
    never read, so small buffers stand in for them)"""
    from re2nn_seq_amd import _lib
    dev = torch.device('cuda', 0)
    c = make_case(3, 4, 3, 2, 2, 2, 2, seed=9)
    tc = _lib.Decomp1TrainContext(3, 4, 3, 2, 2, nl='relu')
    w = {n: torch.from_numpy(c['p'][n]).to(dev) for n in NAMES}
    x, lengths, labels = (torch.from_numpy(c[n]).to(dev) for n in ('x', 'lengths', 'labels'))
    outs = {n: torch.full_like(w[n], 7.0) for n in NAMES}
    loss, tags = torch.full((1,), 3.0, device=dev), torch.full((4,), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(_lib.FarnnError) as e:
        tc.step(dict({ABI[n]: t.data_ptr() for n, t in w.items()}, P=None), x.data_ptr(), lengths.data_ptr(), labels.data_ptr(),
                1 << 15, 1 << 15, 5, dict({'d' + ABI[n]: t.data_ptr() for n, t in outs.items()}, loss=loss.data_ptr(),
                                         tags=tags.data_ptr()))
    assert '2^30' in str(e.value)
    torch.cuda.synchronize()
    assert float(loss) == 3.0 and (tags == 77).all() and all(bool((t == 7.0).all()) for t in outs.values())
    got = run_step_c_abi(c, tc=tc)                            # the context still works
    tc.close()
    assert_float_path(got[0], c['_ref'][0][0], c['_ref'][1][0], err_msg='loss after a refused step')


def _adam_batches(V, C, seed, n=3):
    rng = np.random.RandomState(seed)
    return [(rng.randint(0, V, size=(6, 4)).astype(np.int64), rng.randint(1, 5, size=6).astype(np.int64),
             rng.randint(0, C, size=(6, 4)).astype(np.int64)) for _ in range(n)]


@pytest.mark.parametrize('native', [False, True])
def test_three_adam_steps_match_the_restatement(native):
    """strictly positive weights: no relu of a later step sits at its kink after an optimizer step"""
    from re2nn_seq_amd.farnn.model_decompose_independent import FARNN_S_D_W_I
    from test_decomp1_train_cpu import FLAGS
    from util import ns
    V, S, R, RO, C, D = 9, 5, 4, 3, 4, 3
    rng = np.random.RandomState(31)
    pos = lambda *s: rng.choice(np.array([0.125, 0.25, 0.375, 0.5], np.float32), size=s)      # noqa: E731
    Vm, S1, S2, W, Co, S1o, S2o = pos(V, R), pos(S, R), pos(S, R), pos(S, S) / 4, pos(C, RO), pos(S, RO), pos(S, RO)
    E = pos(V, D)
    h0, hT = np.full(S, 0.5, np.float32), np.full(S, 0.5, np.float32)
    a = ns(independent=1, update_nonlinear='relu', **FLAGS)
    m = FARNN_S_D_W_I(V=Vm, S1=S1, S2=S2, C_output=Co, S1_output=S1o, S2_output=S2o, wildcard_mat=W,
                      wildcard_output=np.zeros((S, S), np.float32), final_vector=hT, start_vector=h0, pretrained_word_embed=E,
                      priority_mat=None, args=a, o_idx=0)
    p0 = {n: np.ascontiguousarray(t.numpy(), dtype=np.float32) for n, t in m.state_dict().items() if n in PARAMS}
    wo = m.state_dict()['wildcard_output'].numpy().copy()
    batches = _adam_batches(V, C, 32)
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
    kw = dict(P=None, batches=batches, trainable=set(PARAMS), nl='relu', lr=0.01)
    p32, p64 = dtr.adam_steps(p0, dtype=torch.float32, **kw), dtr.adam_steps(p0, dtype=torch.float64, **kw)
    for k in (0, 1, 2):                                       # the inputs of every step keep the gap rule
        pk = p0 if k == 0 else dtr.adam_steps(p0, dtype=torch.float64, **dict(kw, batches=batches[:k]))
        dtr.check_gap(pk, None, batches[k][0], batches[k][1], nl='relu')
    for n in PARAMS:
        assert_float_path(sd[n].numpy(), p32[n], p64[n], err_msg=n + ' after 3 Adam steps')
        assert np.abs(sd[n].numpy() - p0[n]).max() > 0, n
    assert np.array_equal(sd['wildcard_output'].numpy(), wo)


def test_thirty_steps_lower_the_loss_and_tagging_reads_the_trained_weights():
    _, inp, _ = case(4)
    m = model(4)
    x, lt, lab = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths']), torch.from_numpy(inp['labels'])
    _, before, _ = m.forward_local(x, lab, lt, train=False)
    opt = torch.optim.Adam(list(m.enable_training().parameters()), lr=0.02, weight_decay=0)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss, _, _ = m.forward_local(x, lab, lt, train=True)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0]
    _, after, _ = m.forward_local(x, lab, lt, train=False)
    fresh = model(4)
    fresh.load_state_dict(m.state_dict())
    _, want, _ = fresh.forward_local(x, lab, lt, train=False)
    assert np.array_equal(after.numpy(), want.numpy())
    assert not np.array_equal(after.numpy(), before.numpy()), 'thirty steps left every tag as it was: the test shows nothing'


def _cli_argv(tmp_path):
    from re2nn_seq_amd import synth
    tree = synth.write_dataset_tree(str(tmp_path / 'data'), dataset='ATIS-BIO', seed=4)
    return ['--dataset', 'ATIS-BIO', '--method', 'decompose', '--independent', '1',
            '--automata_path', tree['paths']['IID'], '--rank', '100', '--rank_wildcard', '70', '--seed', '1',
            '--beta', '0.9', '--embed_dim', '16', '--normalize_automata', 'none', '--rand_constant', '0',
            '--update_nonlinear', 'tanh', '--bz', '9', '--seq_max_len', '12', '--epoch', '2', '--lr', '0.01',
            '--train_portion', '1.0', '--data_dir', tree['paths']['data_dir'], '--model_dir', str(tmp_path / 'm')]


def test_decompose_independent1_cli_trains_for_two_epochs(tmp_path):
    """--method decompose --independent 1 --epoch 2 through train_epochs"""
    from re2nn_seq_amd import main as cli
    results, stats, res_path = cli.main(_cli_argv(tmp_path))
    steps = stats['train_step']
    assert len(steps) == 2 and all(s['tokens'] > 0 and s['tokens_per_s'] > 0 for s in steps)
    saved = cli.load_res(res_path)
    losses = [float(line.split('LOSS:')[1]) for line in saved['logger'].record if 'TRAIN' in line and 'LOSS:' in line]
    assert len(losses) == 2 and all(np.isfinite(losses))


def test_the_cli_without_the_opt_in_is_refused_before_any_evaluation(tmp_path, monkeypatch):
    from re2nn_seq_amd import main as cli
    from re2nn_seq_amd import train_onehot
    monkeypatch.delenv('RE2NN_DECOMP_IND1_TRAIN')

    def boom(*a, **k):
        raise AssertionError('an evaluation ran before the refusal')
    monkeypatch.setattr(train_onehot, 'val_onehot', boom)
    with pytest.raises(NotImplementedError) as e:
        cli.main(_cli_argv(tmp_path))
    assert str(e.value) == REFUSAL
