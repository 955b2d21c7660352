"""The HIP training step of the onehot FST (FARNN_S_O): the model mirror against the loss / gradients /
predictions captured from the reference, the C-ABI against the torch restatement (tests/fst4_train_ref.py) at the shape
edges of its kernels, its refusals, Adam steps on the device, and the command line."""
import os

import numpy as np
import pytest
import torch

import fst4_train_ref as ftr
from test_fst4_train_cpu import N_CASES, case
from util import GOLDEN, assert_float_path, check_grad, ns, present_words

pytestmark = pytest.mark.gpu
GUARD = 64


def _model(inp, cfg):
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O
    C, S, _ = inp['W4'].shape
    pri = inp['P'][:-1, :-1] if cfg['use_priority'] else np.eye(C - 1)
    a = ns(independent=0, use_priority=cfg['use_priority'], train_wildcard=cfg['train_wildcard'], threshold=inp['threshold'])
    return FARNN_S_O(inp['T4'], inp['W4'], np.zeros((S, S)), inp['hT'], inp['h0'], pri, a, o_idx=inp['o_idx'])


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    monkeypatch.setenv('RE2NN_ONEHOT_FST_TRAIN', '1')


@pytest.mark.parametrize('k', range(N_CASES))
def test_model_mirror_matches_the_reference_capture(k):
    cfg, inp, ref = case(k)
    m = _model(inp, cfg)
    x, lt, lab = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths']), torch.from_numpy(inp['labels'])
    m.train()
    loss, pred, true = m.forward_local(x, lab, lt, train=True)
    loss.backward()
    named = dict(m.named_parameters())
    assert set(named) == {'language_tensor'} | ({'wildcard_tensor'} if cfg['train_wildcard'] else set())
    l64, g64, w64, _ = ftr.step(dtype=torch.float64, **inp)
    assert_float_path(float(loss.detach()), ref['loss'], l64, err_msg='loss')
    present = present_words(inp['x'], inp['lengths'], inp['T4'].shape[0])
    check_grad('fst4 capture c{}'.format(k), 'dT4', named['language_tensor'].grad.cpu().numpy(), ref['dT4'], g64, slices=0,
               present=present)
    if cfg['train_wildcard']:
        check_grad('fst4 capture c{}'.format(k), 'dW4', named['wildcard_tensor'].grad.cpu().numpy(), ref['dW4'], w64)
    assert np.array_equal(pred.cpu().numpy(), ref['flat_pred'])
    assert true.shape == pred.shape


def make_case(V, S, C, B, L, seed, lengths=None, priority=False, x=None):
    """a signed real-valued case that keeps the gap rule; drawn again (next seed) while the float64 restatement's gradient
    is below 1e-3 -- chains that die at the first relu, a saturated softmax -- so that every case has something to compare.
    Both conditions are read off the restatement alone."""
    for attempt in range(50):
        c = _draw(V, S, C, B, L, seed + 1000 * attempt, lengths, priority, x)
        g = ftr.step(dtype=torch.float64, **c)[1]
        if np.abs(g).max() < 1e-3:
            continue
        # and while the float32 restatement leaves a present word's block beyond a tenth of the bar from float64 (cancellation:
        # tests/util.py judges such a block at the tensor's scale and allows 1 % of the words, none of so few)
        g32 = ftr.step(dtype=torch.float32, **c)[1]
        sw = np.abs(g).reshape(V, -1).max(1)
        if (np.abs(g32 - g).reshape(V, -1).max(1) <= 1e-5 * sw).all():
            return c
    raise AssertionError('no live case in 50 draws')


def _draw(V, S, C, B, L, seed, lengths, priority, x):
    rng = np.random.RandomState(seed)
    T4, W4, h0, hT = ftr.signed_base(V, S, C, rng)
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
    c = dict(T4=T4, W4=W4, h0=h0, hT=hT, P=P, x=x, lengths=lengths, labels=labels)
    ftr.check_gap(T4, W4, h0, hT, x, lengths)
    return c


def run_step_c_abi(c, wildcard=True, tc=None, threshold=0.5, o_idx=0):
    """farnn_fst4_train_step on pre-filled outputs with guard elements around dT4, dW4 and tags; returns
    (loss, dT4, dW4 or None, tags) and asserts that the guards are untouched"""
    from re2nn_seq_amd import _lib
    dev = torch.device('cuda', 0)
    V, C, S, _ = c['T4'].shape
    own = tc is None
    if own:
        tc = _lib.Fst4TrainContext(V, S, C, threshold=threshold, o_idx=o_idx, device=0)
    try:
        w = {n: torch.from_numpy(np.ascontiguousarray(c[n], dtype=np.float32)).to(dev) for n in ('T4', 'W4', 'h0', 'hT')}
        P = None if c['P'] is None else torch.from_numpy(np.ascontiguousarray(c['P'], dtype=np.float32)).to(dev)
        x, lengths, labels = (torch.from_numpy(np.ascontiguousarray(c[n])).to(dev) for n in ('x', 'lengths', 'labels'))
        B, L = c['x'].shape
        bufs = {'dT4': torch.full((w['T4'].numel() + 2 * GUARD,), 7.0, device=dev),
                'dW4': torch.full((w['W4'].numel() + 2 * GUARD,), 7.0, device=dev),
                'tags': torch.full((B * L + 2 * GUARD,), 77, dtype=torch.int32, device=dev)}
        loss = torch.full((1,), 3.0, device=dev)
        es = {'dT4': 4, 'dW4': 4, 'tags': 4}
        out = {n: t.data_ptr() + GUARD * es[n] for n, t in bufs.items()}
        if not wildcard:
            out['dW4'] = None
        tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None if P is None else P.data_ptr()), x.data_ptr(),
                lengths.data_ptr(), labels.data_ptr(), B, L, int(np.clip(c['lengths'], 0, L).sum()), dict(out, loss=loss.data_ptr()))
        torch.cuda.synchronize()
        h = {n: t.cpu().numpy() for n, t in bufs.items()}
        for n, fill in (('dT4', 7.0), ('dW4', 7.0), ('tags', 77)):
            assert (h[n][:GUARD] == fill).all() and (h[n][-GUARD:] == fill).all(), 'guard elements around {} overwritten'.format(n)
        if not wildcard:
            assert (h['dW4'] == 7.0).all()
        return (float(loss), h['dT4'][GUARD:-GUARD].reshape(c['T4'].shape),
                h['dW4'][GUARD:-GUARD].reshape(c['W4'].shape) if wildcard else None, h['tags'][GUARD:-GUARD].reshape(B, L))
    finally:
        if own:
            tc.close()


_REF = {}


def reference(name, c):
    """the restatement in float32 and float64, computed once per case"""
    if name not in _REF:
        kw = {k: c[k] for k in ('T4', 'W4', 'h0', 'hT', 'P', 'x', 'lengths', 'labels')}
        _REF[name] = (ftr.step(dtype=torch.float32, **kw), ftr.step(dtype=torch.float64, **kw))
    return _REF[name]


def check_case(name, c):
    (l32, g32, w32, p32), (l64, g64, w64, p64) = reference(name, c)
    loss, dT4, dW4, tags = run_step_c_abi(c)
    assert_float_path(loss, l32, l64, err_msg=name + ' loss')
    present = present_words(c['x'], c['lengths'], dT4.shape[0])
    check_grad(name, 'dT4', dT4, g32, g64, slices=0, present=present)
    check_grad(name, 'dW4', dW4, w32, w64)
    B, L = c['x'].shape
    valid = np.arange(L)[None, :] < np.clip(c['lengths'], 0, L)[:, None]
    assert (tags[~valid] == -1).all()
    assert np.array_equal(p32, p64), 'badly drawn: the restatement decodes differently in float32 and float64'
    assert np.array_equal(tags[valid], p64)
    return loss, dT4, dW4, tags


@pytest.mark.parametrize('S', [1, 3, 4, 5, 63, 64, 65, 71, 104, 127, 128])
def test_state_counts_at_the_chunk_and_row_share_edges(S):
    C, V = (5, 6) if S <= 71 else (2, 5)
    c = make_case(V, S, C, 4, 3, seed=100 + S, lengths=[3, 0, 2, 1], priority=S % 2 == 0)
    check_case('fst4 S{}'.format(S), c)


@pytest.mark.parametrize('C', [2, 5, 64, 65])
def test_label_counts(C):
    c = make_case(7, 5, C, 3, 4, seed=200 + C, priority=C == 5)
    check_case('fst4 C{}'.format(C), c)


def test_the_largest_label_count_and_the_first_refused_one():
    from re2nn_seq_amd import _lib
    c = make_case(2, 1, 2400, 2, 2, seed=5)
    check_case('fst4 C2400', c)
    with pytest.raises(_lib.FarnnError) as e:
        _lib.Fst4TrainContext(2, 1, 2401)
    assert 'score columns' in str(e.value)


@pytest.mark.parametrize('V,B,L,lengths', [(1, 3, 3, [3, 1, 2]), (9, 2, 2, [2, 1]), (4, 1, 1, [1]), (5, 4, 5, [0, 5, 2, 0])])
def test_vocabulary_and_batch_edges(V, B, L, lengths):
    """one word only; absent words; a single position; zero-length beside full-length sequences"""
    c = make_case(V, 6, 3, B, L, seed=300 + V, lengths=lengths)
    _, dT4, _, _ = check_case('fst4 V{} B{} L{}'.format(V, B, L), c)
    present = present_words(c['x'], c['lengths'], V)
    assert not dT4[~present].any()
    if V == 9:
        assert (~present).any()


@pytest.mark.parametrize('n,C', [(31, 3), (32, 3), (33, 3), (65, 3), (65, 40)])
def test_a_word_at_the_edges_of_a_run_of_32_positions(n, C):
    """C = 40 with V = 3: three labels per group, so a word of several rounds also meets the second and third label of a
    group -- the partials of d alpha / d beta added to what the group's first label wrote, the stash staged again per label"""
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
    c = make_case(V, 7, C, B, L, seed=400 + n + C, lengths=lengths, x=x)
    check_case('fst4 run{} C{}'.format(n, C), c)


def test_two_steps_are_bit_identical_and_the_wildcard_gradient_is_optional():
    from re2nn_seq_amd import _lib
    c = make_case(6, 71, 5, 6, 4, seed=21, priority=True)
    tc = _lib.Fst4TrainContext(6, 71, 5)
    a = run_step_c_abi(c, tc=tc)
    b = run_step_c_abi(c, tc=tc)
    n = run_step_c_abi(c, tc=tc, wildcard=False)
    tc.close()
    assert a[0] == b[0] and all(np.array_equal(p, q) for p, q in zip(a[1:], b[1:]))
    assert a[0] == n[0] and np.array_equal(a[1], n[1]) and np.array_equal(a[3], n[3]) and n[2] is None


def test_create_refuses_more_than_128_states():
    from re2nn_seq_amd import _lib
    with pytest.raises(_lib.FarnnError) as e:
        _lib.Fst4TrainContext(4, 129, 3)
    assert '128 states' in str(e.value)
    assert _lib.load().farnn_fst4_train_create is not None


def test_a_refused_step_leaves_the_outputs_untouched():
    """B (L + 1) >= 2^30 is refused by the plan: FARNN_ERANGE, nothing enqueued, nothing written (x / lengths / labels are
    never read, so small buffers stand in for them)"""
    from re2nn_seq_amd import _lib
    dev = torch.device('cuda', 0)
    c = make_case(3, 4, 2, 2, 2, seed=9)
    tc = _lib.Fst4TrainContext(3, 4, 2)
    w = {n: torch.from_numpy(c[n]).to(dev) for n in ('T4', 'W4', 'h0', 'hT')}
    x, lengths, labels = (torch.from_numpy(c[n]).to(dev) for n in ('x', 'lengths', 'labels'))
    dT4, dW4 = torch.full_like(w['T4'], 7.0), torch.full_like(w['W4'], 7.0)
    loss, tags = torch.full((1,), 3.0, device=dev), torch.full((4,), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(_lib.FarnnError) as e:
        tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None), x.data_ptr(), lengths.data_ptr(), labels.data_ptr(),
                1 << 15, 1 << 15, 5, dict(loss=loss.data_ptr(), dT4=dT4.data_ptr(), dW4=dW4.data_ptr(), tags=tags.data_ptr()))
    assert '2^30' in str(e.value)
    torch.cuda.synchronize()
    assert float(loss) == 3.0 and (dT4 == 7.0).all() and (dW4 == 7.0).all() and (tags == 77).all()
    # the context still works
    got = run_step_c_abi(c, tc=tc)
    tc.close()
    assert np.isfinite(got[0])


def _adam_batches(V, C, seed, n=3):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        lengths = rng.randint(1, 5, size=6).astype(np.int64)
        out.append((rng.randint(0, V, size=(6, 4)).astype(np.int64), lengths, rng.randint(0, C, size=(6, 4)).astype(np.int64)))
    return out


@pytest.mark.parametrize('native', [False, True])
def test_three_adam_steps_match_the_restatement(native, monkeypatch):
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O
    # every weight strictly positive: an optimizer step moves them all, and no relu of a later step sits near its kink (the
    # signed bases lose the gap rule after one Adam step: entries that were zero become +-lr; the relu masks are the
    # business of the single-step cases above)
    V, S, C = 9, 5, 4
    rng = np.random.RandomState(31)
    T4 = rng.choice(np.array([0.125, 0.25, 0.375, 0.5], np.float32), size=(V, C, S, S))
    W4 = rng.choice(np.array([0.125, 0.25], np.float32), size=(C, S, S))
    h0, hT = np.full(S, 0.5, np.float32), np.full(S, 0.5, np.float32)
    ftr.check_gap(T4, W4, h0, hT, *_adam_batches(V, C, 32)[0][:2])
    batches = _adam_batches(V, C, 32)
    m = FARNN_S_O(T4, W4, np.zeros((S, S)), hT, h0, np.eye(C - 1), ns(independent=0, train_wildcard=1), o_idx=0)
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
    kw = dict(P=None, batches=batches, train_wildcard=True, lr=0.01)
    T32, W32 = ftr.adam_steps(T4, W4, h0, hT, dtype=torch.float32, **kw)
    T64, W64 = ftr.adam_steps(T4, W4, h0, hT, dtype=torch.float64, **kw)
    # the inputs of the later steps (the float64 restatement's weights after one and two steps) keep the gap rule
    for k in (1, 2):
        Tk, Wk = ftr.adam_steps(T4, W4, h0, hT, dtype=torch.float64, **dict(kw, batches=batches[:k]))
        ftr.check_gap(Tk, Wk, h0, hT, batches[k][0], batches[k][1])
    assert_float_path(sd['language_tensor'], T32, T64, err_msg='language_tensor after 3 Adam steps')
    assert_float_path(sd['wildcard_tensor'], W32, W64, err_msg='wildcard_tensor after 3 Adam steps')
    assert np.abs(sd['language_tensor'] - T4).max() > 0 and np.abs(sd['wildcard_tensor'] - W4).max() > 0


def test_thirty_steps_lower_the_loss_and_tagging_reads_the_trained_weights():
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O
    g = np.load(os.path.join(GOLDEN, 'fst4_small.npz'))
    V, C, S, _ = g['T4'].shape
    a = ns(independent=0)
    m = FARNN_S_O(g['T4'], g['W4'], np.zeros((S, S)), g['hT'], g['h0'], np.eye(C - 1), a, o_idx=int(g['o_idx']))
    x, lt = torch.from_numpy(g['x']), torch.from_numpy(g['lengths'])
    lab = torch.from_numpy(np.random.RandomState(3).randint(0, C, size=g['x'].shape).astype(np.int64))
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
    sd = m.state_dict()
    fresh = FARNN_S_O(sd['language_tensor'], sd['wildcard_tensor'], np.zeros((S, S)), g['hT'], g['h0'], np.eye(C - 1), a,
                      o_idx=int(g['o_idx']))
    _, want, _ = fresh.forward_local(x, lab, lt, train=False)
    assert np.array_equal(after.numpy(), want.numpy())
    assert not np.array_equal(after.numpy(), before.numpy()), 'thirty steps left every tag as it was: the test shows nothing'


def _cli_argv(tmp_path):
    from re2nn_seq_amd import synth
    tree = synth.write_dataset_tree(str(tmp_path / 'data'), dataset='ATIS-BIO', seed=4)
    return ['--dataset', 'ATIS-BIO', '--method', 'onehot', '--independent', '0',
            '--automata_path', tree['paths']['ID0'], '--normalize_automata', 'none', '--rand_constant', '0',
            '--bz', '9', '--seq_max_len', '12', '--epoch', '2', '--lr', '0.01',
            '--train_portion', '1.0', '--data_dir', tree['paths']['data_dir'], '--model_dir', str(tmp_path / 'm')]


@pytest.mark.parametrize('native', [False, True])
def test_fst_cli_trains_for_two_epochs(tmp_path, monkeypatch, native):
    """--method onehot --independent 0 --epoch 2 through train_epochs, with torch.optim and with RE2NN_NATIVE_OPTIM=1 (the
    library's one-launch Adam on the 4-D tensor's many chunks); an edge-built model, densified by enable_training"""
    from re2nn_seq_amd import main as cli
    if native:
        monkeypatch.setenv('RE2NN_NATIVE_OPTIM', '1')
    results, stats, res_path = cli.main(_cli_argv(tmp_path))
    steps = stats['train_step']
    assert len(steps) == 2 and all(s['tokens'] > 0 and s['tokens_per_s'] > 0 for s in steps)
    saved = cli.load_res(res_path)
    losses = [float(line.split('LOSS:')[1]) for line in saved['logger'].record if 'TRAIN' in line and 'LOSS:' in line]
    assert len(losses) == 2 and all(np.isfinite(losses))


def test_an_edge_built_model_densifies_to_the_tensors_it_tags_with():
    """FARNN_S_O.from_automaton: _dense() (what enable_training trains) gives the same tags as the edge-built handle"""
    from re2nn_seq_amd import synth
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O
    dset, automaton = synth.make_dataset(60, 4, 20, 4)[:2]
    t2i = dict(dset['t2i']); t2i['<pad>'] = len(t2i)
    s2i = dset['s2i']
    a = ns(independent=0)
    me = FARNN_S_O.from_automaton(automaton, t2i, s2i, None, a, o_idx=s2i['o'])
    T4, W4 = me._dense()
    md = FARNN_S_O(T4, W4, np.zeros((me.S, me.S)), me.hT, me.h0, None, a, o_idx=s2i['o'])
    x, lengths = synth.random_batch(len(t2i), 8, 10, np.random.RandomState(3), min_len=2)
    x, lengths = torch.from_numpy(x), torch.from_numpy(lengths)
    _, pe, _ = me.forward_local(x, x, lengths, train=False)
    _, pd, _ = md.forward_local(x, x, lengths, train=False)
    assert np.array_equal(pe.numpy(), pd.numpy())
    # and training starts from them: one step on either model gives bit-identical gradients
    lab = torch.from_numpy(np.random.RandomState(4).randint(0, me.C, size=tuple(x.shape)).astype(np.int64))
    grads = []
    for m in (me, md):
        loss, _, _ = m.forward_local(x, lab, lengths, train=True)
        loss.backward()
        grads.append(dict(m.named_parameters())['language_tensor'].grad.cpu().numpy())
    assert np.array_equal(grads[0], grads[1]) and np.abs(grads[0]).max() > 0


def test_pin_the_fst_cli_without_the_opt_in_raises_as_it_did(tmp_path, monkeypatch):
    """a pin of existing behaviour (it passes before this step existed too): no opt-in, the refusal and its message as before"""
    from re2nn_seq_amd import main as cli
    monkeypatch.delenv('RE2NN_ONEHOT_FST_TRAIN')
    with pytest.raises(NotImplementedError) as e:
        cli.main(_cli_argv(tmp_path))
    assert 'decomposed only' not in str(e.value) and '--epoch 0' in str(e.value)
