"""The HIP training step of the onehot independent=1 model (FARNN_S_O_I): the model mirror against the
loss / gradients / predictions captured from the reference, the C-ABI against the torch restatement
(tests/ind1_train_ref.py) at the shape edges of its kernels, its refusals, Adam steps on the device, and the command line."""
import os

import numpy as np
import pytest
import torch

import ind1_train_ref as itr
from test_ind1_train_cpu import N_CASES, REFUSAL, case
from util import GOLDEN, assert_float_path, check_grad, ns, present_words

pytestmark = pytest.mark.gpu
GUARD = 64
KEYS = ('T', 'W', 'O', 'h0', 'hT', 'P', 'x', 'lengths', 'labels', 'mask')


def _model(inp, cfg):
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I
    C = inp['O'].shape[0]
    pri = inp['P'][:-1, :-1] if cfg['use_priority'] else np.eye(C - 1)
    a = ns(independent=cfg['independent'], use_priority=cfg['use_priority'], threshold=inp['threshold'])
    return FARNN_S_O_I(inp['T'], inp['O'], inp['W'], None, inp['hT'], inp['h0'], pri, a, o_idx=inp['o_idx'])


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    monkeypatch.setenv('RE2NN_ONEHOT_IND1_TRAIN', '1')


@pytest.mark.parametrize('k', range(N_CASES))
def test_model_mirror_matches_the_reference_capture(k):
    cfg, inp, ref = case(k)
    m = _model(inp, cfg)
    x, lt, lab = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths']), torch.from_numpy(inp['labels'])
    m.train()
    loss, pred, true = m.forward_local(x, lab, lt, train=True)
    loss.backward()
    named = dict(m.named_parameters())
    assert set(named) == {'language_tensor'}
    l64, g64, _ = itr.step(dtype=torch.float64, **inp)
    assert_float_path(float(loss.detach()), ref['loss'], l64, err_msg='loss')
    present = present_words(inp['x'], inp['lengths'], inp['T'].shape[0])
    check_grad('ind1 capture c{}'.format(k), 'dT', named['language_tensor'].grad.cpu().numpy(), ref['dT'], g64, slices=0,
               present=present)
    assert np.array_equal(pred.cpu().numpy(), ref['flat_pred'])
    assert true.shape == pred.shape


def make_case(V, S, C, B, L, seed, lengths=None, priority=False, x=None, mask=False):
    """a signed real-valued case that keeps the gap rule; drawn again (next seed) while the float64 restatement's gradient
    is below 1e-3 -- chains that die at the first relu, a saturated softmax -- so that every case has something to compare.
    Both conditions are read off the restatement alone."""
    for attempt in range(50):
        c = _draw(V, S, C, B, L, seed + 1000 * attempt, lengths, priority, x, mask)
        g = itr.step(dtype=torch.float64, **c)[1]
        if np.abs(g).max() < 1e-3:
            continue
        # and while the float32 restatement leaves a present word's block beyond a tenth of the bar from float64 (cancellation:
        # tests/util.py judges such a block at the tensor's scale and allows 1 % of the words, none of so few)
        g32 = itr.step(dtype=torch.float32, **c)[1]
        sw = np.abs(g).reshape(V, -1).max(1)
        if (np.abs(g32 - g).reshape(V, -1).max(1) <= 1e-5 * sw).all():
            return c
    raise AssertionError('no live case in 50 draws')


def _draw(V, S, C, B, L, seed, lengths, priority, x, mask):
    rng = np.random.RandomState(seed)
    T, W, O, h0, hT = itr.signed_base(V, S, C, rng)
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
    itr.check_gap(T, W, O, h0, hT, x, lengths, mask=mask)
    return dict(T=T, W=W, O=O, h0=h0, hT=hT, P=P, x=x, lengths=lengths, labels=labels, mask=mask)


def run_step_c_abi(c, tc=None, threshold=0.5, o_idx=0):
    """farnn_ind1_train_step on pre-filled outputs with guard elements around dT and tags; returns (loss, dT, tags) and
    asserts that the guards are untouched"""
    from re2nn_seq_amd import _lib
    dev = torch.device('cuda', 0)
    V, S, _ = c['T'].shape
    C = c['O'].shape[0]
    own = tc is None
    if own:
        tc = _lib.Ind1TrainContext(V, S, C, mask_by_output=c['mask'], threshold=threshold, o_idx=o_idx, device=0)
    try:
        w = {n: torch.from_numpy(np.ascontiguousarray(c[n], dtype=np.float32)).to(dev) for n in ('T', 'W', 'O', 'h0', 'hT')}
        P = None if c['P'] is None else torch.from_numpy(np.ascontiguousarray(c['P'], dtype=np.float32)).to(dev)
        x, lengths, labels = (torch.from_numpy(np.ascontiguousarray(c[n])).to(dev) for n in ('x', 'lengths', 'labels'))
        B, L = c['x'].shape
        bufs = {'dT': torch.full((w['T'].numel() + 2 * GUARD,), 7.0, device=dev),
                'tags': torch.full((B * L + 2 * GUARD,), 77, dtype=torch.int32, device=dev)}
        loss = torch.full((1 + 2 * GUARD,), 3.0, device=dev)
        out = {n: t.data_ptr() + GUARD * 4 for n, t in bufs.items()}
        tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None if P is None else P.data_ptr()), x.data_ptr(),
                lengths.data_ptr(), labels.data_ptr(), B, L, int(np.clip(c['lengths'], 0, L).sum()),
                dict(out, loss=loss.data_ptr() + GUARD * 4))
        torch.cuda.synchronize()
        h = {n: t.cpu().numpy() for n, t in bufs.items()}
        hl = loss.cpu().numpy()
        for n, fill in (('dT', 7.0), ('tags', 77)):
            assert (h[n][:GUARD] == fill).all() and (h[n][-GUARD:] == fill).all(), 'guard elements around {} overwritten'.format(n)
        assert (hl[:GUARD] == 3.0).all() and (hl[-GUARD:] == 3.0).all(), 'guard elements around loss overwritten'
        return float(hl[GUARD]), h['dT'][GUARD:-GUARD].reshape(c['T'].shape), h['tags'][GUARD:-GUARD].reshape(B, L)
    finally:
        if own:
            tc.close()


_REF = {}


def reference(name, c):
    """the restatement in float32 and float64, computed once per case"""
    if name not in _REF:
        kw = {k: c[k] for k in KEYS}
        _REF[name] = (itr.step(dtype=torch.float32, **kw), itr.step(dtype=torch.float64, **kw))
    return _REF[name]


def check_case(name, c):
    (l32, g32, p32), (l64, g64, p64) = reference(name, c)
    loss, dT, tags = run_step_c_abi(c)
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


@pytest.mark.parametrize('k,S', list(enumerate([1, 3, 4, 5, 63, 64, 65, 71, 104, 127, 128])))
def test_state_counts_at_the_chunk_and_row_share_edges(k, S):
    """priority and mask alternate, and every combination of the two is met (k % 2, k // 2 % 2)"""
    C, V = (5, 6) if S <= 71 else (2, 5)
    c = make_case(V, S, C, 4, 3, seed=100 + S, lengths=[3, 0, 2, 1], priority=k % 2 == 0, mask=(k // 2) % 2 == 1)
    check_case('ind1 S{}'.format(S), c)


@pytest.mark.parametrize('C', [2, 5, 64, 65])
def test_label_counts(C):
    c = make_case(7, 5, C, 3, 4, seed=200 + C, priority=C == 5, mask=C == 64)
    check_case('ind1 C{}'.format(C), c)


def test_the_largest_label_count_and_the_first_refused_one():
    from re2nn_seq_amd import _lib
    c = make_case(2, 1, 2400, 2, 2, seed=5)
    check_case('ind1 C2400', c)
    with pytest.raises(_lib.FarnnError) as e:
        _lib.Ind1TrainContext(2, 1, 2401)
    assert 'score columns' in str(e.value)


@pytest.mark.parametrize('V,B,L,lengths', [(1, 3, 3, [3, 1, 2]), (9, 2, 2, [2, 1]), (4, 1, 1, [1]), (5, 4, 5, [0, 5, 2, 0])])
def test_vocabulary_and_batch_edges(V, B, L, lengths):
    """one word only; absent words; a single position; zero-length beside full-length sequences"""
    c = make_case(V, 6, 3, B, L, seed=300 + V, lengths=lengths, mask=V == 9)
    _, dT, _ = check_case('ind1 V{} B{} L{}'.format(V, B, L), c)
    present = present_words(c['x'], c['lengths'], V)
    assert not dT[~present].any()
    if V == 9:
        assert (~present).any()


@pytest.mark.parametrize('n,C', [(31, 3), (32, 3), (33, 3), (65, 3), (65, 40)])
def test_a_word_at_the_edges_of_a_run_of_32_positions(n, C):
    """C = 40 with V = 3: three labels per group in the score and adjoint passes, so a word of several rounds also meets the
    second and third label of a group -- the partials of d alpha / d beta added to what the group's first label wrote, the
    stash staged again per label; the dT pass stages it again for each of the 40 labels"""
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
    c = make_case(V, 7, C, B, L, seed=400 + n + C, lengths=lengths, x=x, mask=n == 33)
    check_case('ind1 run{} C{}'.format(n, C), c)


def test_two_steps_are_bit_identical_and_the_mask_changes_the_step():
    from re2nn_seq_amd import _lib
    c = make_case(6, 71, 5, 6, 4, seed=21, priority=True, mask=True)
    tc = _lib.Ind1TrainContext(6, 71, 5, mask_by_output=True)
    a = run_step_c_abi(c, tc=tc)
    b = run_step_c_abi(c, tc=tc)
    tc.close()
    assert a[0] == b[0] and all(np.array_equal(p, q) for p, q in zip(a[1:], b[1:]))
    check_case('ind1 bitwise masked', c)
    off = dict(c, mask=False)
    (_, g_on, _), (_, g_off, _) = reference('ind1 bitwise masked', c)[1], reference('ind1 bitwise unmasked', off)[1]
    assert np.abs(g_on - g_off).max() > 1e-3 * np.abs(g_on).max(), 'badly drawn: the mask changes nothing in the restatement'
    n = check_case('ind1 bitwise unmasked', off)
    assert not np.array_equal(a[1], n[1])


def test_create_refuses_more_than_128_states():
    from re2nn_seq_amd import _lib
    with pytest.raises(_lib.FarnnError) as e:
        _lib.Ind1TrainContext(4, 129, 3)
    assert '128 states' in str(e.value)
    assert _lib.load().farnn_ind1_train_create is not None


def test_a_refused_step_leaves_the_outputs_untouched():
    """B (L + 1) >= 2^30 is refused by the plan: FARNN_ERANGE, nothing enqueued, nothing written (x / lengths / labels are
    never read, so small buffers stand in for them)"""
    from re2nn_seq_amd import _lib
    dev = torch.device('cuda', 0)
    c = make_case(3, 4, 2, 2, 2, seed=9)
    tc = _lib.Ind1TrainContext(3, 4, 2)
    w = {n: torch.from_numpy(c[n]).to(dev) for n in ('T', 'W', 'O', 'h0', 'hT')}
    x, lengths, labels = (torch.from_numpy(c[n]).to(dev) for n in ('x', 'lengths', 'labels'))
    dT = torch.full_like(w['T'], 7.0)
    loss, tags = torch.full((1,), 3.0, device=dev), torch.full((4,), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(_lib.FarnnError) as e:
        tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None), x.data_ptr(), lengths.data_ptr(), labels.data_ptr(),
                1 << 15, 1 << 15, 5, dict(loss=loss.data_ptr(), dT=dT.data_ptr(), tags=tags.data_ptr()))
    assert '2^30' in str(e.value)
    torch.cuda.synchronize()
    assert float(loss) == 3.0 and (dT == 7.0).all() and (tags == 77).all()
    # the context still works
    got = run_step_c_abi(c, tc=tc)
    tc.close()
    l64 = reference('ind1 after a refusal', c)[1][0]
    assert_float_path(got[0], reference('ind1 after a refusal', c)[0][0], l64, err_msg='loss after a refused step')


def _adam_batches(V, C, seed, n=3):
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        lengths = rng.randint(1, 5, size=6).astype(np.int64)
        out.append((rng.randint(0, V, size=(6, 4)).astype(np.int64), lengths, rng.randint(0, C, size=(6, 4)).astype(np.int64)))
    return out


@pytest.mark.parametrize('native', [False, True])
def test_three_adam_steps_match_the_restatement(native, monkeypatch):
    """torch.optim with independent = 1, the library's optimizer with independent = 2 (the masked chains)"""
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I
    # every weight strictly positive: an optimizer step moves every entry of a present word, and no relu of a later step sits
    # near its kink (the signed bases lose the gap rule after one Adam step: entries that were zero become +-lr; the relu masks
    # are the business of the single-step cases above)
    V, S, C = 9, 5, 4
    mask = native
    rng = np.random.RandomState(31)
    T = rng.choice(np.array([0.125, 0.25, 0.375, 0.5], np.float32), size=(V, S, S))
    W = rng.choice(np.array([0.125, 0.25], np.float32), size=(S, S))
    O = rng.choice(np.array([0.25, 0.5, 1.0], np.float32), size=(C, S, S))
    h0, hT = np.full(S, 0.5, np.float32), np.full(S, 0.5, np.float32)
    batches = _adam_batches(V, C, 32)
    itr.check_gap(T, W, O, h0, hT, *batches[0][:2], mask=mask)
    m = FARNN_S_O_I(T, O, W, None, hT, h0, np.eye(C - 1), ns(independent=2 if mask else 1), o_idx=0)
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
    kw = dict(P=None, batches=batches, mask=mask, lr=0.01)
    T32 = itr.adam_steps(T, W, O, h0, hT, dtype=torch.float32, **kw)
    T64 = itr.adam_steps(T, W, O, h0, hT, dtype=torch.float64, **kw)
    # the inputs of the later steps (the float64 restatement's weights after one and two steps) keep the gap rule
    for k in (1, 2):
        Tk = itr.adam_steps(T, W, O, h0, hT, dtype=torch.float64, **dict(kw, batches=batches[:k]))
        itr.check_gap(Tk, W, O, h0, hT, batches[k][0], batches[k][1], mask=mask)
    assert_float_path(sd['language_tensor'], T32, T64, err_msg='language_tensor after 3 Adam steps')
    assert np.abs(sd['language_tensor'] - T).max() > 0
    assert np.array_equal(sd['wildcard_mat'], W) and np.array_equal(sd['output_tensor'], O)


def test_thirty_steps_lower_the_loss_and_tagging_reads_the_trained_weights():
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I
    g = np.load(os.path.join(GOLDEN, 'ind1_small.npz'))
    C = g['Oten'].shape[0]
    a = ns(independent=1)
    m = FARNN_S_O_I(g['T'], g['Oten'], g['W'], None, g['hT'], g['h0'], np.eye(C - 1), a, o_idx=int(g['o_idx']))
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
    fresh = FARNN_S_O_I(sd['language_tensor'], sd['output_tensor'], sd['wildcard_mat'], None, g['hT'], g['h0'], np.eye(C - 1), a,
                        o_idx=int(g['o_idx']))
    _, want, _ = fresh.forward_local(x, lab, lt, train=False)
    assert np.array_equal(after.numpy(), want.numpy())
    assert not np.array_equal(after.numpy(), before.numpy()), 'thirty steps left every tag as it was: the test shows nothing'


def _cli_argv(tmp_path):
    from re2nn_seq_amd import synth
    tree = synth.write_dataset_tree(str(tmp_path / 'data'), dataset='ATIS-BIO', seed=4)
    return ['--dataset', 'ATIS-BIO', '--method', 'onehot', '--independent', '1',
            '--automata_path', tree['paths']['ID1'], '--normalize_automata', 'none', '--rand_constant', '0',
            '--bz', '9', '--seq_max_len', '12', '--epoch', '2', '--lr', '0.01',
            '--train_portion', '1.0', '--data_dir', tree['paths']['data_dir'], '--model_dir', str(tmp_path / 'm')]


def test_ind1_cli_trains_for_two_epochs(tmp_path):
    """--method onehot --independent 1 --epoch 2 through train_epochs"""
    from re2nn_seq_amd import main as cli
    results, stats, res_path = cli.main(_cli_argv(tmp_path))
    steps = stats['train_step']
    assert len(steps) == 2 and all(s['tokens'] > 0 and s['tokens_per_s'] > 0 for s in steps)
    saved = cli.load_res(res_path)
    losses = [float(line.split('LOSS:')[1]) for line in saved['logger'].record if 'TRAIN' in line and 'LOSS:' in line]
    assert len(losses) == 2 and all(np.isfinite(losses))


def test_pin_the_ind1_cli_without_the_opt_in_raises_as_it_did(tmp_path, monkeypatch):
    """a pin of existing behaviour (it passes before this step existed too): no opt-in, the refusal and its message as before"""
    from re2nn_seq_amd import main as cli
    monkeypatch.delenv('RE2NN_ONEHOT_IND1_TRAIN')
    with pytest.raises(NotImplementedError) as e:
        cli.main(_cli_argv(tmp_path))
    assert str(e.value) == REFUSAL


def test_an_edge_built_model_densifies_to_the_tensors_it_tags_with():
    """FARNN_S_O_I.from_automaton: _dense() (what enable_training trains) gives the same tags as the edge-built handle, also
    with a vocabulary that lacks members of the automaton's word classes (the label stays in output_tensor)"""
    from re2nn_seq_amd import synth
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I
    dset, automaton = synth.make_dataset(60, 4, 20, 4)[:2]
    t2i = dict(dset['t2i']); t2i['<pad>'] = len(t2i)
    s2i = dset['s2i']
    a = ns(independent=1)
    me = FARNN_S_O_I.from_automaton(automaton, t2i, s2i, None, a, o_idx=s2i['o'])
    T, W, O = me._dense()
    md = FARNN_S_O_I(T, O, W, None, me.hT, me.h0, None, a, o_idx=s2i['o'])
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
