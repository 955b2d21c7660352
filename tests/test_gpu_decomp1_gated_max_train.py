"""The HIP training step of the gated decomposed independent=1 model in the max semiring (FARNN_S_D_W_I, --farnn 1 | 2
--train_mode max): the model mirror against the loss / gradients / predictions captured from the reference,
the C-ABI (farnn_decomp_ind1_gated_max_train_step) against the torch restatement (tests/decomp1_gated_max_train_ref.py) under
the arg-max gap rule at the shape edges of its kernels, an exact tie, its refusals, the plain max step and the gated sum step
beside it on one context, Adam steps on the device, and the command line."""
import numpy as np
import pytest
import torch

import decomp1_gated_max_train_ref as dgm
import decomp1_train_ref as dtr
from test_decomp1_gated_max_train_cpu import MAX_REFUSAL, N_CASES, build, case, params_of, present_of
from test_decomp1_train_cpu import FLAGS, check_all_grads
from test_gpu_decomp1_gated_train import make_case as make_gated_sum_case
from test_gpu_decomp1_gated_train import run_step_c_abi as run_gated_sum_step
from test_gpu_decomp1_train import ABI, GUARD, NAMES, _cli_argv
from test_gpu_decomp1_train import run_step_c_abi as run_plain_step
from test_gpu_decomp1_train_max import make_case as make_plain_max_case
from util import assert_float_path, ns, present_words

pytestmark = pytest.mark.gpu

SWITCHES = ('DECOMP_IND1_TRAIN', 'DECOMP_IND1_GATED_TRAIN', 'DECOMP_IND1_CRF_TRAIN', 'BUCKETED_MAX_TRAIN', 'DECOMP_IND1_GATED_MAX_TRAIN')


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    for name in SWITCHES:
        monkeypatch.setenv('RE2NN_' + name, '1')


@pytest.mark.parametrize('k', range(N_CASES))
def test_model_mirror_matches_the_reference_capture(k):
    cfg, inp, ref = case(k)
    m = build(k)
    x, lt, lab = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths']), torch.from_numpy(inp['labels'])
    m.train()
    loss, pred, true = m.forward_local(x, lab, lt, train=True)
    loss.backward()
    named = dict(m.named_parameters())
    assert set(named) == set(params_of(cfg))
    l64, g64, _ = dgm.step(dtype=torch.float64, **inp)
    assert_float_path(float(loss.detach()), ref['loss'], l64, err_msg='loss')
    got = {n: t.grad.cpu().numpy() for n, t in named.items()}
    check_all_grads('decomp1 gated max capture c{}'.format(k), got, ref['grads'], g64, present_of(inp, ref))
    assert np.array_equal(pred.cpu().numpy(), ref['flat_pred'])
    assert true.shape == pred.shape


def plant_twin(p, farnn, i=0, j=1):
    """state j becomes an exact copy of state i in every tensor, the gates' columns included (the fixtures' twin)"""
    for n in ('S1', 'S2', 'S1_output', 'S2_output', 'h0', 'hT'):
        p[n][j] = p[n][i]
    p['wildcard_mat'][j, :] = p['wildcard_mat'][i, :]
    p['wildcard_mat'][:, j] = p['wildcard_mat'][:, i]
    for n in dgm.gate_keys(farnn):
        p[n][..., j] = p[n][..., i]


def make_case(V, S, R, RO, C, B, L, seed, farnn, lengths=None, priority=False, x=None, nl='tanh', crf=False, twin=False):
    """a signed real-valued case (decomp1_train_ref.signed_base) with seeded gates that keeps the arg-max gap rule and the decode
    rule (decomp1_gated_max_train_ref.check_gap), drawn again (next seed) until the float64 restatement's gradients are live and
    the float32 restatement sits within a tenth of the bar (decomp1_train_ref.badly_drawn) -- conditions read off the
    restatement alone"""
    why = None
    for attempt in range(60):
        rng = np.random.RandomState(seed + 1000 * attempt)
        p = dtr.signed_base(V, S, R, RO, C, rng)
        p.update(dgm.gates_for(S, R, farnn, rng))
        if twin:
            plant_twin(p, farnn)
        ln = rng.randint(1, L + 1, size=B) if lengths is None else lengths
        if lengths is None:
            ln[0] = L
        ln = np.asarray(ln, np.int64)
        xx = rng.randint(0, V, size=(B, L)).astype(np.int64) if x is None else x
        labels = rng.randint(0, C - 2 if crf else C, size=(B, L)).astype(np.int64)
        P = None
        if priority:
            P = np.eye(C, dtype=np.float32)
            P[rng.randint(0, C, 4), rng.randint(0, C, 4)] = -1.0
        trans = None
        if crf:
            trans = dgm.dcr.default_transitions(C)
            trans += np.where(trans > -5000.0, rng.uniform(-0.5, 0.5, size=trans.shape), 0.0).astype(np.float32)
        c = dict(p=p, P=P, x=xx, lengths=ln, labels=labels, nl=nl, farnn=farnn, k=5.0, trans=trans)
        try:
            dgm.check_gap(**{q: v for q, v in c.items() if q != 'labels'})
        except dgm.GapError as e:
            why = str(e)
            continue
        r32, r64 = dgm.step(dtype=torch.float32, **c), dgm.step(dtype=torch.float64, **c)
        # (no sequence of two tokens: no chain step reaches a score, and the gates' gradients are exactly zero in both)
        live = [n for n in r64[1] if ln.max() > 1 or n not in dgm.GATE_KEYS]
        why = dtr.badly_drawn({n: r32[1][n] for n in live}, {n: r64[1][n] for n in live}, present_words(xx, ln, V))
        if why is None and not np.array_equal(r32[2], r64[2]):
            why = 'float32 and float64 decode differently'
        if why is None:
            c['_ref'] = (r32, r64)
            return c
    raise AssertionError('no live case in 60 draws: ' + str(why))


def _ctx(c, semiring='max'):
    from re2nn_seq_amd import _lib
    p = c['p']
    V, R = p['Vgen'].shape
    C, RO = p['C_output'].shape
    return _lib.Decomp1TrainContext(V, p['S1'].shape[0], R, RO, C, nl=c['nl'], semiring=semiring)


def run_step_c_abi(c, tc=None, skip=(), method='gated_max_step'):
    """farnn_decomp_ind1_gated_max_train_step on pre-filled outputs with guard elements around every output; returns (loss,
    grads, tags) and asserts that the guards are untouched.  skip: outputs handed over as NULL."""
    dev = torch.device('cuda', 0)
    p, farnn = c['p'], c['farnn']
    names = NAMES + dgm.gate_keys(farnn) + ((dgm.TRANS,) if c['trans'] is not None else ())
    abi = dict(ABI, **{n: n for n in dgm.GATE_KEYS})
    own = tc is None
    if own:
        tc = _ctx(c)
    try:
        src = dict(p, **{dgm.TRANS: c['trans']})
        w = {n: torch.from_numpy(np.ascontiguousarray(src[n], dtype=np.float32)).to(dev) for n in names}
        P = None if c['P'] is None else torch.from_numpy(np.ascontiguousarray(c['P'], dtype=np.float32)).to(dev)
        x, lengths, labels = (torch.from_numpy(np.ascontiguousarray(c[n])).to(dev) for n in ('x', 'lengths', 'labels'))
        B, L = c['x'].shape
        bufs = {n: torch.full((w[n].numel() + 2 * GUARD,), 7.0, device=dev) for n in names}
        tags = torch.full((B * L + 2 * GUARD,), 77, dtype=torch.int32, device=dev)
        loss = torch.full((1 + 2 * GUARD,), 3.0, device=dev)
        out = {'d' + abi[n]: t.data_ptr() + GUARD * 4 for n, t in bufs.items() if n != dgm.TRANS and n not in skip}
        out.update(loss=loss.data_ptr() + GUARD * 4, tags=tags.data_ptr() + GUARD * 4)
        wp = dict({abi[n]: t.data_ptr() for n, t in w.items() if n != dgm.TRANS}, P=None if P is None else P.data_ptr())
        crf = c['trans'] is not None
        getattr(tc, method)(wp, farnn, c['k'], x.data_ptr(), lengths.data_ptr(), labels.data_ptr(), B, L,
                            int(np.clip(c['lengths'], 0, L).sum()), out, None,
                            trans_ptr=w[dgm.TRANS].data_ptr() if crf else None,
                            dtrans_ptr=bufs[dgm.TRANS].data_ptr() + GUARD * 4 if crf else None)
        torch.cuda.synchronize()
        h = {n: t.cpu().numpy() for n, t in bufs.items()}
        ht, hl = tags.cpu().numpy(), loss.cpu().numpy()
        for n in names:
            assert (h[n][:GUARD] == 7.0).all() and (h[n][-GUARD:] == 7.0).all(), 'guard elements around d{} overwritten'.format(n)
            if n in skip:
                assert (h[n] == 7.0).all(), n
        assert (ht[:GUARD] == 77).all() and (ht[-GUARD:] == 77).all(), 'guard elements around tags overwritten'
        assert (hl[:GUARD] == 3.0).all() and (hl[-GUARD:] == 3.0).all(), 'guard elements around loss overwritten'
        return (float(hl[GUARD]), {n: h[n][GUARD:-GUARD].reshape(np.shape(src[n])) for n in names if n not in skip},
                ht[GUARD:-GUARD].reshape(B, L))
    finally:
        if own:
            tc.close()


def check_case(name, c, **kw):
    (l32, g32, p32), (l64, g64, p64) = c['_ref']
    loss, grads, tags = run_step_c_abi(c, **kw)
    assert_float_path(loss, l32, l64, err_msg=name + ' loss')
    present = present_words(c['x'], c['lengths'], c['p']['Vgen'].shape[0])
    check_all_grads(name, grads, {n: g32[n] for n in grads}, {n: g64[n] for n in grads}, present)
    assert not grads['Vgen'][~present].any(), 'the row of an absent word is not zero'
    B, L = c['x'].shape
    valid = np.arange(L)[None, :] < np.clip(c['lengths'], 0, L)[:, None]
    assert (tags[~valid] == -1).all()
    assert np.array_equal(tags[valid], p64)
    return loss, grads, tags


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[2], b[2]) and all(np.array_equal(a[1][n], b[1][n]) for n in a[1])


@pytest.mark.parametrize('farnn', [1, 2])
@pytest.mark.parametrize('k,S', list(enumerate([1, 3, 4, 5, 63, 64, 65, 96, 97, 127, 128])))
def test_state_counts_at_the_chunk_row_share_and_register_slot_edges(k, S, farnn):
    c = make_case(5, S, 5, 4, 5, 3, 4, seed=100 + S + 7 * farnn, farnn=farnn, lengths=[4, 0, 2] if k % 2 else [3, 4, 1],
                  priority=k % 2 == 0, nl=('relu', 'none', 'tanh', 'relutanh')[k % 4])
    check_case('decomp1 gated{} max S{}'.format(farnn, S), c)


@pytest.mark.parametrize('farnn', [1, 2])
@pytest.mark.parametrize('R', [1, 4, 5, 64, 65, 250])
def test_ranks_at_the_tile_edges(R, farnn):
    c = make_case(7, 5, R, 4, 4, 3, 4, seed=200 + R + 7 * farnn, farnn=farnn, priority=R % 2 == 0, nl='relu' if R % 3 else 'tanh')
    check_case('decomp1 gated{} max R{}'.format(farnn, R), c)


@pytest.mark.parametrize('farnn', [1, 2])
@pytest.mark.parametrize('V,B,L,lengths', [(1, 3, 3, [3, 1, 2]), (4, 1, 1, [1]), (5, 4, 5, [0, 5, 2, 0])])
def test_vocabulary_and_batch_edges(V, B, L, lengths, farnn):
    """one word only; a single position; zero-length beside full-length sequences"""
    c = make_case(V, 6, 5, 4, 3, B, L, seed=600 + V + 7 * farnn, farnn=farnn, lengths=lengths)
    check_case('decomp1 gated{} max V{} B{} L{}'.format(farnn, V, B, L), c)


@pytest.mark.parametrize('farnn', [1, 2])
@pytest.mark.parametrize('n', [31, 32, 33, 65])
def test_a_word_at_the_edges_of_a_run_of_32_positions(n, farnn):
    """the OT_G run edges of onehot_max_dT_kernel behind the gated back-propagation: one run, a full run, two runs, three"""
    B, L, V = 35, 3, 3
    rng = np.random.RandomState(n)
    lengths = np.full(B, 3, np.int64)
    lengths[:4] = [1, 2, 1, 3]
    x = rng.randint(1, V, size=(B, L)).astype(np.int64)
    valid = np.arange(L)[None, :] < lengths[:, None]
    flat = np.flatnonzero(valid.reshape(-1))
    x.reshape(-1)[flat[::len(flat) // n][:n] if len(flat) // n > 1 else flat[:n]] = 0
    assert int((x[valid] == 0).sum()) == n
    c = make_case(V, 7, 5, 6, 3, B, L, seed=700 + n + 7 * farnn, farnn=farnn, lengths=lengths, x=x)
    check_case('decomp1 gated{} max run{}'.format(farnn, n), c)


def test_the_crf_on_the_gated_max_chains():
    c = make_case(5, 65, 5, 4, 6, 3, 5, seed=801, farnn=2, lengths=[5, 1, 3], priority=True, crf=True)
    check_case('decomp1 gated2 max crf S65', c)


@pytest.mark.parametrize('farnn', [1, 2])
@pytest.mark.parametrize('S', [6, 70])
def test_on_an_exact_tie_the_first_index_wins(S, farnn):
    """state 1 is an exact copy of state 0 (the gates' columns included) and the chains run relu: wherever state 0 wins it ties
    state 1 at a non-zero value, and the last maximal index would give other gradients (S 70: the twin lies inside one share of
    18 rows; S 6: one row per share, the twin spans two shares)"""
    c = make_case(5, S, 5, 4, 5, 4, 4, seed=903 if S == 6 else 970 + 7 * farnn, farnn=farnn, lengths=[4, 3, 2, 4], nl='relu', twin=True)
    kw = {q: v for q, v in c.items() if q != '_ref'}
    first, last = c['_ref'][1][1], dgm.step(dtype=torch.float64, fault='last', **kw)[1]
    assert any(np.abs(first[n] - last[n]).max() > 1e-2 * np.abs(first[n]).max() for n in first), 'badly drawn: no tie decides anything'
    check_case('decomp1 gated{} max tie S{}'.format(farnn, S), c)


@pytest.mark.parametrize('farnn', [1, 2])
def test_two_steps_on_one_context_are_bit_identical(farnn):
    c = make_case(6, 71, 9, 5, 5, 6, 4, seed=21 + farnn, farnn=farnn, priority=True)
    tc = _ctx(c)
    a = run_step_c_abi(c, tc=tc)
    b = run_step_c_abi(c, tc=tc)
    tc.close()
    assert _same(a, b)


@pytest.mark.parametrize('farnn', [1, 2])
def test_optional_outputs_may_be_null(farnn):
    c = make_case(6, 7, 5, 4, 4, 4, 3, seed=40 + farnn, farnn=farnn)
    full = check_case('decomp1 gated{} max all outputs'.format(farnn), c)
    part = run_step_c_abi(c, skip=('wildcard_mat', 'C_output', 'h0'))
    assert part[0] == full[0] and np.array_equal(part[2], full[2])
    assert all(np.array_equal(part[1][n], full[1][n]) for n in part[1]) and 'h0' not in part[1]


@pytest.mark.parametrize('what', ['sum context on the new entry', 'max context on the old entry', 'farnn 3', 'null Wss2',
                                  'sigmoid_exponent 0', 'dtrans without crf_trans'])
def test_a_refused_step_leaves_the_outputs_untouched(what):
    """refused by the plan with FARNN_EINVAL: nothing enqueued, nothing written, and the context still works"""
    from re2nn_seq_amd import _lib
    c = make_case(5, 6, 4, 3, 3, 2, 3, seed=9, farnn=2, lengths=[3, 3])
    tc = _ctx(c, semiring='sum' if what.startswith('sum') else 'max')
    method = 'gated_step' if what.startswith('max') else 'gated_max_step'
    bad = dict(c)
    if what == 'farnn 3':
        bad['farnn'] = 3
    elif what == 'null Wss2':
        bad['p'] = dict(c['p'], Wss2=None)
    elif what == 'sigmoid_exponent 0':
        bad['k'] = 0.0
    dev = torch.device('cuda', 0)
    names = NAMES + dgm.GATE_KEYS
    w = {n: None if bad['p'][n] is None else torch.from_numpy(bad['p'][n]).to(dev) for n in names}
    x, lengths, labels = (torch.from_numpy(c[n]).to(dev) for n in ('x', 'lengths', 'labels'))
    outs = {n: torch.full(c['p'][n].shape, 7.0, device=dev) for n in names}
    loss, tags = torch.full((1,), 3.0, device=dev), torch.full((6,), 77, dtype=torch.int32, device=dev)
    dtrans = torch.full((9,), 5.0, device=dev)
    abi = dict(ABI, **{n: n for n in dgm.GATE_KEYS})
    torch.cuda.synchronize()
    with pytest.raises(_lib.FarnnError) as e:
        getattr(tc, method)(dict({abi[n]: None if t is None else t.data_ptr() for n, t in w.items()}, P=None), bad['farnn'], bad['k'],
                            x.data_ptr(), lengths.data_ptr(), labels.data_ptr(), 2, 3, 6,
                            dict({'d' + abi[n]: t.data_ptr() for n, t in outs.items()}, loss=loss.data_ptr(), tags=tags.data_ptr()),
                            None, dtrans_ptr=dtrans.data_ptr() if what.startswith('dtrans') else None)
    msg = str(e.value)
    assert {'sum context on the new entry': 'sum semiring', 'max context on the old entry': 'max semiring', 'farnn 3': 'farnn must be 1 or 2',
            'null Wss2': 'null', 'sigmoid_exponent 0': 'sigmoid_exponent', 'dtrans without crf_trans': 'go together'}[what] in msg
    assert ('decomp_ind1_gated_train_step' if what.startswith('max') else 'decomp_ind1_gated_max_train_step') in msg
    if what.startswith('max'):       # word for word what the entry answered before the max entry existed
        assert msg.endswith('decomp_ind1_gated_train_step: the context is in the max semiring; the gated chains are built for the '
                            'sum semiring only')
    torch.cuda.synchronize()
    assert float(loss) == 3.0 and (tags == 77).all() and all(bool((t == 7.0).all()) for t in outs.values())
    assert bool((dtrans == 5.0).all())
    tc.set_semiring('max')
    got = run_step_c_abi(c, tc=tc)
    tc.close()
    assert_float_path(got[0], c['_ref'][0][0], c['_ref'][1][0], err_msg='loss after a refused step')


def test_the_other_steps_on_the_same_context_return_the_same_bits_before_and_after_a_gated_max_step():
    """the plain max step (max context) and the gated sum step (sum context): the gated max step's arrays lie behind theirs"""
    dims = (6, 71, 9, 5, 5, 6, 4)
    plain = make_plain_max_case(*dims, seed=21, priority=True, nl='relu')
    gated = make_gated_sum_case(*dims, seed=23, farnn=2, nl='relu')
    c = make_case(*dims, seed=25, farnn=2, nl='relu')
    tc = _ctx(c)
    a = run_plain_step(plain, tc=tc)
    tc.set_semiring('sum')
    g = run_gated_sum_step(gated, tc=tc)
    tc.set_semiring('max')
    check_case('decomp1 gated2 max between other steps', c, tc=tc)
    b = run_plain_step(plain, tc=tc)
    tc.set_semiring('sum')
    h = run_gated_sum_step(gated, tc=tc)
    tc.close()
    assert a[0] == b[0] and np.array_equal(a[2], b[2]) and all(np.array_equal(a[1][n], b[1][n]) for n in NAMES)
    assert _same(g, h)


def test_three_adam_steps_match_the_restatement():
    """strictly positive, generic weights and tanh chains: no kink, and the arg-max rule is asserted on the float64
    restatement's weights before every step"""
    from re2nn_seq_amd.farnn.model_decompose_independent import FARNN_S_D_W_I
    V, S, R, RO, C, D = 9, 5, 4, 3, 4, 3
    rng = np.random.RandomState(41)
    pos = lambda *s: (0.2 + 0.8 * rng.rand(*s)).astype(np.float32)      # noqa: E731
    Vm, S1, S2, W, Co, S1o, S2o = pos(V, R), pos(S, R), pos(S, R), pos(S, S) / 4, pos(C, RO), pos(S, RO), pos(S, RO)
    torch.manual_seed(5)
    a = ns(independent=1, update_nonlinear='tanh', farnn=2, xavier=1, bias_init=0.1, sigmoid_exponent=2, train_mode='max', **FLAGS)
    m = FARNN_S_D_W_I(V=Vm, S1=S1, S2=S2, C_output=Co, S1_output=S1o, S2_output=S2o, wildcard_mat=W,
                      wildcard_output=np.zeros((S, S), np.float32), final_vector=pos(S), start_vector=pos(S),
                      pretrained_word_embed=pos(V, D), priority_mat=None, args=a, o_idx=0)
    names = dtr.FLOAT_KEYS + dtr.VGEN_KEYS + dgm.GATE_KEYS
    p0 = {n: np.ascontiguousarray(t.numpy(), dtype=np.float32) for n, t in m.state_dict().items() if n in names}
    batches = [(rng.randint(0, V, size=(6, 4)).astype(np.int64), rng.randint(1, 5, size=6).astype(np.int64),
                rng.randint(0, C, size=(6, 4)).astype(np.int64)) for _ in range(3)]
    kw = dict(P=None, batches=batches, trainable=set(names), nl='tanh', farnn=2, k=2.0, lr=0.01)
    p64 = dgm.adam_steps(p0, dtype=torch.float64, min_gap=2e-5, **kw)
    p32 = dgm.adam_steps(p0, dtype=torch.float32, **kw)
    opt = torch.optim.Adam(list(m.enable_training().parameters()), lr=0.01, weight_decay=0)
    for x, lengths, labels in batches:
        opt.zero_grad()
        loss, _, _ = m.forward_local(torch.from_numpy(x), torch.from_numpy(labels), torch.from_numpy(lengths))
        loss.backward()
        opt.step()
    m.eval()                                                  # the trained tensors, the gates among them, return to the host
    sd = m.state_dict()
    for n in names:
        assert_float_path(sd[n].numpy(), p32[n], p64[n], err_msg=n + ' after 3 Adam steps')
        assert np.abs(sd[n].numpy() - p0[n]).max() > 0, n


def _argv(tmp_path):
    return _cli_argv(tmp_path) + ['--farnn', '2', '--train_mode', 'max']


def test_the_cli_trains_the_gated_model_in_the_max_semiring_for_two_epochs(tmp_path):
    from re2nn_seq_amd import main as cli
    results, stats, res_path = cli.main(_argv(tmp_path))
    steps = stats['train_step']
    assert len(steps) == 2 and all(s['tokens'] > 0 and s['tokens_per_s'] > 0 for s in steps)
    saved = cli.load_res(res_path)
    losses = [float(line.split('LOSS:')[1]) for line in saved['logger'].record if 'TRAIN' in line and 'LOSS:' in line]
    assert len(losses) == 2 and all(np.isfinite(losses))


def test_the_cli_without_the_new_switch_is_refused_before_any_evaluation(tmp_path, monkeypatch):
    from re2nn_seq_amd import main as cli
    from re2nn_seq_amd import train_onehot
    monkeypatch.delenv('RE2NN_DECOMP_IND1_GATED_MAX_TRAIN')

    def boom(*a, **k):
        raise AssertionError('an evaluation ran before the refusal')
    monkeypatch.setattr(train_onehot, 'val_onehot', boom)
    with pytest.raises(NotImplementedError) as e:
        cli.main(_argv(tmp_path))
    assert str(e.value) == MAX_REFUSAL
