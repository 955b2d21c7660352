"""The HIP training step of the decomposed independent=1 model under the CRF (FARNN_S_D_W_I, --use_crf 1):
the model mirror against the captures of the reference, the C-ABI (farnn_decomp_ind1_crf_train_step) against the torch
restatement (tests/decomp1_crf_train_ref.py) at the shape edges of the CRF kernel, determinism, the tagging handle after a
step, the command line and the refusals."""
import numpy as np
import pytest
import torch

import decomp1_crf_train_ref as dcr
import decomp1_train_ref as dtr
from test_decomp1_crf_train_cpu import N_CASES, NAMED, case, model
from test_decomp1_train_cpu import check_all_grads
from test_gpu_decomp1_train import ABI, GUARD, NAMES
from test_gpu_decomp1_train import run_step_c_abi as run_plain_step
from util import assert_float_path, present_words

pytestmark = pytest.mark.gpu
LDS_LIMIT = 160 * 1024


def crf_lds_bytes(K, L, big):
    """train_crf_lds_bytes (csrc/train.hip.h), the carve of the CRF kernels"""
    floats = (1 if big else 3) * K * (K + 1) + (2 if big else 3) * L * K + L + 5 * K + 8
    return floats * 4 + ((L * K + 3) & ~3)


def first_c_beyond(L, big):
    return next(C for C in range(4, 400) if crf_lds_bytes(C, L, big) > LDS_LIMIT)


EDGE_L = 8
C_BIG = first_c_beyond(EDGE_L, False)         # the first C whose three tables leave LDS: the large-tag-set form
C_REFUSED = first_c_beyond(EDGE_L, True)      # the first C even that form cannot hold


@pytest.fixture(autouse=True)
def _opt_in(monkeypatch):
    monkeypatch.setenv('RE2NN_DECOMP_IND1_TRAIN', '1')
    monkeypatch.setenv('RE2NN_DECOMP_IND1_CRF_TRAIN', '1')
    monkeypatch.setenv('RE2NN_BUCKETED_MAX_TRAIN', '1')


@pytest.mark.parametrize('k', range(N_CASES))
def test_model_mirror_matches_the_reference_capture(k):
    cfg, inp, ref = case(k)
    m = model(k)
    x, lt, lab = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths']), torch.from_numpy(inp['labels'])
    m.train()
    loss, pred, true = m.forward_local(x, lab, lt, train=True)
    loss.backward()
    named = dict(m.named_parameters())
    assert set(named) == set(NAMED)
    l64, g64, _ = dcr.step(dtype=torch.float64, **inp)
    assert_float_path(float(loss.detach()), ref['loss'], l64, err_msg='loss')
    present = present_words(inp['x'], inp['lengths'], inp['p']['V_embed'].shape[0])
    check_all_grads('decomp1 crf capture c{}'.format(k), {n: t.grad.cpu().numpy() for n, t in named.items()}, ref['grads'], g64,
                    present)
    assert np.array_equal(pred.cpu().numpy(), ref['flat_pred'])
    assert true.shape == pred.shape


def test_named_parameters_hold_crf_transitions_exactly_when_use_crf():
    for use_crf in (0, 1):
        m = model(0, use_crf=use_crf).enable_training()
        assert (dcr.TRANS in dict(m.named_parameters())) == bool(use_crf)


def make_case(V, S, R, RO, C, B, L, seed, lengths=None, priority=False, nl='relu', semiring='sum'):
    """a signed real-valued case with C - 2 labels that keeps the gap rule (decomp1_crf_train_ref.check_gap), drawn again (next
    seed) until the float64 restatement's gradients are live, the float32 restatement sits within a tenth of the bar
    (decomp1_train_ref.badly_drawn) and both decode alike -- conditions read off the restatement alone"""
    why = None
    for attempt in range(60):
        try:
            c = _draw(V, S, R, RO, C, B, L, seed + 1000 * attempt, lengths, priority, nl, semiring)
        except (dtr.GapError, dcr.dmr.GapError) as e:
            why = str(e)
            continue
        present = present_words(c['x'], c['lengths'], V)
        r32, r64 = dcr.step(dtype=torch.float32, **c), dcr.step(dtype=torch.float64, **c)
        why = dtr.badly_drawn(r32[1], r64[1], present)
        if why is None and not np.array_equal(r32[2], r64[2]):
            why = 'float32 and float64 decode differently'
        if why is None:
            c['_ref'] = (r32, r64)
            return c
    raise AssertionError('no live case in 60 draws: ' + str(why))


def _draw(V, S, R, RO, C, B, L, seed, lengths, priority, nl, semiring):
    rng = np.random.RandomState(seed)
    p = dtr.signed_base(V, S, R, RO, C, rng)
    if lengths is None:
        lengths = rng.randint(1, L + 1, size=B)
        lengths[0] = L
    lengths = np.asarray(lengths, np.int64)
    x = rng.randint(0, V, size=(B, L)).astype(np.int64)
    labels = rng.randint(0, C - 2, size=(B, L)).astype(np.int64)
    trans = dcr.default_transitions(C)
    trans += np.where(trans > -5000.0, rng.uniform(-0.5, 0.5, size=(C, C)), 0.0).astype(np.float32)
    P = None
    if priority:
        P = np.eye(C, dtype=np.float32)
        P[rng.randint(0, C, 4), rng.randint(0, C, 4)] = -1.0
    dcr.check_gap(p, P, trans, x, lengths, nl=nl, semiring=semiring)
    return dict(p=p, P=P, trans=trans, x=x, lengths=lengths, labels=labels, nl=nl, semiring=semiring)


def _ctx(c):
    from re2nn_seq_amd import _lib
    p = c['p']
    V, R = p['Vgen'].shape
    C, RO = p['C_output'].shape
    return _lib.Decomp1TrainContext(V, p['S1'].shape[0], R, RO, C, nl=c['nl'], semiring=c['semiring'])


def run_crf_step(c, tc=None, expect_error=None, trans_null=False, dtrans_null=False):
    """farnn_decomp_ind1_crf_train_step on pre-filled outputs with guard elements around every output and around dtrans;
    returns (loss, grads with 'crf.transitions', tags) and asserts that the guards are untouched.  expect_error: the step must
    raise FarnnError with that word in it and leave every output as pre-filled"""
    from re2nn_seq_amd import _lib
    dev = torch.device('cuda', 0)
    p = c['p']
    C = p['C_output'].shape[0]
    own = tc is None
    tc = _ctx(c) if own else tc
    try:
        w = {n: torch.from_numpy(np.ascontiguousarray(p[n], dtype=np.float32)).to(dev) for n in NAMES}
        P = None if c['P'] is None else torch.from_numpy(np.ascontiguousarray(c['P'], dtype=np.float32)).to(dev)
        tr = torch.from_numpy(np.ascontiguousarray(c['trans'], dtype=np.float32)).to(dev)
        x, lengths, labels = (torch.from_numpy(np.ascontiguousarray(c[n])).to(dev) for n in ('x', 'lengths', 'labels'))
        B, L = c['x'].shape
        bufs = {n: torch.full((w[n].numel() + 2 * GUARD,), 7.0, device=dev) for n in NAMES}
        bufs[dcr.TRANS] = torch.full((C * C + 2 * GUARD,), 7.0, device=dev)
        tags = torch.full((B * L + 2 * GUARD,), 77, dtype=torch.int32, device=dev)
        loss = torch.full((1 + 2 * GUARD,), 3.0, device=dev)
        out = {'d' + ABI[n]: bufs[n].data_ptr() + GUARD * 4 for n in NAMES}
        out.update(loss=loss.data_ptr() + GUARD * 4, tags=tags.data_ptr() + GUARD * 4)
        args = (dict({ABI[n]: t.data_ptr() for n, t in w.items()}, P=None if P is None else P.data_ptr()),
                None if trans_null else tr.data_ptr(), x.data_ptr(), lengths.data_ptr(), labels.data_ptr(), B, L,
                int(np.clip(c['lengths'], 0, L).sum()), out, None if dtrans_null else bufs[dcr.TRANS].data_ptr() + GUARD * 4)
        torch.cuda.synchronize()
        if expect_error is not None:
            with pytest.raises(_lib.FarnnError) as e:
                tc.step_crf(*args)
            assert expect_error in str(e.value), str(e.value)
        else:
            tc.step_crf(*args)
        torch.cuda.synchronize()
        h = {n: t.cpu().numpy() for n, t in bufs.items()}
        ht, hl = tags.cpu().numpy(), loss.cpu().numpy()
        if expect_error is not None:
            assert all((a == 7.0).all() for a in h.values()) and (ht == 77).all() and (hl == 3.0).all(), 'a refused step wrote'
            return None
        for n in h:
            assert (h[n][:GUARD] == 7.0).all() and (h[n][-GUARD:] == 7.0).all(), 'guard elements around d{} overwritten'.format(n)
        assert (ht[:GUARD] == 77).all() and (ht[-GUARD:] == 77).all(), 'guard elements around tags overwritten'
        assert (hl[:GUARD] == 3.0).all() and (hl[-GUARD:] == 3.0).all(), 'guard elements around loss overwritten'
        grads = {n: h[n][GUARD:-GUARD].reshape(p[n].shape) for n in NAMES}
        grads[dcr.TRANS] = h[dcr.TRANS][GUARD:-GUARD].reshape(C, C)
        return float(hl[GUARD]), grads, ht[GUARD:-GUARD].reshape(B, L)
    finally:
        if own:
            tc.close()


def check_case(name, c):
    (l32, g32, p32), (l64, g64, p64) = c['_ref']
    loss, grads, tags = run_crf_step(c)
    assert_float_path(loss, l32, l64, err_msg=name + ' loss')
    present = present_words(c['x'], c['lengths'], grads['Vgen'].shape[0])
    check_all_grads(name, grads, g32, g64, present)          # crf.transitions among them
    assert not grads['Vgen'][~present].any(), 'the row of an absent word is not zero'
    B, L = c['x'].shape
    valid = np.arange(L)[None, :] < np.clip(c['lengths'], 0, L)[:, None]
    assert (tags[~valid] == -1).all()
    assert np.array_equal(tags[valid], p64)
    return loss, grads, tags


def test_the_thresholds_are_the_kernels():
    """what the cases below rely on, read off bucketed_crf_kernel's conditions (csrc/train_bucketed_crf.hip.h): the expected
    counts stay in registers while a thread owns at most 32 rows of a column (256 threads over K + 1 columns)"""
    def xreg(K):
        step = max(256 // (K + 1), 1)
        return K + 1 <= 256 and (K + step - 1) // step <= 32
    assert xreg(84) and not xreg(85)
    assert 85 < C_BIG < C_REFUSED - 1 and C_REFUSED - 1 <= 255         # (the back-pointers are bytes)
    assert crf_lds_bytes(C_REFUSED - 1, EDGE_L, True) <= LDS_LIMIT < crf_lds_bytes(C_REFUSED, EDGE_L, True)


# C = 4: the smallest accepted; 7: the dot products' tail; 84 | 85: the expected counts leave the registers; C_BIG: the first
# large-tag-set form; C_REFUSED - 1: the last size accepted at this L.  Lengths 0, 1 and L in one batch; with and without a signed
# priority matrix; both semirings
@pytest.mark.parametrize('C,priority,semiring', [(4, False, 'sum'), (4, True, 'max'), (7, True, 'sum'), (7, False, 'max'),
                                                 (84, True, 'sum'), (84, False, 'max'), (85, False, 'sum'), (85, True, 'max'),
                                                 (C_BIG - 1, False, 'sum'), (C_BIG, True, 'sum'), (C_BIG, False, 'max'),
                                                 (C_REFUSED - 1, True, 'sum')])
def test_tag_counts_at_the_crf_kernels_edges(C, priority, semiring):
    c = make_case(9, 6, 4, 5, C, 5, EDGE_L, seed=800 + C, lengths=[EDGE_L, 0, 1, 3, EDGE_L - 1], priority=priority,
                  nl='tanh' if C % 2 else 'relu', semiring=semiring)
    check_case('decomp1 crf C{} {}'.format(C, semiring), c)


def test_a_batch_of_one_token_and_a_batch_with_only_one_valid_sequence():
    check_case('decomp1 crf B1 L1', make_case(5, 4, 3, 3, 5, 1, 1, seed=31, lengths=[1], nl='none'))
    check_case('decomp1 crf one valid', make_case(5, 4, 3, 3, 6, 3, 4, seed=32, lengths=[0, 4, 0], priority=True))


def test_the_first_tag_count_beyond_lds_is_refused_with_the_outputs_untouched():
    """FARNN_ERANGE at the plan stage, naming the quantity; C < 4 and the null pointers: FARNN_EINVAL.  The inputs are never
    read, so an undrawn case stands in"""
    def stub(C, L=EDGE_L):
        rng = np.random.RandomState(C)
        p = dtr.signed_base(6, 4, 3, 3, C, rng)
        return dict(p=p, P=None, trans=dcr.default_transitions(C), x=rng.randint(0, 6, size=(2, L)).astype(np.int64),
                    lengths=np.array([L, 1], np.int64), labels=np.zeros((2, L), np.int64), nl='relu', semiring='sum')
    run_crf_step(stub(C_REFUSED), expect_error='LDS')
    run_crf_step(stub(3), expect_error='at least 4 score columns')
    run_crf_step(stub(6), expect_error='transitions', trans_null=True)
    run_crf_step(stub(6), expect_error='transitions', dtrans_null=True)


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[2], b[2]) and all(np.array_equal(a[1][n], b[1][n]) for n in a[1])


@pytest.mark.parametrize('C,semiring', [(7, 'sum'), (85, 'max'), (C_BIG, 'sum')])
def test_two_steps_are_bit_identical_and_the_plain_step_is_a_fresh_contexts(C, semiring):
    c = make_case(9, 6, 4, 5, C, 5, EDGE_L, seed=900 + C, lengths=[EDGE_L, 0, 1, 3, 5], priority=True, semiring=semiring)
    tc = _ctx(c)
    a = run_crf_step(c, tc=tc)
    b = run_crf_step(c, tc=tc)
    assert _same(a, b)
    # the plain step (the cross-entropy over all C columns) on the context that ran the CRF step, and on a fresh one
    plain = {k: v for k, v in c.items() if k not in ('trans', 'semiring', '_ref')}
    used = run_plain_step(plain, tc=tc)
    tc.close()
    fresh_tc = _ctx(c)
    fresh = run_plain_step(plain, tc=fresh_tc)
    fresh_tc.close()
    assert _same(used, fresh)


def _adam_step(m, x, lab, lt):
    opt = torch.optim.Adam(list(m.enable_training().parameters()), lr=0.05, weight_decay=0)
    opt.zero_grad()
    loss, _, _ = m.forward_local(x, lab, lt, train=True)
    loss.backward()
    opt.step()


@pytest.mark.parametrize('k', [2, 6, 9])
def test_training_and_tagging_decode_alike_after_an_adam_step(k):
    """the same weights and the same Viterbi through two kernels: the tags of forward_local(train=False) after one Adam step
    equal the tags the next training step returns on that batch (a capture whose weights after the step keep the gap rule)"""
    cfg, inp, _ = case(k)
    m = model(k)
    x, lt, lab = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths']), torch.from_numpy(inp['labels'])
    before = m.state_dict()[dcr.TRANS].clone()
    _adam_step(m, x, lab, lt)
    _, tagged, _ = m.forward_local(x, lab, lt, train=False)
    sd = {n: t.detach().cpu().numpy() for n, t in m.state_dict().items()}
    assert np.abs(sd[dcr.TRANS] - before.numpy()).max() > 0
    after = dict(inp, p={n: sd[n] for n in inp['p']}, trans=sd[dcr.TRANS])
    dcr.check_gap(min_gap=0.0, **{q: v for q, v in after.items() if q != 'labels'})
    _, trained, _ = m.forward_local(x, lab, lt, train=True)
    assert np.array_equal(tagged.cpu().numpy(), trained.cpu().numpy())
    assert np.array_equal(trained.cpu().numpy(), dcr.step(dtype=torch.float64, **after)[2])


def _cli_argv(tmp_path):
    from test_gpu_decomp1_train import _cli_argv as plain
    return plain(tmp_path) + ['--use_crf', '1']


@pytest.mark.parametrize('native', [False, True])
def test_decompose_independent1_crf_cli_trains_for_two_epochs(tmp_path, monkeypatch, native):
    """--method decompose --independent 1 --use_crf 1 --epoch 2 through train_epochs, with torch.optim.Adam and with
    RE2NN_NATIVE_OPTIM=1 (the transitions are one more tensor of the one-launch step); the loss falls from the first epoch,
    which starts at the INIT weights, to the second"""
    from re2nn_seq_amd import main as cli
    if native:
        monkeypatch.setenv('RE2NN_NATIVE_OPTIM', '1')
    results, stats, res_path = cli.main(_cli_argv(tmp_path))
    steps = stats['train_step']
    assert len(steps) == 2 and all(s['tokens'] > 0 and s['tokens_per_s'] > 0 for s in steps)
    saved = cli.load_res(res_path)
    losses = [float(line.split('LOSS:')[1]) for line in saved['logger'].record if 'TRAIN' in line and 'LOSS:' in line]
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[1] < losses[0], losses


def test_the_cli_without_the_crf_switch_is_refused_before_any_evaluation(tmp_path, monkeypatch):
    from re2nn_seq_amd import main as cli
    from re2nn_seq_amd import train_onehot
    from test_decomp1_crf_train_cpu import CRF_REFUSAL
    monkeypatch.delenv('RE2NN_DECOMP_IND1_CRF_TRAIN')

    def boom(*a, **k):
        raise AssertionError('an evaluation ran before the refusal')
    monkeypatch.setattr(train_onehot, 'val_onehot', boom)
    with pytest.raises(NotImplementedError) as e:
        cli.main(_cli_argv(tmp_path))
    assert str(e.value) == CRF_REFUSAL
