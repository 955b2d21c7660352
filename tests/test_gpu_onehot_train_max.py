"""The HIP training step of the onehot i-FST in the max semiring (--train_mode max; farnn_onehot_train_set_semiring;
DESIGN.md, row f5) against the capture of the reference's forward_local(train=True) + loss.backward(), against the float64
restatement (tests/onehot_train_max_ref.py) on gap-checked draws at every size where the kernels take another path, and
through the command line."""
import os

import numpy as np
import pytest
import torch

import onehot_train_max_ref as omr
from test_onehot_train_max_cpu import MIN_GAP, N_CASES, case
from util import assert_float_path, check_grad, ns, present_words

pytestmark = pytest.mark.gpu

NLS = ('none', 'relu', 'tanh', 'relutanh')
EINVAL = -22          # FARNN_EINVAL (include/farnn.h)


def _model(inp, cfg_nl, up, threshold):
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I_S
    S = inp['T'].shape[1]
    pri = inp['P'][:-1, :-1] if up else np.eye(inp['O'].shape[0] - 1)
    a = ns(update_nonlinear=cfg_nl, use_priority=up, threshold=threshold, train_mode='max')
    return FARNN_S_O_I_S(inp['T'], inp['O'], inp['W'], np.zeros(S), inp['hT'], inp['h0'], pri, a, o_idx=inp['o_idx'])


@pytest.mark.parametrize('k', range(N_CASES))
def test_model_mirror_matches_the_reference_capture(k, monkeypatch):
    monkeypatch.setenv('RE2NN_ONEHOT_MAX_TRAIN', '1')
    cfg, inp, ref = case(k)
    m = _model(inp, cfg['update_nonlinear'], cfg['use_priority'], inp['threshold'])
    x, lt, lab = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths']), torch.from_numpy(inp['labels'])
    _, tag_pred, _ = m.forward_local(x, lab, lt, train=False)
    m.train()
    loss, pred, true = m.forward_local(x, lab, lt, train=True)
    loss.backward()
    named = dict(m.named_parameters())
    assert set(named) == {'language_tensor'}
    l64, g64, _ = omr.step(dtype=torch.float64, min_gap=MIN_GAP, **inp)
    assert_float_path(float(loss.detach()), ref['loss'], l64, err_msg='loss')
    assert_float_path(named['language_tensor'].grad.cpu().numpy(), ref['dT'], g64, err_msg='dT')
    assert np.array_equal(pred.cpu().numpy(), ref['flat_pred'])
    assert true.shape == pred.shape
    assert np.array_equal(pred.cpu().numpy(), tag_pred.cpu().numpy())      # the step's tags == the tagging path's


def _context(c, nl='none', semiring='max'):
    from re2nn_seq_amd import _lib
    V, S, _ = c['T'].shape
    return _lib.OnehotTrainContext(V, S, c['O'].shape[0], nl=nl, threshold=0.5, o_idx=0, device=0, semiring=semiring)


def step_c_abi(tc, c):
    """farnn_onehot_ifst_train_step on pre-filled outputs (7.0 in dT, 3.0 in loss, -7 in tags); returns (loss, dT, tags)"""
    dev = torch.device('cuda', 0)
    w = {n: torch.from_numpy(np.ascontiguousarray(c[n], dtype=np.float32)).to(dev) for n in ('T', 'W', 'O', 'h0', 'hT')}
    P = None if c.get('P') is None else torch.from_numpy(np.ascontiguousarray(c['P'], dtype=np.float32)).to(dev)
    x, lengths, labels = (torch.from_numpy(np.ascontiguousarray(c[n])).to(dev) for n in ('x', 'lengths', 'labels'))
    B, L = c['x'].shape
    dT = torch.full_like(w['T'], 7.0)
    loss = torch.full((1,), 3.0, device=dev)
    tags = torch.full((B, L), -7, dtype=torch.int32, device=dev)
    try:
        tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None if P is None else P.data_ptr()), x.data_ptr(),
                lengths.data_ptr(), labels.data_ptr(), B, L, max(int(np.clip(c['lengths'], 0, L).sum()), c.get('ntok', 0)),
                dict(loss=loss.data_ptr(), dT=dT.data_ptr(), tags=tags.data_ptr()))
    finally:
        torch.cuda.synchronize()
    return float(loss), dT.cpu().numpy(), tags.cpu().numpy()


def real_case(V, S, C, B, L, seed, priority=False, per_column=4, negative=False):
    """A real-valued model and a batch with one empty and one full-length sequence where B > 3.  per_column: the expected
    non-zero candidates of a maximum (None: dense) -- few candidates keep the top two apart; their magnitudes are spread
    over e^-2..1.  negative: M < 0 everywhere and h0, hT > 0."""
    rng = np.random.RandomState(seed)

    def mat(shape, k):
        v = np.exp(rng.uniform(-2.0, 0.0, size=shape)) * (-1.0 if negative else rng.choice([-1.0, 1.0], size=shape))
        if k is not None and S > k:
            v = v * (rng.rand(*shape) < float(k) / S)
        return v.astype(np.float32)
    T = mat((V, S, S), per_column)
    W = mat((S, S), None if per_column is None else 1) * np.float32(0.5)
    O = (rng.uniform(0.2, 1.8, size=(C, S)) / C).astype(np.float32)          # o = O.sum(0) is about 1
    sign = 1.0 if negative else rng.choice([-1.0, 1.0], size=(2, S))
    h0, hT = (rng.uniform(0.5, 1.5, size=(2, S)) * sign).astype(np.float32)
    lengths = rng.randint(1, L + 1, size=B).astype(np.int64)
    lengths[0] = L
    if B > 3:
        lengths[2] = 0
    x = rng.randint(0, V, size=(B, L)).astype(np.int64)
    labels = rng.randint(0, C, size=(B, L)).astype(np.int64)
    P = None
    if priority:
        P = np.eye(C, dtype=np.float32)
        P[rng.randint(0, C, 4), rng.randint(0, C, 4)] = -1.0
    return dict(T=T, W=W, O=O, h0=h0, hT=hT, P=P, x=x, lengths=lengths, labels=labels)


def gap_checked(draw, nl, seed0, tries=40):
    """the first of `tries` seeded draws that the gap rule accepts"""
    for seed in range(seed0, seed0 + tries):
        c = draw(seed)
        try:
            omr.check_gap(c['T'], c['W'], c['O'], c['h0'], c['hT'], c['x'], c['lengths'], nl, MIN_GAP)
            return c
        except omr.GapError:
            continue
    pytest.fail('no draw in {} seeds passes the gap rule'.format(tries))


def _against_restatement(c, nl, name):
    tc = _context(c, nl)
    try:
        loss, dT, tags = step_c_abi(tc, c)
    finally:
        tc.close()
    l32, g32, p32 = omr.step(dtype=torch.float32, nl=nl, **c)
    l64, g64, p64 = omr.step(dtype=torch.float64, nl=nl, **c)
    assert_float_path(loss, l32, l64, err_msg=name + ' loss')
    check_grad(name, 'dT', dT, g32, g64, slices=0, present=present_words(c['x'], c['lengths'], dT.shape[0]))
    return loss, dT, tags


@pytest.mark.parametrize('S,B,L,nl,up', [(1, 1, 1, 'tanh', False), (14, 5, 1, 'none', True), (63, 4, 6, 'relu', False),
                                         (64, 4, 6, 'tanh', True), (65, 4, 6, 'relutanh', False), (71, 4, 6, 'none', False),
                                         (127, 3, 5, 'relutanh', True), (128, 3, 5, 'relu', True)])
def test_c_abi_against_the_float64_restatement(S, B, L, nl, up):
    V, C = (60, 9) if S > 1 else (5, 3)
    c = gap_checked(lambda seed: real_case(V, S, C, B, L, seed, priority=up, per_column=None if S <= 14 else 4), nl,
                    seed0=1000 * S + 10 * B + L)
    assert c['lengths'].max() == L and (B <= 3 or c['lengths'].min() == 0)
    _against_restatement(c, nl, 'onehot max S{} B{} L{} {}'.format(S, B, L, nl))


@pytest.mark.parametrize('S', [14, 65, 71])
def test_all_candidates_negative(S):
    """nl = none, h0 and hT > 0, M < 0 everywhere: every candidate of the first step is negative, so a padded row or an
    unused register slot that entered the comparison as 0 would win it and change the loss"""
    c = gap_checked(lambda seed: real_case(40, S, 6, 2, 3, seed, per_column=None, negative=True), 'none', seed0=7000 + S)
    assert (c['T'] + c['W']).max() < 0 and min(c['h0'].min(), c['hT'].min()) > 0
    _against_restatement(c, 'none', 'onehot max negative S{}'.format(S))


def test_ties_go_to_the_first_index():
    """one-hot h0 / hT with relu on a 0/1 automaton (ifst_small's tensors): structurally identical paths tie exactly"""
    _, inp, _ = case(2)
    c = {k: inp[k] for k in ('T', 'W', 'O', 'P', 'x', 'lengths', 'labels')}
    S = c['T'].shape[1]
    c['h0'] = np.eye(S, dtype=np.float32)[int(np.argmax(inp['h0']))]
    c['hT'] = np.eye(S, dtype=np.float32)[int(np.argmax(inp['hT']))]
    omr.check_gap(c['T'], c['W'], c['O'], c['h0'], c['hT'], c['x'], c['lengths'], 'relu', MIN_GAP)
    _against_restatement(c, 'relu', 'onehot max ties')


def _large_case(seed):
    return real_case(300, 71, 20, 32, 16, seed)


def test_two_steps_are_bit_identical():
    c = _large_case(5)
    tc = _context(c)
    try:
        l1, g1, t1 = step_c_abi(tc, c)
        l2, g2, t2 = step_c_abi(tc, c)
    finally:
        tc.close()
    assert np.isfinite(l1) and np.isfinite(g1).all() and g1.any()
    assert l1 == l2 and np.array_equal(g1, g2) and np.array_equal(t1, t2)


def test_a_context_switched_back_to_sum_equals_a_fresh_sum_context():
    c = _large_case(6)
    fresh = _context(c, semiring='sum')
    tc = _context(c, semiring='max')
    try:
        ls, gs, ts = step_c_abi(fresh, c)
        lm, gm, _ = step_c_abi(tc, c)
        tc.set_semiring('sum')
        l2, g2, t2 = step_c_abi(tc, c)
    finally:
        fresh.close()
        tc.close()
    assert lm != ls and not np.array_equal(gm, gs)          # the two semirings differ on this draw
    assert l2 == ls and np.array_equal(g2, gs) and np.array_equal(t2, ts)


def test_refused_inputs_leave_the_outputs_untouched():
    from re2nn_seq_amd import _lib
    c = real_case(20, 14, 5, 3, 4, seed=8)
    tc = _context(c)
    try:
        for bad in (2, -1, 7):
            assert _lib.load().farnn_onehot_train_set_semiring(tc._raw, bad) == EINVAL
        assert _lib.load().farnn_onehot_train_set_semiring(None, 1) == EINVAL
        refused = dict(c, lengths=np.zeros_like(c['lengths']))          # valid_tokens = 0
        with pytest.raises(_lib.FarnnError):
            step_c_abi(tc, refused)
        # pre-filled buffers of a refused step: read back through a step whose arguments are refused
        dev = torch.device('cuda', 0)
        dT = torch.full((20, 14, 14), 7.0, device=dev)
        loss = torch.full((1,), 3.0, device=dev)
        tags = torch.full((3, 4), -7, dtype=torch.int32, device=dev)
        w = {n: torch.from_numpy(c[n]).to(dev) for n in ('T', 'W', 'O', 'h0', 'hT')}
        x, lengths, labels = (torch.from_numpy(c[n]).to(dev) for n in ('x', 'lengths', 'labels'))
        outs = dict(loss=loss.data_ptr(), dT=dT.data_ptr(), tags=tags.data_ptr())
        with pytest.raises(_lib.FarnnError):
            tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None), x.data_ptr(), lengths.data_ptr(), labels.data_ptr(),
                    3, 4, 0, outs)
        with pytest.raises(_lib.FarnnError):                                # B (L+1) >= 2^30: FARNN_ERANGE before any launch
            tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None), x.data_ptr(), lengths.data_ptr(), labels.data_ptr(),
                    1 << 20, 1 << 10, 5, outs)
        torch.cuda.synchronize()
        assert (dT == 7.0).all() and float(loss) == 3.0 and (tags == -7).all()
        l, g, _ = step_c_abi(tc, c)                                       # the context still works
        assert np.isfinite(l) and np.isfinite(g).all()
    finally:
        tc.close()


def _adam_on_the_device(c, batches, nl, lr, semiring='max'):
    """Adam steps (torch.optim.Adam) on the library step; returns (language_tensor, losses)"""
    from re2nn_seq_amd.farnn.train_step import onehot_ifst_train_step
    dev = torch.device('cuda', 0)
    tc = _context(c, nl, semiring)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    Tt = d(c['T']).requires_grad_(True)
    W, O, h0, hT = d(c['W']), d(c['O']), d(c['h0']), d(c['hT'])
    opt = torch.optim.Adam([Tt], lr=lr, weight_decay=0)
    losses = []
    try:
        for x, lengths, labels in batches:
            opt.zero_grad()
            loss, _ = onehot_ifst_train_step(tc, Tt, W, O, h0, hT, None, torch.from_numpy(x), torch.from_numpy(lengths),
                                             torch.from_numpy(labels))
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        torch.cuda.synchronize()
    finally:
        tc.close()
    return Tt.detach().cpu().numpy(), losses


def _adam_case(seed, n_batches, V=30, S=20, C=6, B=6, L=5):
    c = real_case(V, S, C, B, L, seed)
    rng = np.random.RandomState(seed + 1)
    batches = []
    for _ in range(n_batches):
        lengths = rng.randint(1, L + 1, size=B).astype(np.int64)
        batches.append((rng.randint(0, V, size=(B, L)).astype(np.int64), lengths,
                        rng.randint(0, C, size=(B, L)).astype(np.int64)))
    return c, batches


def test_three_adam_steps_against_the_restatement():
    nl, lr = 'tanh', 0.01
    for seed in range(300, 340):
        c, batches = _adam_case(seed, 3)
        kw = dict(W=c['W'], O=c['O'], h0=c['h0'], hT=c['hT'], P=None, batches=batches, nl=nl, lr=lr)
        try:
            r64 = omr.adam_steps(c['T'], dtype=torch.float64, min_gap=MIN_GAP, **kw)
            r32 = omr.adam_steps(c['T'], dtype=torch.float32, min_gap=MIN_GAP, **kw)
            break
        except omr.GapError:
            continue
    else:
        pytest.fail('no draw in 40 seeds keeps the gap rule over three steps')
    got, losses = _adam_on_the_device(c, batches, nl, lr)
    assert np.isfinite(losses).all()
    assert_float_path(got, r32, r64, err_msg='language_tensor after 3 Adam steps')


ADAM30 = dict(seed=400, lr=0.1, nl='tanh')        # chosen on the CPU: the float64 restatement ends at 0.69 of its first loss


def test_thirty_adam_steps_lower_the_loss():
    c, batches = _adam_case(ADAM30['seed'], 1)
    batches = batches * 30
    ref = []
    omr.adam_steps(c['T'], c['W'], c['O'], c['h0'], c['hT'], None, batches, nl=ADAM30['nl'], lr=ADAM30['lr'],
                   dtype=torch.float64, losses=ref)
    assert ref[-1] < 0.8 * ref[0], ref
    _, losses = _adam_on_the_device(c, batches, ADAM30['nl'], ADAM30['lr'])
    assert np.isfinite(losses).all() and losses[-1] < 0.9 * losses[0], losses


def test_onehot_cli_trains_two_epochs_in_the_max_semiring(tmp_path, monkeypatch):
    """--method onehot --independent 2 --train_mode max --epoch 2 with the switch set, on the synthetic tree"""
    from re2nn_seq_amd import main as cli
    from re2nn_seq_amd import synth
    monkeypatch.setenv('RE2NN_ONEHOT_MAX_TRAIN', '1')
    tree = synth.write_dataset_tree(str(tmp_path / 'data'), dataset='ATIS-BIO', seed=4)
    argv = ['--dataset', 'ATIS-BIO', '--method', 'onehot', '--independent', '2', '--train_mode', 'max',
            '--automata_path', tree['paths']['ID2'], '--normalize_automata', 'none', '--rand_constant', '0',
            '--update_nonlinear', 'tanh', '--bz', '9', '--seq_max_len', '12', '--epoch', '2', '--lr', '0.01',
            '--train_portion', '1.0', '--data_dir', tree['paths']['data_dir'], '--model_dir', str(tmp_path / 'm')]
    results, stats, res_path = cli.main(argv)
    assert len(stats['train_step']) == 2
    assert os.path.exists(res_path)
    saved = cli.load_res(res_path)
    losses = [float(line.split('LOSS:')[1]) for line in saved['logger'].record if 'LOSS:' in line]
    assert len(losses) == 2 and np.isfinite(losses).all()
    assert saved['args'].train_mode == 'max'

