"""GPU checks of the decomposed FST's training step in the max semiring (FARNN_S_D_W, --train_mode max): the
model mirror against every capture of the reference (tests/golden/decomp0_train_max_small), the C-ABI against the float32 /
float64 restatement (tests/decomp0_max_train_ref.py) on the drawn cases of tests/decomp0_max_train_cases.py, exact ties,
bit-identical repeats, sum -> max -> sum on one context, the decomposed i-FST's own max step before and after, the refusals, and
three Adam steps through train_onehot.train_epochs."""
import numpy as np
import pytest
import torch

import decomp0_max_train_cases as cases
import decomp0_max_train_ref as d0m
import test_gpu_decomp0_train as sum_gpu
from util import assert_float_path, check_grad

pytestmark = pytest.mark.gpu

GUARD = 12345.0
EINVAL, ERANGE = -22, -34       # FARNN_EINVAL, FARNN_ERANGE (include/farnn.h)


def context(case, semiring='max'):
    from re2nn_seq_amd import _lib
    p = case['p']
    V, R = p['Vgen'].shape
    S, Q = p['S1_wildcard'].shape
    return _lib.DecompFstTrainContext(V, S, R, Q, p['C_embed'].shape[0], nl=case['nl'], threshold=0.5, o_idx=0, device=0,
                                      use_crf=case['trans'] is not None, farnn=case['farnn'], sigmoid_exponent=case['k'],
                                      semiring=semiring)


def run_max(case, tc=None):
    """one library step in the max semiring (or on the context given); (loss, {restatement name: gradient}, tags [B, L])"""
    own = tc is None
    if own:
        tc = context(case)
    try:
        return sum_gpu.run_lib(case, tc=tc)
    finally:
        if own:
            tc.close()


def same_bytes(a, b):
    assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes()
    assert set(a[1]) == set(b[1])
    for n in a[1]:
        assert a[1][n].tobytes() == b[1][n].tobytes(), n
    assert np.array_equal(a[2], b[2])


def check_case(name, case):
    loss, grads, tags = run_max(case)
    assert_float_path(loss, case['l32'], case['l64'], err_msg=name + ' loss')
    assert set(grads) == set(case['g64'])
    for n in sorted(case['g64']):
        word = n == 'Vgen'
        check_grad(name, n, grads[n].reshape(case['g64'][n].shape), case['g32'][n], case['g64'][n], slices=0 if word else None,
                   present=case['present'] if word else None)
    assert not grads['Vgen'][~case['present']].any(), 'a row of dVgen of an absent word is not exactly 0'
    L = case['x'].shape[1]
    mask = np.arange(L)[None, :] < np.clip(case['lengths'], 0, L)[:, None]
    assert np.array_equal(tags[mask].astype(np.int64), case['pred'])
    assert (tags[~mask] == -1).all()
    return loss, grads, tags


# ---- the decomposed i-FST's own max step (row f3), first in this module: before any max step of the decomposed FST ---------------
def _ifst_max_step(w, x, ln, lab, K):
    from re2nn_seq_amd import _lib
    dev = torch.device('cuda', 0)
    B, L = x.shape
    V, R = w['Vgen'].shape
    tc = _lib.TrainContext(V, w['S1'].shape[0], R, K, nl='tanh', semiring='max')
    t = {n: torch.from_numpy(a).to(dev) for n, a in w.items()}
    g = {n: torch.zeros_like(a) for n, a in t.items()}
    loss = torch.zeros(1, device=dev)
    tags = torch.zeros((B, L), dtype=torch.int32, device=dev)
    outs = dict({'d' + n: a.data_ptr() for n, a in g.items()}, loss=loss.data_ptr(), tags=tags.data_ptr())
    xd, ld, labd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, ln, lab))
    tc.step({n: a.data_ptr() for n, a in t.items()}, xd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, int(ln.sum()), outs,
            torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    tc.close()
    return float(loss.cpu()), {n: a.cpu().numpy() for n, a in g.items()}, tags.cpu().numpy()


def test_the_ifst_max_step_is_not_disturbed():
    """The decomposed i-FST's max step on a fixed batch, before any max step of the decomposed FST in this module and after one.
    That step adds with float atomics: its bits are its own from run to run only where every sum has at most
    two addends -- one sequence of two distinct words.  There the bits are equal; on a ragged 4 x 6 batch the tags are equal and
    the sums agree to the atomics' order."""
    rng = np.random.RandomState(3)
    V, S, R, K, B, L = 12, 9, 6, 5, 4, 6
    base = d0m.signed_base(V, S, R, 4, K, rng)
    w = {'Vgen': base['Vgen'], 'S1': base['S1'], 'S2': base['S2'], 'W': base['wildcard_wildcard'],
         'C': np.abs(rng.choice([0.5, 1.0], size=(K, S))).astype(np.float32), 'h0': base['h0'], 'hT': base['hT']}
    x = rng.randint(0, V, size=(B, L)).astype(np.int64)
    ln = np.array([6, 1, 4, 3], np.int64)
    lab = rng.randint(0, K, size=(B, L)).astype(np.int64)
    two = (np.array([[3, 7]], np.int64), np.array([2], np.int64), lab[:1, :2].copy())
    two_before, before = _ifst_max_step(w, *two, K), _ifst_max_step(w, x, ln, lab, K)
    run_max(cases.get_case('farnn2-ce1')[0])
    two_after, after = _ifst_max_step(w, *two, K), _ifst_max_step(w, x, ln, lab, K)
    assert np.float32(two_before[0]).tobytes() == np.float32(two_after[0]).tobytes() and np.array_equal(two_before[2], two_after[2])
    for n in two_before[1]:
        assert two_before[1][n].tobytes() == two_after[1][n].tobytes(), n
    assert any(np.abs(g).max() > 0 for g in two_before[1].values())
    assert np.array_equal(before[2], after[2])
    assert abs(before[0] - after[0]) <= 1e-6 * (1 + abs(before[0]))
    for n in before[1]:
        np.testing.assert_allclose(after[1][n], before[1][n], rtol=1e-5, atol=1e-6 * np.abs(before[1][n]).max(), err_msg=n)


# ---- the C-ABI against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(cases.CASES))
def test_step_matches_the_restatement(name):
    check_case('d0max-' + name, cases.get_case(name)[0])


def test_193_states_are_refused_and_192_accepted():
    from re2nn_seq_amd import _lib
    tc = _lib.DecompFstTrainContext(3, 193, 3, 2, 3, nl='tanh')
    try:
        with pytest.raises(_lib.FarnnError, match=r'code {}: .*at most 192 states'.format(ERANGE)):
            tc.set_semiring('max')
        assert tc.semiring == 'sum'
        with pytest.raises(_lib.FarnnError, match='code {}'.format(EINVAL)):
            _lib.check(getattr(_lib.load(), 'farnn_decomp_fst_train_set_semiring')(tc._raw, 7), 'set_semiring')
    finally:
        tc.close()
    tc = _lib.DecompFstTrainContext(3, 192, 3, 2, 3, nl='tanh', semiring='max')
    assert tc.semiring == 'max'
    tc.close()


def tie_case(farnn=0):
    """one-hot h0 / hT, relu and 0 / 1 factors: every candidate is 0 or a small integer, the maxima tie exactly all over"""
    rng = np.random.RandomState(5)
    V, S, R, Q, K, B, L = 6, 12, 4, 3, 4, 3, 4
    f = lambda *s: (rng.rand(*s) < 0.4).astype(np.float32)      # noqa: E731
    h0, hT = np.zeros(S, np.float32), np.zeros(S, np.float32)
    h0[0], hT[S - 1] = 1.0, 1.0
    p = {'Vgen': f(V, R), 'S1': f(S, R), 'S2': f(S, R), 'C_embed': f(K, R), 'C_wildcard': f(K, Q), 'S1_wildcard': f(S, Q),
         'S2_wildcard': f(S, Q), 'wildcard_wildcard': f(S, S), 'h0': h0, 'hT': hT}
    p['C_embed'][:, 0] += np.arange(1, K + 1, dtype=np.float32)      # the label columns apart: the decode has no tie
    x = rng.randint(0, V, size=(B, L)).astype(np.int64)
    ln = np.array([4, 2, 3], np.int64)
    lab = rng.randint(0, K, size=(B, L)).astype(np.int64)
    # every factor feeds the chains, whose candidates must stay small integers; a priority layer of a power of two times the
    # identity brings the largest score into [4, 8)
    with torch.no_grad():
        top = float(d0m.forward(d0m._params(p, torch.float64), None, x, ln, nl='relu')[0].abs().max())
    P = np.eye(K, dtype=np.float32) * np.float32(2.0 ** (2 - np.floor(np.log2(top))))
    kw = dict(p=p, P=P, x=x, lengths=ln, nl='relu', farnn=farnn, k=5.0, trans=None)
    out = dict(kw, labels=lab, present=cases.present_words(x, ln, V))
    out['l32'], out['g32'], _ = d0m.step(dtype=torch.float32, labels=lab, **kw)
    out['l64'], out['g64'], out['pred'] = d0m.step(dtype=torch.float64, labels=lab, **kw)
    out['last'] = d0m.step(dtype=torch.float64, labels=lab, fault='last', **kw)[1]
    return out


def test_exact_ties_go_to_the_first_index():
    case = tie_case()
    tops = []
    with torch.no_grad():
        d0m.forward(d0m._params(case['p'], torch.float64), d0m._t(case['P'], torch.float64), case['x'], case['lengths'], nl='relu', tops=tops)
    t = torch.stack(tops)
    assert int(((t[:, :, 0] == t[:, :, 1]) & (t[:, :, 0] != 0)).sum()) > 10          # non-zero maxima that tie exactly
    # the last maximal index gives other gradients: the case tells the two apart
    assert any(np.abs(case['last'][n] - case['g64'][n]).max() > 1e-3 * np.abs(case['g64'][n]).max() for n in case['g64'])
    d0m.check_gap(**{q: case[q] for q in ('p', 'P', 'x', 'lengths', 'nl', 'farnn', 'k', 'trans')})
    check_case('d0max-ties', case)


# ---- repeats -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['repeat', 'repeat-gated', 'repeat-crf'])
def test_two_max_steps_are_bit_identical(name):
    case = cases.get_case(name)[0]
    a = check_case('d0max-' + name, case)
    same_bytes(a, run_max(case))
    tc = context(case)
    try:
        same_bytes(a, run_max(case, tc))
        same_bytes(a, run_max(case, tc))
    finally:
        tc.close()


@pytest.mark.parametrize('name', ['repeat', 'repeat-gated', 'repeat-crf'])
def test_sum_max_sum_on_one_context_equals_a_fresh_sum_context(name):
    case = cases.get_case(name)[0]
    fresh = sum_gpu.run_lib(case)
    tc = context(case, 'sum')
    try:
        first = sum_gpu.run_lib(case, tc=tc)
        tc.set_semiring('max')
        mx = sum_gpu.run_lib(case, tc=tc)
        tc.set_semiring('sum')
        again = sum_gpu.run_lib(case, tc=tc)
    finally:
        tc.close()
    same_bytes(fresh, first)
    same_bytes(fresh, again)
    same_bytes(mx, run_max(case))
    assert any(mx[1][n].tobytes() != fresh[1][n].tobytes() for n in fresh[1])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
REFUSED = {'lds': dict(S=192, R=512, Q=512),                 # the score head's tile: 16 (2 S + 3 R + 3 Q + 2 K) floats above 160 KiB
           'q30': dict(Q=512, B=32768, L=63),                # B (L + 1) Q = 2^30
           'crf': dict(K=150, L=64)}


@pytest.mark.parametrize('dim', sorted(REFUSED))
def test_plan_stage_refusals_leave_the_outputs_untouched(dim):
    from re2nn_seq_amd import _lib
    kw = dict(dict(V=3, S=4, R=3, Q=2, K=3, B=2, L=3), **REFUSED[dim])
    V, S, R, Q, K, B, L = (kw[n] for n in 'VSRQKBL')
    dev = torch.device('cuda', 0)
    shapes = dict(Vgen=(V, R), S1=(S, R), S2=(S, R), Ce=(K, R), Cw=(K, Q), S1w=(S, Q), S2w=(S, Q), WW=(S, S), h0=(S,), hT=(S,))
    w = {n: torch.zeros(s, device=dev) for n, s in shapes.items()}
    g = {'d' + n: torch.full(s, GUARD, device=dev) for n, s in shapes.items()}
    if dim == 'crf':
        w['crf_trans'] = torch.from_numpy(cases.default_trans(K, np.random.RandomState(5))).to(dev)
        g['dtrans'] = torch.full((K, K), GUARD, device=dev)
    g['loss'] = torch.full((1,), GUARD, device=dev)
    g['tags'] = torch.full((B, L), -7, dtype=torch.int32, device=dev)
    x = torch.zeros((B, L), dtype=torch.int64, device=dev)
    ln = torch.full((B,), L, dtype=torch.int64, device=dev)
    tc = _lib.DecompFstTrainContext(V, S, R, Q, K, nl='tanh', use_crf=dim == 'crf', semiring='max')
    try:
        with pytest.raises(_lib.FarnnError, match='code {}'.format(ERANGE)):
            tc.step({n: t.data_ptr() for n, t in w.items()}, x.data_ptr(), ln.data_ptr(), x.data_ptr(), B, L, B * L,
                    {n: t.data_ptr() for n, t in g.items()}, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
    finally:
        tc.close()
    for n, t in g.items():
        assert bool((t == (-7 if n == 'tags' else GUARD)).all()), n


# ---- the model mirror against the captures of the reference (tests/golden/decomp0_train_max_small) -----------------------------------
def mirror(k):
    from re2nn_seq_amd.farnn.model_decompose import FARNN_S_D_W
    from test_decomp0_max_train_cpu import case
    from test_decomp0_train_cpu import FLAGS
    from util import ns
    cfg, inp, ref = case(k)
    p = inp['p']
    a = ns(independent=0, threshold=inp['threshold'], bias_init=0.1, **dict(FLAGS, **cfg))
    assert a.train_mode == 'max'
    a.additional_states, a.rand_constant = 0, 0.0            # the captured tensors are already padded
    C = p['C_embed'].shape[0] - 2 * cfg['use_crf']
    m = FARNN_S_D_W(V=p['V_embed'], C=p['C_embed'][:C], S1=p['S1'], S2=p['S2'], C_wildcard=p['C_wildcard'][:C],
                    S1_wildcard=p['S1_wildcard'], S2_wildcard=p['S2_wildcard'], wildcard_wildcard=p['wildcard_wildcard'],
                    final_vector=p['hT'], start_vector=p['h0'], pretrained_word_embed=p['embedding.weight'], priority_mat=None,
                    args=a, o_idx=inp['o_idx'])
    sd = {n: torch.from_numpy(v) for n, v in p.items()}
    if inp['trans'] is not None:
        sd[d0m.TRANS] = torch.from_numpy(inp['trans'])
    m.load_state_dict(sd)
    if inp['P'] is not None:
        m.priority_full = inp['P']
    return m, inp, ref


def both_switches(monkeypatch):
    monkeypatch.setenv('RE2NN_DECOMP_FST_TRAIN', '1')
    monkeypatch.setenv('RE2NN_DECOMP_FST_MAX_TRAIN', '1')


@pytest.mark.parametrize('k', range(13))
def test_the_model_mirror_matches_the_reference_capture(monkeypatch, k):
    """forward_local(train=True) + loss.backward() against capture k: the loss, every named parameter's gradient, the flat
    predictions; after eval() the max-semiring tagging handle tags as a freshly built model does from the trained state_dict()"""
    from test_decomp0_max_train_cpu import present_of
    from test_decomp0_train_cpu import check_all_grads
    both_switches(monkeypatch)
    m, inp, ref = mirror(k)
    l64, g64, _ = d0m.step(dtype=torch.float64, **inp)
    l32, g32, _ = d0m.step(dtype=torch.float32, **inp)
    loss, grads, pred = sum_gpu.mirror_step(m, inp)
    assert m._tc.semiring == 'max'
    assert set(grads) == set(ref['grads'])
    assert_float_path(loss, l32, l64, err_msg='loss')
    assert_float_path(loss, ref['loss'], l64, err_msg='loss against the capture')
    present = present_of(inp, ref)
    check_all_grads('d0max-mirror-c{}'.format(k), grads, g32, g64, present)
    check_all_grads('d0max-mirror-capture-c{}'.format(k), grads, ref['grads'], g64, present)
    assert np.array_equal(pred, ref['flat_pred'])
    m.eval()
    fresh = mirror(k)[0].load_state_dict(m.state_dict())
    xs, lns = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths'])
    got, want = m.forward_local(xs, xs, lns, train=False)[1], fresh.forward_local(xs, xs, lns, train=False)[1]
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())


class _Log:
    def __init__(self):
        self.lines = []

    def add(self, line):
        self.lines.append(line)

    def update_and_record(self, *a):
        pass


def test_three_adam_steps_through_train_epochs_lower_the_loss(monkeypatch):
    """three epochs of one batch through train_onehot.train_epochs (Adam) on the gated model of capture 8: the training loss falls,
    and the trained model's max-semiring tagging handle tags as the step itself does on the same weights"""
    from re2nn_seq_amd import train_onehot
    from util import ns
    both_switches(monkeypatch)
    monkeypatch.delenv('RE2NN_NATIVE_OPTIM', raising=False)
    monkeypatch.delenv('RE2NN_DEVICE_METRICS', raising=False)
    m, inp, _ = mirror(8)
    data = [{'x': inp['x'][b], 's': inp['labels'][b], 'l': inp['lengths'][b]} for b in range(inp['x'].shape[0])]
    i2s = {0: 'o', 1: 'B-a', 2: 'I-a', 3: 'B-b', 4: 'I-b'}
    args = ns(epoch=3, bz=len(data), optimizer='ADAM', lr=0.01, method='decompose', marryup_type='none')
    log = _Log()
    train_onehot.train_epochs(m, {'train': data, 'dev': data, 'test': data}, args, {'o': 0}, i2s, log, log, {})
    losses = [float(line.rsplit(' ', 1)[1]) for line in log.lines if line.startswith('TRAIN Epoch')]
    assert len(losses) == 3 and losses[2] < losses[1] < losses[0], losses
    xs, lab, lns = (torch.from_numpy(inp[q]) for q in ('x', 'labels', 'lengths'))
    m.train()
    step_tags = m.forward_local(xs, lab, lns, train=True)[1].cpu().numpy()
    m.eval()
    assert m._semiring() == 'max'
    assert np.array_equal(m.forward_local(xs, lab, lns, train=False)[1].cpu().numpy(), step_tags)
