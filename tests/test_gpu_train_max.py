"""The max-semiring training step of the decomposed i-FST (--train_mode max) on the GPU: against the
reference's captures through the model mirror, against the float64 restatement (tests/decomp_max_train_ref.py) through the
C-ABI, tie handling, switching semirings on one context, training progress and the command line.

Large shapes: rounding must never decide a maximum, so the float64 restatement asserts a minimum relative gap of 2e-5 for
every non-zero maximum and the weights are drawn again (next seed) until it holds; exact-zero ties stay in."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import decomp_max_train_ref as dmr  # noqa: E402
from util import GOLDEN, assert_float_path, check_grad, ns, present_words  # noqa: E402

pytestmark = pytest.mark.gpu

PARAMS = ('S1', 'S2', 'V_embed', 'embed_r_generalized', 'C_output_mat', 'wildcard_mat', 'h0', 'hT', 'beta_vec',
          'embedding.weight')
GATES = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')
MIN_GAP = 2e-5


def load():
    with open(os.path.join(GOLDEN, 'decomp_train_max_small.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, 'decomp_train_max_small.npz')), np.load(os.path.join(GOLDEN, 'decomp_small.npz'))


def close(got, ref, name, rtol=2e-3, atol=2e-6, frac=2e-4):
    scale = max(float(np.abs(ref).max()), 1e-6)
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol + frac * scale, err_msg=name)


def mirror(k):
    from re2nn_seq_amd.farnn.model_decompose_single import FARNN_S_D_W_I_S
    meta, g, base = load()
    cfg = {kk: v for kk, v in meta['configs'][k].items() if kk != 'seed'}
    a = ns(**dict(meta['train_flags'], **cfg))
    torch.manual_seed(0)
    m = FARNN_S_D_W_I_S(V=base['V_in'], S1=base['S1_in'], S2=base['S2_in'], C_output_mat=base['O_in'],
                        wildcard_mat=base['W_in'], wildcard_output_vector=base['Ow_in'], final_vector=base['final_in'],
                        start_vector=base['start_in'], pretrained_word_embed=base['E_in'], priority_mat=base['priority_in'],
                        args=a, o_idx=meta['o_idx'])
    pre = 'c{}.'.format(k)
    sd = {n: g[pre + 'w.' + n] for n in PARAMS}
    sd['priority_layer.priority_mat'] = g[pre + 'w.priority_mat']
    names = PARAMS
    if cfg.get('use_crf'):
        sd['crf.transitions'] = g[pre + 'w.crf.transitions']
        names = PARAMS + ('crf.transitions',)
    for n in GATES:
        if pre + 'w.' + n in g.files:
            sd[n] = g[pre + 'w.' + n]
            names = names + (n,)
    m.load_state_dict(sd)
    return m, names, g, base, pre


@pytest.mark.parametrize('k', range(10))
def test_train_step_matches_reference_captures(k):
    """forward_local(train=True) -> loss.backward() -> .grad of every parameter and the flat predictions, against the
    reference's own max-semiring step; the step's tags equal forward_local(train=False) on the same weights."""
    m, names, g, base, pre = mirror(k)
    x, lengths, labels = torch.from_numpy(base['x']), torch.from_numpy(base['lengths']), torch.from_numpy(g['labels'])
    m.train()
    loss, pred, _ = m.forward_local(x, labels, lengths, train=True)
    loss.backward()
    ref_loss = float(g[pre + 'loss'])
    assert abs(float(loss.detach()) - ref_loss) < 2e-5 * max(1.0, abs(ref_loss))
    assert np.array_equal(pred.cpu().numpy(), g[pre + 'flat_pred'])
    named = dict(m.named_parameters())
    assert set(named) == set(names)
    for n in names:
        close(named[n].grad.cpu().numpy(), g[pre + 'g.' + n], n)
    m.eval()
    _, pred_eval, _ = m.forward_local(x, labels, lengths, train=False)
    assert np.array_equal(pred.cpu().numpy(), pred_eval.cpu().numpy())


def draw(S, R, K, V, B, L, nl, farnn, crf, prio, seed, onehot_h=False):
    rng = np.random.RandomState(seed)
    f = lambda *shape, sc=0.3: (rng.randn(*shape) * sc).astype(np.float32)   # noqa: E731
    Cm = np.zeros((K, S), np.float32)
    Cm[rng.randint(0, K - (2 if crf else 0), size=S), np.arange(S)] = 1.0
    w = {'Vgen': f(V, R, sc=0.8), 'S1': f(S, R, sc=1.0 / np.sqrt(S)), 'S2': f(S, R, sc=1.0 / np.sqrt(S)),
         'W': ((rng.rand(S, S) < 2.0 / S) * 0.5 + f(S, S, sc=0.02)).astype(np.float32),
         'C': (Cm + rng.rand(K, S).astype(np.float32) * 0.02).astype(np.float32),
         'h0': f(S, sc=0.5), 'hT': f(S, sc=0.5)}
    if onehot_h:
        w['h0'] = np.eye(S, dtype=np.float32)[0]
        w['hT'] = np.eye(S, dtype=np.float32)[S - 1]
    if prio:
        w['P'] = (np.eye(K) + (rng.rand(K, K) < 0.05) * 0.5).astype(np.float32)
    if crf:
        tr = f(K, K, sc=0.5)
        tr[:, K - 2] = -10000.0
        tr[K - 1, :] = -10000.0
        w['trans'] = tr
    if farnn >= 1:
        w.update(Wss1=f(S, S, sc=1.0 / np.sqrt(S)), Wrs1=f(R, S, sc=1.0 / np.sqrt(R)), bs1=f(S, sc=0.5))
    if farnn == 2:
        w.update(Wss2=f(S, S, sc=1.0 / np.sqrt(S)), Wrs2=f(R, S, sc=1.0 / np.sqrt(R)), bs2=f(S, sc=0.5))
    lengths = rng.randint(1, L + 1, size=B).astype(np.int64)
    lengths[0] = L
    if B > 3:
        lengths[1] = 0
    x = rng.randint(0, V, size=(B, L)).astype(np.int64)
    labels = rng.randint(0, K - (2 if crf else 0), size=(B, L)).astype(np.int64)
    return w, x, lengths, labels


def gapped_case(*args, seed0, **kw):
    """the first draw whose float64 restatement has no maximum decided by less than MIN_GAP relative"""
    S, R, K, V, B, L, nl, farnn, crf, prio = args
    for seed in range(seed0, seed0 + 40):
        w, x, lengths, labels = draw(*args, seed=seed, **kw)
        xt, lt = torch.from_numpy(x), torch.from_numpy(lengths)
        try:
            ref64 = dmr.step_on_table(w, xt, lt, labels, nl=nl, farnn=farnn, dtype=torch.float64, min_gap=MIN_GAP)
        except dmr.GapError:
            continue
        ref32 = dmr.step_on_table(w, xt, lt, labels, nl=nl, farnn=farnn, dtype=torch.float32)
        return w, x, lengths, labels, ref32, ref64
    pytest.fail('no draw without a near tie')


OUT_NAMES = ('Vgen', 'S1', 'S2', 'W', 'C', 'h0', 'hT')


def run_library(w, x, lengths, labels, nl, farnn, crf, semiring='max', tc=None, steps=1):
    from re2nn_seq_amd import _lib
    V, R = w['Vgen'].shape
    S, K = w['S1'].shape[0], w['C'].shape[0]
    B, L = x.shape
    dev = torch.device('cuda')
    if tc is None:
        tc = _lib.TrainContext(V, S, R, K, nl=nl, threshold=0.5, o_idx=1, use_crf=crf, farnn=farnn, semiring=semiring)
    wd = {n: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for n, v in w.items()}
    weights = {n: wd[n].data_ptr() for n in OUT_NAMES}
    weights['P'] = wd['P'].data_ptr() if 'P' in wd else None
    weights['crf_trans'] = wd['trans'].data_ptr() if 'trans' in wd else None
    out = {'d' + n: torch.full_like(wd[n], 7.0) for n in OUT_NAMES}          # the library must zero them itself
    for n in GATES[:3 * farnn]:
        weights[n] = wd[n].data_ptr()
        out['d' + n] = torch.full_like(wd[n], 7.0)
    if crf:
        out['dtrans'] = torch.full_like(wd['trans'], 7.0)
    loss = torch.full((1,), 3.0, device=dev)
    tags = torch.empty((B, L), dtype=torch.int32, device=dev)
    xd, ld, labd = (torch.from_numpy(a).to(dev) for a in (x, lengths, labels))
    for _ in range(steps):
        tc.step(weights, xd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, int(lengths.sum()),
                dict({n: t.data_ptr() for n, t in out.items()}, loss=loss.data_ptr(), tags=tags.data_ptr()))
    torch.cuda.synchronize()
    res = {n: t.cpu().numpy() for n, t in out.items()}
    res['loss'] = float(loss)
    res['tags'] = tags.cpu().numpy()
    return res, tc


def check_against(res, ref32, ref64, farnn, crf, tol=1e-4, x=None, lengths=None, case='max'):
    """the ONE rule and the gradient rule (each tensor at its own scale; with the batch, dVgen also row by row at each
    present word's scale and exactly zero at the absent ones)"""
    l32, g32, _ = ref32
    l64, g64, _ = ref64
    assert_float_path([res['loss']], [l32], [l64], tol, 'loss')
    names = list(OUT_NAMES) + list(GATES[:3 * farnn]) + (['trans'] if crf else [])
    for n in names:
        got = res['d' + n].reshape(g64[n].shape)
        assert_float_path(got, g32[n], g64[n], tol, 'd' + n)
        sliced = n == 'Vgen' and x is not None
        check_grad(case, 'd' + n, got, g32[n], g64[n], tol, slices=0 if sliced else None,
                   present=present_words(x, lengths, got.shape[0]) if sliced else None)


@pytest.mark.parametrize('S,R,K,V,B,L,nl,farnn,crf,prio', [
    (134, 250, 130, 60, 4, 8, 'tanh', 2, True, False),       # the shipped shape: 104 + 30 additional states, rank 250, CRF
    (134, 250, 20, 60, 4, 8, 'relu', 0, False, True),
    (104, 50, 73, 300, 6, 12, 'tanh', 1, False, False),
    (23, 70, 9, 50, 7, 9, 'relutanh', 2, False, True),       # rank above the state count
    (64, 64, 12, 40, 4, 16, 'none', 0, True, False),
    (7, 5, 3, 9, 1, 1, 'tanh', 0, False, False),             # one sequence of one token
    (5, 3, 4, 11, 3, 6, 'none', 1, False, False),
])
def test_c_abi_vs_float64_restatement(S, R, K, V, B, L, nl, farnn, crf, prio):
    """The C-ABI entry point with empty and full-length sequences, against the float64 restatement."""
    w, x, lengths, labels, ref32, ref64 = gapped_case(S, R, K, V, B, L, nl, farnn, crf, prio, seed0=S + R + farnn)
    res, tc = run_library(w, x, lengths, labels, nl, farnn, crf, steps=2)          # twice: the workspace is reused
    check_against(res, ref32, ref64, farnn, crf, x=x, lengths=lengths, case='max S{} R{} K{} farnn{} crf{}'.format(S, R, K, farnn, int(crf)))
    t = res['tags']
    mask = np.arange(L)[None, :] < lengths[:, None]
    assert (t[~mask] == -1).all()
    if not crf:
        sc = ref64[2].copy()
        sc[:, K - 1] = np.minimum(sc[:, K - 1], 0.5)
        want = sc.argmax(1)
        want[want == K - 1] = 1
        assert np.array_equal(t[mask], want)


def test_ties_with_a_onehot_start_and_relu():
    """h0 / hT one-hot and relu: most products of a step are exactly +-0, and torch.max's first index takes the adjoint"""
    S, R, K, V, B, L = 16, 8, 6, 12, 5, 7
    w, x, lengths, labels, ref32, ref64 = gapped_case(S, R, K, V, B, L, 'relu', 0, False, False, seed0=5, onehot_h=True)
    res, _ = run_library(w, x, lengths, labels, 'relu', 0, False)
    check_against(res, ref32, ref64, 0, False, x=x, lengths=lengths, case='max ties')


def test_steps_repeat_and_the_context_switches_back_to_sum():
    """Two max steps give the same tags; a context switched to max and back to sum matches a fresh sum context up to the
    summation order of the sum step's atomics (the bar of test_gpu_train_step.py)"""
    S, R, K, V, B, L = 40, 30, 10, 50, 6, 10
    w, x, lengths, labels = draw(S, R, K, V, B, L, 'tanh', 2, False, False, seed=11)
    a, tc = run_library(w, x, lengths, labels, 'tanh', 2, False)
    b, _ = run_library(w, x, lengths, labels, 'tanh', 2, False, tc=tc)
    assert np.array_equal(a['tags'], b['tags'])
    for n in a:
        if n != 'tags':
            assert np.all(np.isfinite(a[n])), n
    tc.set_semiring('sum')
    back, _ = run_library(w, x, lengths, labels, 'tanh', 2, False, tc=tc)
    fresh, _ = run_library(w, x, lengths, labels, 'tanh', 2, False, semiring='sum')
    assert np.array_equal(back['tags'], fresh['tags'])
    for n in fresh:
        if n == 'tags':
            continue
        ref = np.asarray(fresh[n], np.float64)
        assert float(np.abs(np.asarray(back[n]) - ref).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max())), n


def test_set_semiring_refuses_bad_values_and_too_many_states():
    from re2nn_seq_amd import _lib
    tc = _lib.TrainContext(10, 193, 8, 5)
    with pytest.raises(_lib.FarnnError):
        tc.set_semiring('max')
    tc.set_semiring('sum')
    raw = _lib.load().farnn_train_set_semiring(tc._raw, 7)
    assert raw != 0
    _lib.TrainContext(10, 134, 8, 5, semiring='max')


def test_adam_steps_lower_the_loss():
    from re2nn_seq_amd.farnn.train_step import decomp_ifst_train_step
    from re2nn_seq_amd import _lib
    S, R, K, V, B, L = 48, 40, 9, 80, 16, 12
    w, x, lengths, labels = draw(S, R, K, V, B, L, 'tanh', 1, False, False, seed=3)
    dev = torch.device('cuda')
    p = {n: torch.from_numpy(v).to(dev).requires_grad_(True) for n, v in w.items()}
    tc = _lib.TrainContext(V, S, R, K, nl='tanh', farnn=1, semiring='max')
    opt = torch.optim.Adam(list(p.values()), lr=3e-3)
    xd, ld, labd = (torch.from_numpy(a).to(dev) for a in (x, lengths, labels))
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss, _ = decomp_ifst_train_step(tc, p['Vgen'], p['S1'], p['S2'], p['W'], p['C'], p['h0'], p['hT'], None, xd, ld,
                                         labd, gates=(p['Wss1'], p['Wrs1'], p['bs1']), valid_tokens=int(lengths.sum()))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0] * 0.9, losses


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    from re2nn_seq_amd import synth
    root = str(tmp_path_factory.mktemp('data'))
    return synth.write_dataset_tree(root, dataset='ATIS-BIO', seed=4)


def test_decompose_cli_trains_max_for_two_epochs(tree, tmp_path):
    """--train_mode max --epoch 2 through the command line (the epoch loop needs nothing new)"""
    from re2nn_seq_amd import main as cli
    L = 12
    argv = ['--dataset', 'ATIS-BIO', '--method', 'decompose', '--independent', '2', '--train_mode', 'max',
            '--automata_path', tree['paths']['IIID'], '--rank', '100', '--seed', '1', '--beta', '0.9',
            '--embed_dim', '16', '--normalize_automata', 'none', '--rand_constant', '0',
            '--update_nonlinear', 'tanh', '--bz', '9', '--seq_max_len', str(L), '--epoch', '2', '--lr', '0.01',
            '--train_portion', '1.0', '--data_dir', tree['paths']['data_dir'], '--model_dir', str(tmp_path)]
    results, stats, res_path = cli.main(argv)
    steps = stats['train_step']
    assert len(steps) == 2 and all(s['tokens'] > 0 for s in steps)
    saved = cli.load_res(res_path)
    assert saved['args'].train_mode == 'max'
    losses = [float(line.split('LOSS:')[1]) for line in saved['logger'].record if 'LOSS:' in line]
    assert len(losses) == 2 and all(np.isfinite(losses))
