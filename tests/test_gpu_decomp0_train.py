"""GPU checks of the decomposed FST's training step (FARNN_S_D_W): the C-ABI against the float64 / float32
restatement (tests/decomp0_train_ref.py) on drawn signed cases at the shape edges of the score head's tiles (16 positions, 16
columns per MFMA block, 4 k per MFMA) and of the chains, bit-identical repeats, the plan-stage refusals, and the decomposed
i-FST's own step before and after one of these."""
import numpy as np
import pytest
import torch

import decomp0_train_ref as d0r
from util import assert_float_path, check_grad, present_words

pytestmark = pytest.mark.gpu

LIB_NAMES = {'Vgen': 'Vgen', 'C_embed': 'Ce', 'S1': 'S1', 'S2': 'S2', 'C_wildcard': 'Cw', 'S1_wildcard': 'S1w', 'S2_wildcard': 'S2w',
             'wildcard_wildcard': 'WW', 'h0': 'h0', 'hT': 'hT', 'Wss1': 'Wss1', 'Wrs1': 'Wrs1', 'bs1': 'bs1', 'Wss2': 'Wss2',
             'Wrs2': 'Wrs2', 'bs2': 'bs2'}
GUARD = 12345.0


def default_trans(K, rng):
    tr = rng.uniform(-0.5, 0.5, size=(K, K)).astype(np.float32)
    tr[:, K - 2] = -10000.0
    tr[K - 1, :] = -10000.0
    return tr


def make_case(seed, V=12, S=7, R=6, Q=4, K=5, B=4, L=6, nl='tanh', farnn=0, crf=False, priority=False, lengths=None, x=None):
    """a drawn signed case, redrawn until the gap rule holds and every gradient is live and well conditioned in float32"""
    for draw in range(60):
        rng = np.random.RandomState(1000 * seed + draw)
        p = d0r.signed_base(V, S, R, Q, K, rng, farnn=farnn)
        xs = rng.randint(0, V, size=(B, L)).astype(np.int64) if x is None else np.asarray(x, np.int64)
        ln = np.asarray(lengths if lengths is not None else [L, 1] + list(rng.randint(1, L + 1, size=max(0, B - 2))), np.int64)[:B]
        lab = rng.randint(0, K - (2 if crf else 0), size=(B, L)).astype(np.int64)
        P = None
        if priority:
            P = (np.eye(K) + rng.choice([0.0, 0.25, -0.25], size=(K, K), p=[0.7, 0.15, 0.15])).astype(np.float32)
        kw = dict(p=p, P=P, x=xs, lengths=ln, nl=nl, farnn=farnn, k=5.0, trans=default_trans(K, rng) if crf else None)
        # a power of two (exact) on the label factors brings the largest score into [4, 8): many columns then lie well apart
        with torch.no_grad():
            top = float(d0r.forward(d0r._params(p, torch.float64), None if P is None else d0r._t(P, torch.float64), xs, ln, nl=nl,
                                    farnn=farnn, k=5.0)[0].abs().max())
        if top > 0:
            for n in ('C_embed', 'C_wildcard'):
                p[n] = p[n] * np.float32(2.0 ** (2 - np.floor(np.log2(top))))
        try:
            d0r.check_gap(**kw)
        except d0r.GapError:
            continue
        l32, g32, pr32 = d0r.step(dtype=torch.float32, labels=lab, **kw)
        l64, g64, pr64 = d0r.step(dtype=torch.float64, labels=lab, **kw)
        present = present_words(xs, ln, V)
        if d0r.badly_drawn(g32, g64, present) or not np.array_equal(pr32, pr64):
            continue
        return dict(kw, labels=lab, l32=l32, l64=l64, g32=g32, g64=g64, pred=pr64, present=present)
    raise AssertionError('no well-drawn case in 60 draws')


def run_lib(case, tc=None, guard=None):
    """one library step; returns (loss, {restatement name: gradient}, tags [B, L]) as numpy"""
    from re2nn_seq_amd import _lib
    dev = torch.device('cuda', 0)
    p, x = case['p'], case['x']
    V, R = p['Vgen'].shape
    S, Q = p['S1_wildcard'].shape
    K = p['C_embed'].shape[0]
    own = tc is None
    if own:
        tc = _lib.DecompFstTrainContext(V, S, R, Q, K, nl=case['nl'], threshold=0.5, o_idx=0, device=0,
                                        use_crf=case['trans'] is not None, farnn=case['farnn'], sigmoid_exponent=case['k'])
    t = {n: torch.from_numpy(a).to(dev).contiguous() for n, a in p.items()}
    fill = float('nan') if guard is None else guard
    g = {n: torch.full_like(a, fill) for n, a in t.items()}
    weights = {LIB_NAMES[n]: a.data_ptr() for n, a in t.items()}
    outputs = {'d' + LIB_NAMES[n]: a.data_ptr() for n, a in g.items()}
    keep = []
    if case['P'] is not None:
        keep.append(torch.from_numpy(case['P']).to(dev))
        weights['P'] = keep[-1].data_ptr()
    if case['trans'] is not None:
        keep.append(torch.from_numpy(case['trans']).to(dev))
        weights['crf_trans'] = keep[-1].data_ptr()
        g[d0r.TRANS] = torch.full_like(keep[-1], fill)
        outputs['dtrans'] = g[d0r.TRANS].data_ptr()
    B, L = x.shape
    xd, ld, lab = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, case['lengths'], case['labels']))
    loss = torch.full((1,), fill, dtype=torch.float32, device=dev)
    tags = torch.full((B, L), -7, dtype=torch.int32, device=dev)
    outputs['loss'], outputs['tags'] = loss.data_ptr(), tags.data_ptr()
    ntok = int(np.clip(case['lengths'], 0, L).sum())
    try:
        tc.step(weights, xd.data_ptr(), ld.data_ptr(), lab.data_ptr(), B, L, ntok, outputs, torch.cuda.current_stream(dev).cuda_stream)
    finally:
        torch.cuda.synchronize(dev)
        if own:
            tc.close()
    return float(loss.cpu()), {n: a.cpu().numpy() for n, a in g.items()}, tags.cpu().numpy()


def check_case(name, case):
    loss, grads, tags = run_lib(case)
    assert_float_path(loss, case['l32'], case['l64'], err_msg=name + ' loss')
    assert set(grads) == set(case['g64'])
    for n in sorted(case['g64']):
        word = n == 'Vgen'
        check_grad(name, n, grads[n].reshape(case['g64'][n].shape), case['g32'][n], case['g64'][n], slices=0 if word else None,
                   present=case['present'] if word else None)
    L = case['x'].shape[1]
    mask = np.arange(L)[None, :] < np.clip(case['lengths'], 0, L)[:, None]
    assert np.array_equal(tags[mask].astype(np.int64), case['pred'])
    assert (tags[~mask] == -1).all()
    return loss, grads, tags


# the edges: S below / at / above one 64-wide chain block; R and Q around the 16-column MFMA block and the 4-wide k step; K
# around 16 and 64; positions below / at / above the 16-position tile (B x L = 3, 16, 18, 72)
SHAPES = [dict(S=1, R=1, Q=3, K=2, B=1, L=3, lengths=[3]),
          dict(S=3, R=5, Q=1, K=9, B=4, L=4, lengths=[4, 1, 3, 2]),
          dict(S=64, R=64, Q=20, K=64, B=2, L=8, lengths=[8, 1]),
          dict(S=65, R=65, Q=67, K=65, B=8, L=9, lengths=[9, 1, 0, 5, 9, 2, 7, 3]),
          dict(S=7, R=130, Q=20, K=5, B=9, L=2, lengths=[2, 1, 2, 2, 1, 2, 2, 2, 2]),
          dict(S=9, R=16, Q=17, K=16, B=3, L=6, lengths=[6, 5, 1])]


@pytest.mark.parametrize('k', range(len(SHAPES)))
def test_step_matches_the_restatement_at_the_shape_edges(k):
    check_case('d0-shape{}'.format(k), make_case(10 + k, V=12, nl='tanh', **SHAPES[k]))


@pytest.mark.parametrize('nl', ['none', 'relu', 'relutanh'])
def test_every_update_nonlinear(nl):
    check_case('d0-' + nl, make_case(31, nl=nl))


@pytest.mark.parametrize('farnn', [1, 2])
def test_the_gated_recurrences(farnn):
    check_case('d0-farnn{}'.format(farnn), make_case(40 + farnn, farnn=farnn, S=9, R=6, Q=4))


@pytest.mark.parametrize('K,priority,farnn', [(4, False, 0), (9, True, 0), (7, False, 2)])
def test_the_crf_loss(K, priority, farnn):
    check_case('d0-crf-K{}'.format(K), make_case(50 + K, K=K, crf=True, priority=priority, farnn=farnn))


def test_the_priority_layer():
    check_case('d0-priority', make_case(61, priority=True))


def test_one_word_fills_the_batch_and_one_word_per_position():
    check_case('d0-oneword', make_case(71, V=5, B=4, L=6, lengths=[6, 6, 6, 6], x=np.full((4, 6), 3)))
    check_case('d0-distinct', make_case(72, V=30, B=4, L=6, lengths=[6, 6, 6, 6], x=np.arange(24).reshape(4, 6)))


@pytest.mark.parametrize('kw', [dict(), dict(farnn=2), dict(crf=True, K=6, priority=True)])
def test_two_steps_are_bit_identical(kw):
    case = make_case(81, B=8, L=9, S=9, lengths=[9, 1, 4, 9, 2, 7, 3, 5], **kw)
    a, b = run_lib(case), run_lib(case)
    assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes()
    for n in a[1]:
        assert a[1][n].tobytes() == b[1][n].tobytes(), n
    assert np.array_equal(a[2], b[2])


REFUSED = {'S': dict(S=513), 'R': dict(R=513), 'Q': dict(Q=513), 'crf': dict(K=150, L=64),
           'lds': dict(S=512, R=512, Q=512),                  # the score head's tile: 16 (2 S + 3 R + 3 Q + 2 K) floats above 160 KiB
           'q30': dict(Q=512, B=32768, L=63)}                 # B (L + 1) Q = 2^30


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
        w['crf_trans'] = torch.from_numpy(default_trans(K, np.random.RandomState(5))).to(dev)
        g['dtrans'] = torch.full((K, K), GUARD, device=dev)
    g['loss'] = torch.full((1,), GUARD, device=dev)
    g['tags'] = torch.full((B, L), -7, dtype=torch.int32, device=dev)
    x = torch.zeros((B, L), dtype=torch.int64, device=dev)
    ln = torch.full((B,), L, dtype=torch.int64, device=dev)
    tc = _lib.DecompFstTrainContext(V, S, R, Q, K, nl='tanh', use_crf=dim == 'crf')
    try:
        with pytest.raises(_lib.FarnnError):
            tc.step({n: t.data_ptr() for n, t in w.items()}, x.data_ptr(), ln.data_ptr(), x.data_ptr(), B, L, B * L,
                    {n: t.data_ptr() for n, t in g.items()}, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
    finally:
        tc.close()
    for n, t in g.items():
        assert bool((t == (-7 if n == 'tags' else GUARD)).all()), n


def _ifst_step(w, x, ln, lab, K):
    """one plain decomposed i-FST step on a context of its own: (loss, gradients, tags)"""
    from re2nn_seq_amd import _lib
    dev = torch.device('cuda', 0)
    B, L = x.shape
    V, R = w['Vgen'].shape
    tc = _lib.TrainContext(V, w['S1'].shape[0], R, K, nl='tanh')
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


def test_the_ifst_step_is_not_disturbed():
    """A plain decomposed i-FST step on its own context before and after a decomposed FST step in the same process.  That step
    adds with float atomics, so its bits are its own from run to run only where every sum has at most two
    addends: one sequence of two distinct words (two chain steps; each word's row, dOsum, the loss and every product get two
    addends).  There the bits are equal; on a ragged 4 x 6 batch the tags are equal and the sums agree to the atomics' order."""
    rng = np.random.RandomState(3)
    V, S, R, K, B, L = 12, 9, 6, 5, 4, 6
    base = d0r.signed_base(V, S, R, 4, K, rng)
    w = {'Vgen': base['Vgen'], 'S1': base['S1'], 'S2': base['S2'], 'W': base['wildcard_wildcard'],
         'C': np.abs(rng.choice([0.5, 1.0], size=(K, S))).astype(np.float32), 'h0': base['h0'], 'hT': base['hT']}
    x = rng.randint(0, V, size=(B, L)).astype(np.int64)
    ln = np.array([6, 1, 4, 3], np.int64)
    lab = rng.randint(0, K, size=(B, L)).astype(np.int64)
    two = (np.array([[3, 7]], np.int64), np.array([2], np.int64), lab[:1, :2].copy())
    two_before, before = _ifst_step(w, *two, K), _ifst_step(w, x, ln, lab, K)
    run_lib(make_case(91))
    two_after, after = _ifst_step(w, *two, K), _ifst_step(w, x, ln, lab, K)
    assert np.float32(two_before[0]).tobytes() == np.float32(two_after[0]).tobytes() and np.array_equal(two_before[2], two_after[2])
    for n in two_before[1]:
        assert np.abs(two_before[1][n]).max() > 0 and two_before[1][n].tobytes() == two_after[1][n].tobytes(), n
    assert np.array_equal(before[2], after[2])
    assert abs(before[0] - after[0]) <= 1e-6 * (1 + abs(before[0]))
    for n in before[1]:
        np.testing.assert_allclose(after[1][n], before[1][n], rtol=1e-5, atol=1e-6 * np.abs(before[1][n]).max(), err_msg=n)


def test_an_odd_batch_leaves_no_share_of_a_missing_sequence():
    """B = 3 and B = 5: the last workgroup of either chain holds one sequence and an empty slot (two sequences per workgroup),
    and with four per workgroup three empty ones.  A missed or stray row of DVf / DVb / HP would show in dVgen, dh0 or dhT."""
    for B in (3, 5):
        check_case('d0-odd{}'.format(B), make_case(95 + B, B=B, L=4, S=9, farnn=2, lengths=[4, 1, 3, 2, 4][:B]))


# ---- the model mirror against the captures of the reference (tests/golden/decomp0_train_small) ---------------------------------
def mirror(k, **flags):
    """FARNN_S_D_W built from captured configuration k's parameters (every train_* flag on unless `flags` says otherwise)"""
    from re2nn_seq_amd.farnn.model_decompose import FARNN_S_D_W
    from test_decomp0_train_cpu import FLAGS, case
    from util import ns
    cfg, inp, ref = case(k)
    p = inp['p']
    a = ns(independent=0, threshold=inp['threshold'], bias_init=0.1, **dict(FLAGS, **dict(cfg, **flags)))
    a.additional_states, a.rand_constant = 0, 0.0            # the captured tensors are already padded
    C = p['C_embed'].shape[0] - 2 * cfg['use_crf']
    m = FARNN_S_D_W(V=p['V_embed'], C=p['C_embed'][:C], S1=p['S1'], S2=p['S2'], C_wildcard=p['C_wildcard'][:C],
                    S1_wildcard=p['S1_wildcard'], S2_wildcard=p['S2_wildcard'], wildcard_wildcard=p['wildcard_wildcard'],
                    final_vector=p['hT'], start_vector=p['h0'], pretrained_word_embed=p['embedding.weight'], priority_mat=None,
                    args=a, o_idx=inp['o_idx'])
    sd = {n: torch.from_numpy(v) for n, v in p.items()}
    if inp['trans'] is not None:
        sd[d0r.TRANS] = torch.from_numpy(inp['trans'])
    m.load_state_dict(sd)
    if inp['P'] is not None:
        m.priority_full = inp['P']
    return m, inp, ref


def mirror_step(m, inp):
    loss, pred, _ = m.forward_local(torch.from_numpy(inp['x']), torch.from_numpy(inp['labels']), torch.from_numpy(inp['lengths']),
                                    train=True)
    loss.backward()
    return float(loss.detach()), {n: t.grad.cpu().numpy().copy() for n, t in m.named_parameters()}, pred.cpu().numpy()


@pytest.mark.parametrize('k', range(13))
def test_the_model_mirror_matches_the_reference_capture(monkeypatch, k):
    """forward_local(train=True) + loss.backward() against capture k: the loss, every named parameter's gradient, the flat
    predictions; after eval() the tagging handle tags as a freshly built model does from the trained state_dict()"""
    from test_decomp0_train_cpu import check_all_grads
    monkeypatch.setenv('RE2NN_DECOMP_FST_TRAIN', '1')
    m, inp, ref = mirror(k)
    kw = {q: v for q, v in inp.items()}
    l64, g64, _ = d0r.step(dtype=torch.float64, **kw)
    l32, g32, _ = d0r.step(dtype=torch.float32, **kw)
    loss, grads, pred = mirror_step(m, inp)
    assert set(grads) == set(ref['grads'])
    assert_float_path(loss, l32, l64, err_msg='loss')
    assert_float_path(loss, ref['loss'], l64, err_msg='loss against the capture')
    present = np.zeros(inp['p']['V_embed'].shape[0], bool)
    present[ref['words']] = True
    check_all_grads('d0-mirror-c{}'.format(k), grads, g32, g64, present)
    check_all_grads('d0-mirror-capture-c{}'.format(k), grads, ref['grads'], g64, present)
    assert np.array_equal(pred, ref['flat_pred'])
    m.eval()
    fresh = mirror(k)[0].load_state_dict(m.state_dict())
    xs, lns = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths'])
    got, want = m.forward_local(xs, xs, lns, train=False)[1], fresh.forward_local(xs, xs, lns, train=False)[1]
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())


@pytest.mark.parametrize('k', [1, 10])
@pytest.mark.parametrize('off,gone', [(dict(train_wildcard=0), {'C_wildcard', 'S1_wildcard', 'S2_wildcard'}),
                                      (dict(train_wildcard_wildcard=0, train_h0=0, train_hT=0), {'wildcard_wildcard', 'h0', 'hT'}),
                                      (dict(train_V_embed=0, train_beta=0, train_word_embed=0), {'V_embed', 'beta_vec', 'embedding.weight'})])
def test_named_parameters_follow_the_train_flags(monkeypatch, k, off, gone):
    """a flag switched off takes its tensors out of named_parameters() and leaves every other gradient as it was, bit for bit"""
    monkeypatch.setenv('RE2NN_DECOMP_FST_TRAIN', '1')
    m, inp, _ = mirror(k)
    full = mirror_step(m, inp)[1]
    m2, _, _ = mirror(k, **off)
    part = mirror_step(m2, inp)[1]
    assert set(part) == set(full) - gone
    for n in part:
        assert part[n].tobytes() == full[n].tobytes(), n


@pytest.mark.parametrize('native', [False, True])
def test_three_adam_steps_match_the_restatement(monkeypatch, native):
    """three Adam steps as train_onehot.train_epochs makes them (torch.optim, or the library's one-launch optimizer) on the
    gated model of capture 8 (update_nonlinear none: no kink to cross): every parameter against the restatement's trajectory"""
    monkeypatch.setenv('RE2NN_DECOMP_FST_TRAIN', '1')
    m, inp, _ = mirror(8)
    p0 = {n: v.copy() for n, v in inp['p'].items()}
    rng = np.random.RandomState(77)
    V, K = p0['V_embed'].shape[0], p0['C_embed'].shape[0]
    batches = [(rng.randint(0, V, size=(4, 5)).astype(np.int64), np.array([5, 1, 3, 4], np.int64),
                rng.randint(0, K, size=(4, 5)).astype(np.int64)) for _ in range(3)]
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
    m.eval()
    sd = m.state_dict()
    kw = dict(P=None, batches=batches, nl='none', farnn=2, k=5.0, lr=0.01)
    p32, p64 = d0r.adam_steps(p0, dtype=torch.float32, **kw), d0r.adam_steps(p0, dtype=torch.float64, **kw)
    for n in p0:
        got = sd[n].numpy().reshape(p0[n].shape)
        assert_float_path(got, p32[n], p64[n], err_msg=n + ' after 3 Adam steps')
        assert np.abs(got - p0[n]).max() > 0, n
