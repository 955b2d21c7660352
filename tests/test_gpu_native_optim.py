"""The library's optimizer step (farnn_optim_*, re2nn_seq_amd.farnn.optim) on the device: against the
float64 restatement (tests/native_optim_ref.py) and torch's own float32 optimizers at every size at which the kernel takes
another path, with guard elements around every tensor; skipped and zero gradients; bit reproducibility; the interchange of
state dicts with torch.optim.Adam; the refusals of the C-ABI; the onehot i-FST trained end to end; both CLI drivers.

Every case uses lr = 0.05: one Adam update moves a parameter by about 0.05, hundreds of times the 1e-4 of the rule."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import native_optim_ref as nor
import onehot_train_ref as otr
from util import assert_float_path, assert_grad_path, ns

pytestmark = pytest.mark.gpu

LR = 0.05
GUARD = 8                       # guard elements in front of and behind every tensor (a multiple of 4: they keep the alignment)
SENTINEL = 12345.678


def _chunk():
    from re2nn_seq_amd import _lib
    return _lib.OPTIM_CHUNK


def _edge_numels():
    c = _chunk()
    return [1, 3, 4, 5, c - 1, c, c + 1, 2 * c + 7]


class Guarded:
    """n tensors as views into ONE buffer, GUARD sentinel elements around each.  Tensor k starts on a 16-byte boundary, the
    ones listed in `misaligned` one float behind one."""

    def __init__(self, numels, misaligned=(), fill=None, dev='cuda'):
        self.offsets, off = [], 0
        for k, n in enumerate(numels):
            off += GUARD
            off = (off + 3) // 4 * 4 + (1 if k in misaligned else 0)
            self.offsets.append(off)
            off += n
        self.numels = list(numels)
        self.buf = torch.full((off + GUARD + 4,), SENTINEL, dtype=torch.float32, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.is_guard = torch.ones(self.buf.shape, dtype=torch.bool, device=dev)
        self.views = []
        for k, (o, n) in enumerate(zip(self.offsets, self.numels)):
            v = self.buf[o:o + n]
            assert (v.data_ptr() % 16 != 0) == (k in misaligned)
            v.copy_(torch.zeros(n) if fill is None else torch.from_numpy(fill[k]))
            self.is_guard[o:o + n] = False
            self.views.append(v)

    def assert_guards_untouched(self, what):
        g = self.buf[self.is_guard]
        assert bool((g == SENTINEL).all()), '{}: {} guard elements were overwritten'.format(what, int((g != SENTINEL).sum()))


def _draw(numels, steps, seed):
    rng = np.random.RandomState(seed)
    params = [rng.randn(n).astype(np.float32) for n in numels]
    grads = [[(rng.randn(n) * 10.0 ** rng.randint(-2, 2)).astype(np.float32) for n in numels] for _ in range(steps)]
    return params, grads


def _torch_run(kind, params, grads):
    """torch's own optimizer in float32 on the device: (params, exp_avg, exp_avg_sq) as numpy lists"""
    tp = [torch.from_numpy(p.copy()).cuda().requires_grad_(True) for p in params]
    opt = (torch.optim.Adam if kind == 'adam' else torch.optim.SGD)(tp, lr=LR, weight_decay=0)
    for gs in grads:
        for p, g in zip(tp, gs):
            p.grad = None if g is None else torch.from_numpy(g.copy()).cuda()
        opt.step()
    out = [p.detach().cpu().numpy() for p in tp]
    if kind == 'sgd':
        return out, None, None
    return out, [opt.state[p]['exp_avg'].cpu().numpy() for p in tp], [opt.state[p]['exp_avg_sq'].cpu().numpy() for p in tp]


def _native_run(kind, params, grads, misaligned=()):
    """the library's optimizer with params, grads and both moments as guarded views; returns the numpy results and the optimizer"""
    from re2nn_seq_amd.farnn import optim
    numels = [p.size for p in params]
    P, G = Guarded(numels, misaligned, fill=params), Guarded(numels, misaligned)
    M, V = Guarded(numels, misaligned), Guarded(numels, misaligned)
    tp = [v.detach().requires_grad_(True) for v in P.views]
    assert all(t.data_ptr() == v.data_ptr() for t, v in zip(tp, P.views))
    if kind == 'adam':
        opt = optim.Adam(tp, lr=LR, weight_decay=0)
        for p, m, v in zip(tp, M.views, V.views):        # torch's state layout, with the moments where the guards are
            opt.state[p] = {'step': torch.tensor(0.0, dtype=torch.float32), 'exp_avg': m, 'exp_avg_sq': v}
    else:
        opt = optim.SGD(tp, lr=LR, weight_decay=0)
    for gs in grads:
        for p, gv, g in zip(tp, G.views, gs):
            if g is None:
                p.grad = None
            else:
                gv.copy_(torch.from_numpy(g))
                p.grad = gv
        opt.step()
    torch.cuda.synchronize()
    for buf, what in ((P, 'params'), (G, 'grads'), (M, 'exp_avg'), (V, 'exp_avg_sq')):
        buf.assert_guards_untouched(what)
    res = [[v.cpu().numpy() for v in b.views] for b in (P, M, V)]
    return res[0], res[1], res[2], opt


def _check(kind, params, grads, got, misaligned=()):
    gp, gm, gv = got
    tp, tm, tv = _torch_run(kind, params, grads)
    r64 = (nor.AdamRef(params, lr=LR, dtype=np.float64) if kind == 'adam' else nor.SgdRef(params, lr=LR, dtype=np.float64))
    for gs in grads:
        r64.step(gs)
    for i in range(len(params)):
        tag = '{} tensor {} ({} elements)'.format(kind, i, params[i].size)
        assert_float_path(gp[i], tp[i], r64.p[i], err_msg=tag)
        if kind == 'adam':
            assert_grad_path(gm[i], tm[i], r64.m[i], err_msg=tag + ' exp_avg')
            assert_grad_path(gv[i], tv[i], r64.v[i], err_msg=tag + ' exp_avg_sq')
    return r64


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_edge_shapes_in_one_call(kind):
    """eight aligned tensors around the 16-byte width and the chunk size, and a ninth that starts one float into its
    storage (full chunks and a tail on the element-by-element path); three steps with fresh gradients"""
    c = _chunk()
    numels = _edge_numels() + [c + 5]
    params, grads = _draw(numels, 3, seed=21)
    gp, gm, gv, opt = _native_run(kind, params, grads, misaligned=(8,))
    _check(kind, params, grads, (gp, gm, gv))
    if kind == 'adam':
        assert [int(opt.state[p]['step']) for p in opt.param_groups[0]['params']] == [3] * 9
        assert [opt._handles[0][1].steps(i) for i in range(9)] == [3] * 9
    assert len(opt._handles) == 1


def test_more_tensors_than_one_launch_holds():
    """75 small tensors: three launches behind one library call"""
    from re2nn_seq_amd import _lib
    numels = [1 + (7 * k) % 23 for k in range(2 * _lib.OPTIM_MAX_TENSORS + 11)]
    params, grads = _draw(numels, 2, seed=22)
    grads[1][40] = None
    gp, gm, gv, _ = _native_run('adam', params, grads)
    _check('adam', params, grads, (gp, gm, gv))


def test_a_skipped_gradient_leaves_the_tensor_and_its_step_alone():
    c = _chunk()
    numels = [37, c + 9, 6]
    params, grads = _draw(numels, 3, seed=23)
    grads[1][1] = None
    from re2nn_seq_amd.farnn import optim
    tp = [torch.from_numpy(p.copy()).cuda().requires_grad_(True) for p in params]
    opt = optim.Adam(tp, lr=LR)
    snaps = []
    for gs in grads:
        for p, g in zip(tp, gs):
            p.grad = None if g is None else torch.from_numpy(g).cuda()
        opt.step()
        st = opt.state[tp[1]]
        snaps.append([t.detach().cpu().numpy().copy() for t in (tp[1], st['exp_avg'], st['exp_avg_sq'])] + [int(st['step'])])
    for a, b in zip(snaps[0][:3], snaps[1][:3]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))      # bit-unchanged by the step without a gradient
    assert [s[3] for s in snaps] == [1, 1, 2]
    assert [int(opt.state[p]['step']) for p in tp] == [3, 2, 3]
    assert [opt._handles[0][1].steps(i) for i in range(3)] == [3, 2, 3]
    got = ([p.detach().cpu().numpy() for p in tp], [opt.state[p]['exp_avg'].cpu().numpy() for p in tp],
           [opt.state[p]['exp_avg_sq'].cpu().numpy() for p in tp])
    r64 = _check('adam', params, grads, got)             # the restatement and torch skipped likewise
    assert r64.t == [3, 2, 3]
    assert np.abs(snaps[2][0] - snaps[1][0]).max() > 100 * 1e-4         # and the third update did move it


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_zero_gradients_from_the_first_step_change_nothing(kind):
    numels = _edge_numels()
    params, _ = _draw(numels, 1, seed=24)
    grads = [[np.zeros(n, np.float32) for n in numels] for _ in range(2)]
    gp, gm, gv, _ = _native_run(kind, params, grads)
    for p, g in zip(params, gp):
        assert np.array_equal(p.view(np.uint32), g.view(np.uint32))
    if kind == 'adam':
        assert all(not m.any() for m in gm) and all(not v.any() for v in gv)


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_two_runs_from_the_same_state_are_bit_identical(kind):
    c = _chunk()
    numels = _edge_numels() + [c + 5]
    params, grads = _draw(numels, 3, seed=25)
    a = _native_run(kind, params, grads, misaligned=(8,))[:3]
    b = _native_run(kind, params, grads, misaligned=(8,))[:3]
    for xs, ys in zip(a, b):
        for x, y in zip(xs, ys):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def _steps(opt, tp, grads):
    for gs in grads:
        for p, g in zip(tp, gs):
            p.grad = torch.from_numpy(g).cuda()
        opt.step()


@pytest.mark.parametrize('first', ['native', 'torch'])
def test_state_dicts_interchange_with_torch(first):
    """two steps by one optimizer, its state_dict() loaded into the other kind on a copy of the parameters, one more step by
    each: the same results by the rule, both against the restatement's three steps"""
    from re2nn_seq_amd.farnn import optim
    c = _chunk()
    numels = [5, c + 3, 130]
    params, grads = _draw(numels, 3, seed=26)
    kinds = {'native': optim.Adam, 'torch': torch.optim.Adam}
    second = 'torch' if first == 'native' else 'native'
    tp1 = [torch.from_numpy(p.copy()).cuda().requires_grad_(True) for p in params]
    o1 = kinds[first](tp1, lr=LR, weight_decay=0)
    _steps(o1, tp1, grads[:2])
    tp2 = [p.detach().clone().requires_grad_(True) for p in tp1]
    o2 = kinds[second](tp2, lr=0.5, weight_decay=0)                      # (lr comes with the loaded groups)
    o2.load_state_dict(copy.deepcopy(o1.state_dict()))
    assert o2.param_groups[0]['lr'] == LR
    assert [int(o2.state[p]['step']) for p in tp2] == [2, 2, 2]
    _steps(o1, tp1, grads[2:])
    _steps(o2, tp2, grads[2:])
    torch.cuda.synchronize()
    r32, r64 = nor.AdamRef(params, lr=LR, dtype=np.float32), nor.AdamRef(params, lr=LR, dtype=np.float64)
    for gs in grads:
        r32.step(gs)
        r64.step(gs)
    for o, tp, name in ((o1, tp1, first), (o2, tp2, second)):
        assert [int(o.state[p]['step']) for p in tp] == [3, 3, 3]
        if name == 'native':
            assert [o._handles[0][1].steps(i) for i in range(3)] == [3, 3, 3]
        for i, p in enumerate(tp):
            assert_float_path(p.detach().cpu().numpy(), r32.p[i], r64.p[i], err_msg='{} tensor {}'.format(name, i))
            assert_grad_path(o.state[p]['exp_avg'].cpu().numpy(), r32.m[i], r64.m[i], err_msg='{} exp_avg {}'.format(name, i))
            assert_grad_path(o.state[p]['exp_avg_sq'].cpu().numpy(), r32.v[i], r64.v[i], err_msg='{} exp_avg_sq {}'.format(name, i))
    for i, (a, b) in enumerate(zip(tp1, tp2)):                           # and each other, with torch as the float32 reference
        nat, tor = (a, b) if first == 'native' else (b, a)
        assert_float_path(nat.detach().cpu().numpy(), tor.detach().cpu().numpy(), r64.p[i], err_msg='native against torch')


def test_non_contiguous_parameters_and_gradients_raise():
    from re2nn_seq_amd.farnn import optim
    base = torch.zeros((6, 8), device='cuda')
    p = base.t().detach().requires_grad_(True)
    opt = optim.Adam([p], lr=LR)
    p.grad = torch.ones((8, 6), device='cuda')
    with pytest.raises(ValueError, match='contiguous'):
        opt.step()
    q = torch.zeros((8, 6), device='cuda', requires_grad=True)
    opt = optim.SGD([q], lr=LR)
    q.grad = torch.ones((6, 8), device='cuda').t()
    with pytest.raises(ValueError, match='contiguous'):
        opt.step()
    torch.cuda.synchronize()
    assert not q.detach().any() and not base.any()


def test_create_refusals_and_a_valid_create_afterwards():
    from re2nn_seq_amd import _lib
    lib = _lib.load()
    out = ctypes.c_void_p()
    good = _lib.OptimDesc(_lib.OPTIM_ADAM, LR, 0.9, 0.999, 1e-8)
    assert lib.farnn_optim_create(ctypes.byref(good), (ctypes.c_int64 * 2)(5, 0), 2, 0, ctypes.byref(out)) == -22      # FARNN_EINVAL
    assert not out.value
    assert lib.farnn_optim_create(ctypes.byref(_lib.OptimDesc(7, LR, 0.9, 0.999, 1e-8)), (ctypes.c_int64 * 1)(5), 1, 0,
                                  ctypes.byref(out)) == -22
    assert not out.value
    h = _lib.Optim(_lib.OPTIM_ADAM, [5, 3], LR)
    p, g = torch.ones(8, device='cuda'), torch.ones(8, device='cuda')
    m, v = torch.zeros(8, device='cuda'), torch.zeros(8, device='cuda')
    ptrs = lambda t: [t.data_ptr(), t.data_ptr() + 20]                   # noqa: E731
    with pytest.raises(_lib.FarnnError, match='exp_avg'):                # a moment pointer missing under Adam
        h.step(ptrs(p), ptrs(g), [m.data_ptr(), None], ptrs(v))
    assert h.steps(0) == 0 and h.steps(1) == 0
    h.step(ptrs(p), ptrs(g), ptrs(m), ptrs(v), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert h.steps(0) == 1 and h.steps(1) == 1
    np.testing.assert_allclose(p.cpu().numpy(), np.full(8, 1.0 - LR, np.float32), rtol=1e-6)
    h.set_steps(1, 41)
    assert h.steps(1) == 41
    with pytest.raises(_lib.FarnnError):
        h.steps(2)
    h.close()


def test_onehot_ifst_trained_end_to_end_by_the_library_optimizer():
    """the synthetic automaton of test_gpu_onehot_train.py, three batches of 8 x 10, tanh, farnn.optim.Adam(lr = 0.05):
    language_tensor after three steps against the torch restatement's three Adam steps in float32 and float64"""
    from re2nn_seq_amd import synth
    from re2nn_seq_amd.farnn import optim
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I_S
    from re2nn_seq_amd.wfa import fsa_to_tensor as f2t
    dset, automaton = synth.make_dataset(60, 4, 20, 4)[:2]
    t2i = dict(dset['t2i']); t2i['<pad>'] = len(t2i)
    s2i = dset['s2i']
    V = len(t2i)
    T, _, W, O, Ow, fin, sta, _ = f2t.dfa_to_tensor_slot_single_wildcard(automaton, t2i, s2i)
    m = FARNN_S_O_I_S(T, O, W, Ow, fin, sta, None, ns(update_nonlinear='tanh'), o_idx=s2i['o'])
    sd0 = copy.deepcopy(m.state_dict())
    rng = np.random.RandomState(3)
    batches = []
    for _ in range(3):
        x, lengths = synth.random_batch(V, 8, 10, rng, min_len=2)
        batches.append((x, lengths, rng.randint(0, O.shape[0], size=x.shape).astype(np.int64)))
    m.enable_training()
    opt = optim.Adam(list(m.parameters()), lr=LR, weight_decay=0)
    for x, lengths, labels in batches:
        opt.zero_grad()
        loss, _, _ = m.forward_local(torch.from_numpy(x), torch.from_numpy(labels), torch.from_numpy(lengths))
        loss.backward()
        opt.step()
    m.eval()
    got = m.state_dict()['language_tensor']
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    kw = dict(W=sd0['wildcard_mat'], O=sd0['output_mat'], h0=sd0['h0'], hT=sd0['hT'], P=None, batches=batches, nl='tanh', lr=LR)
    r32 = otr.adam_steps(sd0['language_tensor'], dtype=torch.float32, **kw)
    r64 = otr.adam_steps(sd0['language_tensor'], dtype=torch.float64, **kw)
    assert np.abs(r64 - np.asarray(sd0['language_tensor'], np.float64)).max() > 100 * 1e-4
    assert_float_path(got, r32, r64, err_msg='language_tensor after 3 library Adam steps')


def _count_library_steps(monkeypatch):
    from re2nn_seq_amd import _lib
    calls = []
    real = _lib.Optim.step

    def counted(self, *a, **k):
        calls.append(self.n)
        return real(self, *a, **k)
    monkeypatch.setattr(_lib.Optim, 'step', counted)
    return calls


def _losses(cli, res_path):
    saved = cli.load_res(res_path)
    return [float(line.split('LOSS:')[1]) for line in saved['logger'].record if 'LOSS:' in line]


def test_onehot_cli_trains_with_the_library_optimizer(tmp_path, monkeypatch):
    from re2nn_seq_amd import main as cli
    from re2nn_seq_amd import synth
    monkeypatch.setenv('RE2NN_NATIVE_OPTIM', '1')
    calls = _count_library_steps(monkeypatch)
    tree = synth.write_dataset_tree(str(tmp_path / 'data'), dataset='ATIS-BIO', seed=4)
    argv = ['--dataset', 'ATIS-BIO', '--method', 'onehot', '--independent', '2',
            '--automata_path', tree['paths']['ID2'], '--normalize_automata', 'none', '--rand_constant', '0',
            '--update_nonlinear', 'tanh', '--bz', '9', '--seq_max_len', '12', '--epoch', '2', '--lr', '0.01',
            '--train_portion', '1.0', '--data_dir', tree['paths']['data_dir'], '--model_dir', str(tmp_path / 'm')]
    results, stats, res_path = cli.main(argv)
    assert len(stats['train_step']) == 2 and os.path.exists(res_path)
    assert calls and set(calls) == {1}                                   # language_tensor alone, one library call per batch
    losses = _losses(cli, res_path)
    assert len(losses) == 2 and losses[1] < losses[0]


def test_decompose_cli_trains_with_the_library_optimizer(tmp_path, monkeypatch):
    """--farnn 2 --use_crf 1 at the rank the synthetic tree is written for: many small tensors and a crf.transitions gradient"""
    from re2nn_seq_amd import main as cli
    from re2nn_seq_amd import synth
    monkeypatch.setenv('RE2NN_NATIVE_OPTIM', '1')
    calls = _count_library_steps(monkeypatch)
    tree = synth.write_dataset_tree(str(tmp_path / 'data'), dataset='ATIS-BIO', seed=4)
    argv = ['--dataset', 'ATIS-BIO', '--method', 'decompose', '--independent', '2',
            '--automata_path', tree['paths']['IIID'], '--rank', '100', '--seed', '1', '--beta', '0.9',
            '--embed_dim', '16', '--normalize_automata', 'none', '--rand_constant', '0', '--use_crf', '1',
            '--farnn', '2', '--update_nonlinear', 'tanh', '--bz', '9', '--seq_max_len', '12', '--epoch', '2',
            '--lr', '0.005', '--train_portion', '1.0', '--data_dir', tree['paths']['data_dir'],
            '--model_dir', str(tmp_path / 'm')]
    results, stats, res_path = cli.main(argv)
    assert len(stats['train_step']) == 2
    assert calls and min(calls) >= 10                                    # S1, S2, the bridge, C_output_mat, six gate tensors, crf.transitions
    losses = _losses(cli, res_path)
    assert len(losses) == 2 and np.isfinite(losses).all() and losses[1] < losses[0]
