"""The shared training surface (farnn/_trainable.py, farnn/train_step.py) on the device, at V = 5, S = 4, C = 3, B = 3, L = 4
(R = 3, R_O = 2 for the decomposed models) and lengths [4, 1, 2]: a step gives the same bits whether the lengths live on the
host or on the device, the dirty flag and the copy back into the host attributes, and backward() scaling every gradient it
hands out by the incoming one."""
import numpy as np
import pytest
import torch

import trainable_models as tm

pytestmark = pytest.mark.gpu

B, L = 3, 4
LENGTHS = [4, 1, 2]
ALL_ON = dict(train_wildcard=1, train_wildcard_wildcard=1, train_h0=1, train_hT=1, train_beta=1, train_V_embed=1, train_word_embed=1)


def _switches(monkeypatch):
    for name in tm.ALL_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name in ('RE2NN_ONEHOT_FST_TRAIN', 'RE2NN_ONEHOT_IND1_TRAIN', 'RE2NN_DECOMP_IND1_TRAIN', 'RE2NN_DECOMP_IND1_CRF_TRAIN'):
        monkeypatch.setenv(name, '1')


def _batch():
    rng = np.random.RandomState(7)
    x = torch.from_numpy(rng.randint(0, tm.V, size=(B, L)).astype(np.int64))
    lab = torch.from_numpy(rng.randint(0, tm.C, size=(B, L)).astype(np.int64))
    return x, lab, torch.tensor(LENGTHS, dtype=torch.int64)


def _step(m, x, lab, lengths):
    """one forward_local(train=True) + backward: (loss, pred, {name: grad}) as host arrays"""
    for p in m.parameters():
        p.grad = None
    loss, pred, true = m.forward_local(x, lab, lengths, train=True)
    loss.backward()
    grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in m.named_parameters()}
    return loss.detach().cpu().numpy().copy(), pred.cpu().numpy(), true.cpu().numpy(), grads


@pytest.mark.parametrize('kind', tm.KINDS)
def test_lengths_on_the_host_or_on_the_device_give_the_same_bits(monkeypatch, kind):
    """The two calls differ in where the token count is taken (forward_local on the host, the step on the device) and must not
    differ in its value.  The decomposed i-FST's step adds each sequence's share of dh0, dhT and of d Osum (a part of
    d C_output_mat) with float atomics from its workgroups (csrc/train.hip.h), so those three tensors' last bit also depends on
    the order the workgroups arrive in: at this batch (two workgroups per direction, the shorter one first) the order has held;
    with the gates and the CRF on, C_output_mat was seen one ulp apart between two calls (7.6e-6 at |g| = 52) with every other
    tensor and the loss equal, which is why that configuration is not a case here."""
    _switches(monkeypatch)
    m = tm.build(kind)
    x, lab, lengths = _batch()
    dev = m._dev()
    loss_h, pred_h, true_h, g_h = _step(m, x, lab, lengths)
    loss_d, pred_d, true_d, g_d = _step(m, x.to(dev), lab.to(dev), lengths.to(dev))
    print(kind, 'loss', float(loss_h), float(loss_d), {k: float(np.abs(g_h[k] - g_d[k]).max()) for k in g_h})
    assert np.isfinite(loss_h) and pred_h.shape == (sum(LENGTHS),)
    assert loss_h.tobytes() == loss_d.tobytes()
    assert np.array_equal(pred_h, pred_d) and np.array_equal(true_h, true_d)
    assert list(g_h) == list(g_d) == [k for k, _ in m.named_parameters()] and g_h
    for k in g_h:
        assert g_h[k].tobytes() == g_d[k].tobytes(), k


@pytest.mark.parametrize('kind', tm.KINDS + ('edge_ifst',))
def test_the_dirty_flag_and_the_copy_back(monkeypatch, kind):
    _switches(monkeypatch)
    m = tm.build_edge_ifst() if kind == 'edge_ifst' else tm.build(kind)
    x, lab, lengths = _batch()
    m.forward_local(x, lab, lengths, train=False)          # a tagging handle built from the weights as they are
    assert m._h is not None
    m.enable_training()
    assert m._dirty is False
    before = {k: t.detach().cpu().clone() for k, t in m.named_parameters()}
    opt = torch.optim.SGD(list(m.parameters()), lr=0.5)
    loss, _, _ = m.forward_local(x, lab, lengths, train=True)
    assert m._dirty is True and m._h is not None
    loss.backward()
    opt.step()
    assert m.eval() is m and m.training is False
    assert m._dirty is False and m._h is None               # the handle's copy of the weights was stale
    sd = m.state_dict()
    for k, t in m.named_parameters():
        now = t.detach().cpu()
        assert not torch.equal(now, before[k]), k
        assert np.array_equal(np.asarray(sd[k]), now.numpy()), k
    if kind == 'edge_ifst':
        assert m.edges is None and m.language_tensor.shape == (tm.V, tm.S, tm.S)
    h = m.handle
    m.eval()                                               # nothing changed since: the second eval() keeps the handle
    assert m._h is h and m._dirty is False


SCALING = [('onehot_ifst', {}), ('onehot_fst', {}), ('onehot_fst', dict(train_wildcard=1)), ('onehot_ind1', {}),
           ('decomp_ifst', {}), ('decomp_ifst', dict(ALL_ON, farnn=2, use_crf=1)), ('decomp_ind1', ALL_ON),
           ('decomp_ind1', dict(ALL_ON, use_crf=1))]


@pytest.mark.parametrize('kind,kw', SCALING, ids=lambda v: v if isinstance(v, str) else ('crf' if v.get('use_crf') else 'flags' if v else 'default'))
def test_backward_scales_every_gradient_by_the_incoming_one(monkeypatch, kind, kw):
    """(2 * loss).backward() against loss.backward() on one forward call: scaling by two is exact, so the gradients are twice the
    others bit for bit, in every slot backward() returns"""
    _switches(monkeypatch)
    m = tm.build(kind, **kw)
    x, lab, lengths = _batch()
    loss, _, _ = m.forward_local(x, lab, lengths, train=True)
    named = list(m.named_parameters())
    loss.backward(retain_graph=True)
    once = {k: p.grad.detach().cpu().numpy().copy() for k, p in named}
    for _, p in named:
        p.grad = None
    (2 * loss).backward()
    twice = {k: p.grad.detach().cpu().numpy().copy() for k, p in named}
    want = {'onehot_fst': ['language_tensor'] + ['wildcard_tensor'] * bool(kw)}.get(kind)
    if want is not None:
        assert list(once) == want
    if kw.get('use_crf'):
        assert 'crf.transitions' in once
    if kw.get('farnn') == 2:
        assert all(k in once for k in ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2'))
    for k in once:
        assert np.isfinite(once[k]).all() and np.abs(once[k]).max() > 0, k
        assert (2 * once[k]).tobytes() == twice[k].tobytes(), k
