"""The HIP training step of the decomposed i-FST against loss and gradients captured from the
reference's forward_local(train=True) + backward(), and against the torch-fp32 oracle on other shapes."""
import json
import os
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')

from oracle import farnn_train_oracle as to  # noqa: E402
from util import assert_grad_path, check_grad, present_words  # noqa: E402

pytestmark = pytest.mark.gpu

PARAMS = ('S1', 'S2', 'V_embed', 'embed_r_generalized', 'C_output_mat', 'wildcard_mat', 'h0', 'hT', 'beta_vec',
          'embedding.weight')


def ns(**kw):
    d = dict(rand_constant=0.0, train_wildcard=0, train_wildcard_wildcard=0, margin=0.3, threshold=0.5,
             train_mode='sum', local_loss_func='CE1', use_priority=0, independent=2, update_nonlinear='none',
             additional_states=0, train_word_embed=0, use_crf=0, random=0, train_h0=0, train_hT=0, train_V_embed=0,
             train_c_output=1, farnn=0, xavier=0, bias_init=5.0, sigmoid_exponent=5, beta=1.0, train_beta=0,
             additional_nonlinear='none', random_pad_func='uniform', marryup_type='none', c1_kdpr=1.0, c2_kdpr=1.0,
             c3_pr=1.0)
    d.update(kw)
    return Namespace(**d)


def load():
    with open(os.path.join(GOLDEN, 'decomp_train_small.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, 'decomp_train_small.npz')), np.load(os.path.join(GOLDEN, 'decomp_small.npz'))


def dvgen_refs(p, x, lengths, labels, nl, farnn, sig_k, prio=False):
    """d loss / d Vgen (leaf = to.generalized_table(p), the table the library is given) from the batched oracle in float32 and
    in float64, and the words that occur at a valid position"""
    table = to.generalized_table(p).detach()
    ref = []
    for dtype in (torch.float32, torch.float64):
        q = {k: v.to(dtype) if v.dtype.is_floating_point else v for k, v in p.items()}
        q.update(V_embed=table.to(dtype), beta_vec=torch.ones_like(q['beta_vec']))          # Vgen = V_embed exactly
        _, g, _ = to.train_step_batched(q, torch.from_numpy(x), torch.from_numpy(lengths), torch.from_numpy(labels), nl=nl,
                                        use_priority=prio, farnn=farnn, sig_k=sig_k)
        ref.append(g['V_embed'].numpy())
    return ref[0], ref[1], present_words(x, lengths, table.shape[0])


def check_dvgen(case, got, p, x, lengths, labels, nl, farnn, sig_k, prio=False, slices=True):
    """dVgen under the gradient rule (tests/util.py:assert_grad_path): at the tensor's scale and, with slices, row by row at
    each present word's scale and exactly zero for the words that occur at no valid position."""
    ref32, ref64, present = dvgen_refs(p, x, lengths, labels, nl, farnn, sig_k, prio)
    check_grad(case, 'dVgen', got, ref32, ref64, slices=0 if slices else None, present=present if slices else None)


def close(got, ref, name, rtol=2e-3, atol=2e-6, frac=2e-4):
    scale = max(float(np.abs(ref).max()), 1e-6)
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol + frac * scale, err_msg=name)


@pytest.mark.parametrize('k', range(10))
def test_train_step_matches_reference_loss_and_gradients(k):
    """Through the model mirror: forward_local(train=True) -> loss.backward() -> .grad of every parameter."""
    from re2nn_seq_amd.farnn.model_decompose_single import FARNN_S_D_W_I_S
    meta, g, base = load()
    cfg = meta['configs'][k]
    a = ns(**dict(meta['train_flags'], **cfg))
    torch.manual_seed(0)
    m = FARNN_S_D_W_I_S(V=base['V_in'], S1=base['S1_in'], S2=base['S2_in'], C_output_mat=base['O_in'],
                        wildcard_mat=base['W_in'], wildcard_output_vector=base['Ow_in'],
                        final_vector=base['final_in'], start_vector=base['start_in'],
                        pretrained_word_embed=base['E_in'], priority_mat=base['priority_in'], args=a,
                        o_idx=meta['o_idx'])
    pre = 'c{}.'.format(k)
    sd = {n: g[pre + 'w.' + n] for n in PARAMS}
    sd['priority_layer.priority_mat'] = g[pre + 'w.priority_mat']
    names = PARAMS
    if cfg.get('use_crf'):
        sd['crf.transitions'] = g[pre + 'w.crf.transitions']
        names = PARAMS + ('crf.transitions',)
    for n in ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2'):
        if pre + 'w.' + n in g.files:
            sd[n] = g[pre + 'w.' + n]
            names = names + (n,)
    m.load_state_dict(sd)
    x, lengths, labels = torch.from_numpy(base['x']), torch.from_numpy(base['lengths']), torch.from_numpy(g['labels'])
    m.train()
    loss, pred, true = m.forward_local(x, labels, lengths, train=True)
    loss.backward()
    ref_loss = float(g[pre + 'loss'])
    assert abs(float(loss.detach()) - ref_loss) < 2e-5 * max(1.0, abs(ref_loss))
    assert np.array_equal(pred.cpu().numpy(), g[pre + 'flat_pred'])
    named = dict(m.named_parameters())
    assert set(named) == set(names)
    for n in names:
        close(named[n].grad.cpu().numpy(), g[pre + 'g.' + n], n)


@pytest.mark.parametrize('S,R,K,V,B,L,nl,prio', [
    (104, 50, 73, 300, 12, 20, 'tanh', False),     # SNIPS-sized factors
    (23, 70, 9, 50, 7, 9, 'relutanh', True),       # rank above the state count
    (5, 3, 4, 11, 3, 6, 'none', False),
    (64, 64, 130, 40, 4, 33, 'relu', True),        # more score columns than a wavefront
    (7, 5, 3, 9, 1, 1, 'tanh', False),             # one sequence of one token
    (130, 9, 5, 20, 3, 2, 'tanh', True),           # more states than two wavefronts' columns, odd rank
])
def test_train_step_c_abi_vs_oracle(S, R, K, V, B, L, nl, prio):
    """The C-ABI entry point directly, with empty and full-length sequences, against the oracle."""
    from re2nn_seq_amd import _lib
    rng = np.random.RandomState(S + R)
    f = lambda *shape, sc=0.3: torch.from_numpy((rng.randn(*shape) * sc).astype(np.float32))   # noqa: E731
    D = 6
    # automaton-like magnitudes: every state feeds one label (Osum near 0/1), about one wildcard edge per state
    Cm = np.zeros((K, S), np.float32)
    Cm[rng.randint(0, K, size=S), np.arange(S)] = (rng.rand(S) < 0.8)
    p = {'S1': f(S, R, sc=1.0 / np.sqrt(S)), 'S2': f(S, R, sc=1.0 / np.sqrt(S)), 'V_embed': f(V, R, sc=0.8),
         'embed_r_generalized': f(D, R),
         'C_output_mat': torch.from_numpy(Cm + (rng.rand(K, S) * 0.02).astype(np.float32)),
         'wildcard_mat': torch.from_numpy(((rng.rand(S, S) < 1.0 / S) * 0.5).astype(np.float32)),
         'h0': f(S, sc=0.5), 'hT': f(S, sc=0.5), 'beta_vec': torch.full((R,), 0.7), 'embedding.weight': f(V, D),
         'priority_mat': torch.from_numpy((np.eye(K) + (rng.rand(K, K) < 0.05) * 0.5).astype(np.float32))}
    lengths = rng.randint(1, L + 1, size=B).astype(np.int64)
    lengths[0] = L
    if B > 3:
        lengths[1] = 0
    x = rng.randint(0, V, size=(B, L)).astype(np.int64)
    labels = rng.randint(0, K, size=(B, L)).astype(np.int64)
    xt, lt, lab = torch.from_numpy(x), torch.from_numpy(lengths), torch.from_numpy(labels)
    loss_ref, grads_ref, _ = to.train_step(p, xt, lt, lab, nl=nl, use_priority=prio)
    # d loss / d Vgen from the oracle, to compare the library's dVgen itself
    q = {k: v.clone() for k, v in p.items()}
    Vgen = to.generalized_table(q).detach().requires_grad_(True)
    leaves = {n: q[n].clone().requires_grad_(True) for n in ('S1', 'S2', 'wildcard_mat', 'C_output_mat', 'h0', 'hT')}
    s = to.chain_scores(Vgen, leaves['S1'], leaves['S2'], leaves['wildcard_mat'], leaves['C_output_mat'], leaves['h0'],
                        leaves['hT'], xt, lt, nl, q['priority_mat'] if prio else None)
    flat_labels = torch.cat([lab[b, :int(lt[b])] for b in range(B)])
    torch.nn.functional.cross_entropy(s, flat_labels).backward()

    dev = torch.device('cuda')
    tc = _lib.TrainContext(V, S, R, K, nl=nl, threshold=0.5, o_idx=1)
    w = {'Vgen': Vgen.detach().to(dev), 'S1': p['S1'].to(dev), 'S2': p['S2'].to(dev), 'W': p['wildcard_mat'].to(dev),
         'C': p['C_output_mat'].to(dev), 'h0': p['h0'].to(dev), 'hT': p['hT'].to(dev)}
    P = p['priority_mat'].to(dev) if prio else None
    out = {'d' + n: torch.full_like(t, 7.0) for n, t in w.items()}           # the library must zero them itself
    loss = torch.full((1,), 3.0, device=dev)
    tags = torch.empty((B, L), dtype=torch.int32, device=dev)
    xd, ld, labd = xt.to(dev), lt.to(dev), lab.to(dev)
    for _ in range(2):                                                        # twice: the workspace is reused
        tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None if P is None else P.data_ptr()),
                xd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, int(lengths.sum()),
                dict({n: t.data_ptr() for n, t in out.items()}, loss=loss.data_ptr(), tags=tags.data_ptr()))
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss_ref)) < 5e-5 * max(1.0, abs(float(loss_ref)))
    close(out['dVgen'].cpu().numpy(), Vgen.grad.numpy(), 'dVgen')
    for n, key in (('S1', 'S1'), ('S2', 'S2'), ('W', 'wildcard_mat'), ('C', 'C_output_mat'), ('h0', 'h0'), ('hT', 'hT')):
        close(out['d' + n].cpu().numpy(), leaves[key].grad.numpy(), 'd' + n)
        close(out['d' + n].cpu().numpy(), grads_ref[key].numpy(), 'd' + n + ' (full graph)')
    # repeated steps give the same gradients up to the summation order of the atomics (and never a NaN: partial
    # reduction rounds once multiplied a masked input by whatever LDS held past the matrix)
    first = {n: t.clone() for n, t in out.items()}
    for _ in range(10):
        tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None if P is None else P.data_ptr()),
                xd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, int(lengths.sum()),
                dict({n: t.data_ptr() for n, t in out.items()}, loss=loss.data_ptr(), tags=tags.data_ptr()))
        torch.cuda.synchronize()
        for n, t in out.items():
            assert torch.isfinite(t).all(), n
            assert float((t - first[n]).abs().max()) <= 1e-5 * max(1.0, float(first[n].abs().max())), n
    t = tags.cpu().numpy()
    mask = np.arange(L)[None, :] < lengths[:, None]
    assert (t[~mask] == -1).all()
    sc = s.detach().numpy().copy()
    sc[:, K - 1] = np.minimum(sc[:, K - 1], 0.5)
    want = sc.argmax(1)
    want[want == K - 1] = 1
    assert (t[mask] == want).mean() > 0.99                                   # ties / 1-ulp score differences aside


def test_training_loop_reduces_the_loss_and_tagging_sees_the_update():
    """A few Adam steps through the mirror, then eval: the tagging handle is rebuilt from the trained tensors."""
    from re2nn_seq_amd.farnn.model_decompose_single import FARNN_S_D_W_I_S
    meta, g, base = load()
    a = ns(**dict(meta['train_flags'], update_nonlinear='tanh', beta=0.7))
    m = FARNN_S_D_W_I_S(V=base['V_in'], S1=base['S1_in'], S2=base['S2_in'], C_output_mat=base['O_in'],
                        wildcard_mat=base['W_in'], wildcard_output_vector=base['Ow_in'],
                        final_vector=base['final_in'], start_vector=base['start_in'],
                        pretrained_word_embed=base['E_in'], priority_mat=base['priority_in'], args=a,
                        o_idx=meta['o_idx'])
    x, lengths, labels = torch.from_numpy(base['x']), torch.from_numpy(base['lengths']), torch.from_numpy(g['labels'])
    _, before, _ = m.forward_local(x, labels, lengths, train=False)
    m.train()
    m.enable_training()
    opt = torch.optim.Adam(list(m.parameters()), lr=0.02)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss, _, _ = m.forward_local(x, labels, lengths, train=True)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < 0.7 * losses[0], losses
    m.eval()
    _, after, true = m.forward_local(x, labels, lengths, train=False)
    assert (after == true).float().mean() > (before == true).float().mean()


@pytest.mark.parametrize('S,R,K,V,B,L,nl,prio', [
    (104, 50, 75, 200, 9, 40, 'tanh', False),      # SNIPS-sized label set + START/STOP
    (20, 8, 6, 30, 5, 7, 'relu', True),
    (71, 30, 130, 120, 6, 64, 'tanh', False),      # ATIS-sized label set (C=128 + 2) at L=64: the CRF kernel's large-K form
    (40, 20, 140, 60, 3, 64, 'tanh', False),       # the largest tag set that fits at L=64
])
def test_train_step_crf_c_abi_vs_oracle(S, R, K, V, B, L, nl, prio):
    """CRF mode of the C-ABI entry point (loss = sum of log Z - gold score) against the oracle, with an empty and a
    full-length sequence; the decoded tags are the Viterbi path of the clamped emissions."""
    from re2nn_seq_amd import _lib
    from oracle import farnn_oracle as fo
    rng = np.random.RandomState(S + K)
    f = lambda *shape, sc=0.3: torch.from_numpy((rng.randn(*shape) * sc).astype(np.float32))   # noqa: E731
    D = 6
    Cm = np.zeros((K, S), np.float32)
    Cm[rng.randint(0, K - 2, size=S), np.arange(S)] = (rng.rand(S) < 0.8)
    tr = (rng.randn(K, K) * 0.3).astype(np.float32)
    tr[:, K - 2] = -10000.0
    tr[K - 1, :] = -10000.0
    p = {'S1': f(S, R, sc=1.0 / np.sqrt(S)), 'S2': f(S, R, sc=1.0 / np.sqrt(S)), 'V_embed': f(V, R, sc=0.8),
         'embed_r_generalized': f(D, R), 'C_output_mat': torch.from_numpy(Cm + (rng.rand(K, S) * 0.02).astype(np.float32)),
         'wildcard_mat': torch.from_numpy(((rng.rand(S, S) < 1.0 / S) * 0.5).astype(np.float32)),
         'h0': f(S, sc=0.5), 'hT': f(S, sc=0.5), 'beta_vec': torch.full((R,), 0.7), 'embedding.weight': f(V, D),
         'priority_mat': torch.from_numpy((np.eye(K) + (rng.rand(K, K) < 0.05) * 0.5).astype(np.float32)),
         'crf.transitions': torch.from_numpy(tr)}
    lengths = rng.randint(1, L + 1, size=B).astype(np.int64)
    lengths[0] = L
    lengths[1] = 0
    x = rng.randint(0, V, size=(B, L)).astype(np.int64)
    labels = rng.randint(0, K - 2, size=(B, L)).astype(np.int64)
    xt, lt, lab = torch.from_numpy(x), torch.from_numpy(lengths), torch.from_numpy(labels)
    loss_ref, grads_ref, flat_scores = to.train_step(p, xt, lt, lab, nl=nl, use_priority=prio)
    dev = torch.device('cuda')
    Vgen = to.generalized_table(p)
    w = {'Vgen': Vgen.to(dev), 'S1': p['S1'].to(dev), 'S2': p['S2'].to(dev), 'W': p['wildcard_mat'].to(dev),
         'C': p['C_output_mat'].to(dev), 'h0': p['h0'].to(dev), 'hT': p['hT'].to(dev)}
    P = p['priority_mat'].to(dev) if prio else None
    trd = p['crf.transitions'].to(dev)
    tc = _lib.TrainContext(V, S, R, K, nl=nl, threshold=0.5, o_idx=1, use_crf=True)
    out = {'d' + n: torch.full_like(t, 7.0) for n, t in w.items()}
    dtr = torch.full_like(trd, 7.0)
    loss = torch.full((1,), 3.0, device=dev)
    tags = torch.empty((B, L), dtype=torch.int32, device=dev)
    xd, ld, labd = xt.to(dev), lt.to(dev), lab.to(dev)
    for _ in range(2):
        tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None if P is None else P.data_ptr(), crf_trans=trd.data_ptr()),
                xd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, int(lengths.sum()),
                dict({n: t.data_ptr() for n, t in out.items()}, loss=loss.data_ptr(), tags=tags.data_ptr(),
                     dtrans=dtr.data_ptr()))
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss_ref)) < 5e-5 * max(1.0, abs(float(loss_ref)))
    for n, key in (('S1', 'S1'), ('S2', 'S2'), ('W', 'wildcard_mat'), ('C', 'C_output_mat'), ('h0', 'h0'), ('hT', 'hT')):
        close(out['d' + n].cpu().numpy(), grads_ref[key].numpy(), 'd' + n)
    close(dtr.cpu().numpy(), grads_ref['crf.transitions'].numpy(), 'dtrans')
    # Viterbi tags of the oracle's scores
    sc = np.zeros((B, L, K), np.float32)
    o = 0
    for b in range(B):
        n = int(lengths[b])
        sc[b, :n] = flat_scores[o:o + n].numpy()
        o += n
    want = fo.decode_crf(sc, lengths, tr, 0.5, 1)
    t = tags.cpu().numpy()
    mask = np.arange(L)[None, :] < lengths[:, None]
    assert (t[~mask] == -1).all()
    assert (t[mask] == want[mask]).mean() > 0.98


@pytest.mark.parametrize('farnn,S,R,K,V,B,L,nl,crf', [
    (2, 104, 50, 75, 200, 9, 30, 'tanh', True),       # the shipped example configurations' shape: gates + CRF
    (1, 23, 40, 9, 50, 7, 9, 'relu', False),
    (2, 5, 3, 4, 11, 3, 6, 'none', False),
])
def test_train_step_gated_c_abi_vs_oracle(farnn, S, R, K, V, B, L, nl, crf):
    """GRU-gated recurrence (farnn 1/2) through the C-ABI entry point against the oracle, with an empty sequence."""
    from re2nn_seq_amd import _lib
    rng = np.random.RandomState(S + R + farnn)
    f = lambda *shape, sc=0.3: torch.from_numpy((rng.randn(*shape) * sc).astype(np.float32))   # noqa: E731
    D = 6
    Cm = np.zeros((K, S), np.float32)
    Cm[rng.randint(0, K - (2 if crf else 0), size=S), np.arange(S)] = (rng.rand(S) < 0.8)
    p = {'S1': f(S, R, sc=1.0 / np.sqrt(S)), 'S2': f(S, R, sc=1.0 / np.sqrt(S)), 'V_embed': f(V, R, sc=0.8),
         'embed_r_generalized': f(D, R), 'C_output_mat': torch.from_numpy(Cm + (rng.rand(K, S) * 0.02).astype(np.float32)),
         'wildcard_mat': torch.from_numpy(((rng.rand(S, S) < 1.0 / S) * 0.5).astype(np.float32)),
         'h0': f(S, sc=0.5), 'hT': f(S, sc=0.5), 'beta_vec': torch.full((R,), 0.7), 'embedding.weight': f(V, D),
         'priority_mat': torch.eye(K),
         'Wss1': f(S, S, sc=0.5 / np.sqrt(S)), 'Wrs1': f(R, S, sc=0.5 / np.sqrt(R)), 'bs1': f(1, S, sc=0.5)}
    if farnn == 2:
        p.update(Wss2=f(S, S, sc=0.5 / np.sqrt(S)), Wrs2=f(R, S, sc=0.5 / np.sqrt(R)), bs2=f(1, S, sc=0.5))
    if crf:
        tr = (rng.randn(K, K) * 0.3).astype(np.float32)
        tr[:, K - 2] = -10000.0
        tr[K - 1, :] = -10000.0
        p['crf.transitions'] = torch.from_numpy(tr)
    lengths = rng.randint(1, L + 1, size=B).astype(np.int64)
    lengths[0] = L
    if B > 2:
        lengths[1] = 0
    x = rng.randint(0, V, size=(B, L)).astype(np.int64)
    labels = rng.randint(0, K - (2 if crf else 0), size=(B, L)).astype(np.int64)
    xt, lt, lab = torch.from_numpy(x), torch.from_numpy(lengths), torch.from_numpy(labels)
    loss_ref, grads_ref, _ = to.train_step(p, xt, lt, lab, nl=nl, farnn=farnn, sig_k=2.0)
    dev = torch.device('cuda')
    gate_names = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')[:3 * farnn]
    w = {'Vgen': to.generalized_table(p).to(dev), 'S1': p['S1'].to(dev), 'S2': p['S2'].to(dev), 'W': p['wildcard_mat'].to(dev),
         'C': p['C_output_mat'].to(dev), 'h0': p['h0'].to(dev), 'hT': p['hT'].to(dev)}
    w.update({n: p[n].to(dev).contiguous() for n in gate_names})
    trd = p['crf.transitions'].to(dev) if crf else None
    tc = _lib.TrainContext(V, S, R, K, nl=nl, threshold=0.5, o_idx=1, use_crf=crf, farnn=farnn, sigmoid_exponent=2.0)
    out = {'d' + n: torch.full_like(t, 7.0) for n, t in w.items()}
    dtr = torch.full_like(trd, 7.0) if crf else None
    loss = torch.full((1,), 3.0, device=dev)
    tags = torch.empty((B, L), dtype=torch.int32, device=dev)
    xd, ld, labd = xt.to(dev), lt.to(dev), lab.to(dev)
    for _ in range(2):
        tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None, crf_trans=None if trd is None else trd.data_ptr()),
                xd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, int(lengths.sum()),
                dict({n: t.data_ptr() for n, t in out.items()}, loss=loss.data_ptr(), tags=tags.data_ptr(),
                     dtrans=None if dtr is None else dtr.data_ptr()))
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss_ref)) < 5e-5 * max(1.0, abs(float(loss_ref)))
    for n, key in (('S1', 'S1'), ('S2', 'S2'), ('W', 'wildcard_mat'), ('C', 'C_output_mat'), ('h0', 'h0'), ('hT', 'hT')) + \
            tuple((n, n) for n in gate_names):
        close(out['d' + n].cpu().numpy(), grads_ref[key].numpy().reshape(out['d' + n].shape), 'd' + n)
    if crf:
        close(dtr.cpu().numpy(), grads_ref['crf.transitions'].numpy(), 'dtrans')
    for n, t in out.items():
        assert torch.isfinite(t).all(), n


@pytest.mark.parametrize('farnn,crf', [(0, False), (2, True)])
def test_train_step_full_size_vs_batched_oracle(farnn, crf):
    """BASELINE-sized batch (256 x 64, S=104, R=50) through the C-ABI against the batch-vectorised oracle."""
    from re2nn_seq_amd import _lib, synth
    rng = np.random.RandomState(5 + farnn)
    V, S, R, K, B, L, D = 2000, 104, 50, 75 if crf else 73, 256, 64, 16
    f = lambda *shape, sc=0.3: torch.from_numpy((rng.randn(*shape) * sc).astype(np.float32))   # noqa: E731
    Cm = np.zeros((K, S), np.float32)
    Cm[rng.randint(0, K - (2 if crf else 0), size=S), np.arange(S)] = (rng.rand(S) < 0.8)
    p = {'S1': f(S, R, sc=1.0 / np.sqrt(S)), 'S2': f(S, R, sc=1.0 / np.sqrt(S)), 'V_embed': f(V, R, sc=0.8),
         'embed_r_generalized': f(D, R), 'C_output_mat': torch.from_numpy(Cm + (rng.rand(K, S) * 0.02).astype(np.float32)),
         'wildcard_mat': torch.from_numpy(((rng.rand(S, S) < 1.0 / S) * 0.5).astype(np.float32)),
         'h0': f(S, sc=0.5), 'hT': f(S, sc=0.5), 'beta_vec': torch.full((R,), 0.7), 'embedding.weight': f(V, D),
         'priority_mat': torch.eye(K)}
    gate_names = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')[:3 * farnn]
    for n in gate_names:
        p[n] = f(1, S, sc=0.5) if n.startswith('bs') else (f(S, S, sc=0.5 / np.sqrt(S)) if n.startswith('Wss') else f(R, S, sc=0.5 / np.sqrt(R)))
    if crf:
        tr = (rng.randn(K, K) * 0.3).astype(np.float32)
        tr[:, K - 2] = -10000.0
        tr[K - 1, :] = -10000.0
        p['crf.transitions'] = torch.from_numpy(tr)
    x, lengths = synth.random_batch(V, B, L, rng)
    labels = rng.randint(0, K - (2 if crf else 0), size=(B, L)).astype(np.int64)
    xt, lt, lab = torch.from_numpy(x), torch.from_numpy(lengths), torch.from_numpy(labels)
    loss_ref, grads_ref, _ = to.train_step_batched(p, xt, lt, lab, nl='tanh', farnn=farnn, sig_k=3.0)
    dev = torch.device('cuda')
    w = {'Vgen': to.generalized_table(p).to(dev), 'S1': p['S1'].to(dev), 'S2': p['S2'].to(dev), 'W': p['wildcard_mat'].to(dev),
         'C': p['C_output_mat'].to(dev), 'h0': p['h0'].to(dev), 'hT': p['hT'].to(dev)}
    w.update({n: p[n].to(dev).contiguous() for n in gate_names})
    trd = p['crf.transitions'].to(dev) if crf else None
    tc = _lib.TrainContext(V, S, R, K, nl='tanh', threshold=0.5, o_idx=1, use_crf=crf, farnn=farnn, sigmoid_exponent=3.0)
    out = {'d' + n: torch.full_like(t, 7.0) for n, t in w.items()}           # the library must zero them itself
    dtr = torch.empty_like(trd) if crf else None
    loss = torch.empty(1, device=dev)
    tags = torch.empty((B, L), dtype=torch.int32, device=dev)
    xd, ld, labd = xt.to(dev), lt.to(dev), lab.to(dev)          # kept alive: the call takes raw pointers
    tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None, crf_trans=None if trd is None else trd.data_ptr()),
            xd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, int(lengths.sum()),
            dict({n: t.data_ptr() for n, t in out.items()}, loss=loss.data_ptr(), tags=tags.data_ptr(),
                 dtrans=None if dtr is None else dtr.data_ptr()))
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss_ref)) < 1e-4 * max(1.0, abs(float(loss_ref)))
    for n, key in (('S1', 'S1'), ('S2', 'S2'), ('W', 'wildcard_mat'), ('C', 'C_output_mat'), ('h0', 'h0'), ('hT', 'hT')) + \
            tuple((n, n) for n in gate_names):
        close(out['d' + n].cpu().numpy(), grads_ref[key].numpy().reshape(out['d' + n].shape), 'd' + n, rtol=5e-3)
    if crf:
        close(dtr.cpu().numpy(), grads_ref['crf.transitions'].numpy(), 'dtrans', rtol=5e-3)
    case = 'full-size farnn{} crf{}'.format(farnn, int(crf))
    if not crf:
        check_dvgen(case, out['dVgen'].cpu().numpy(), p, x, lengths, labels, 'tanh', farnn, 3.0)
    else:
        # float32 carries log Z of a 75-tag CRF to about eps x log Z: 1e-5 relative once a sequence passes ~30 tokens, which is
        # the rule's own bar for its float32 oracle (3.5 % of this batch's words sit beyond it, 1 % is the cap).  So the whole
        # batch is held to the tensor clause, and the word clause runs on a second step of the same context with every
        # sequence cut to 24 tokens, where the oracle is inside the rule's conditions.
        check_dvgen(case, out['dVgen'].cpu().numpy(), p, x, lengths, labels, 'tanh', farnn, 3.0, slices=False)
        short = np.minimum(lengths, 24)
        sd = torch.from_numpy(short).to(dev)
        tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None, crf_trans=trd.data_ptr()),
                xd.data_ptr(), sd.data_ptr(), labd.data_ptr(), B, L, int(short.sum()),
                dict({n: t.data_ptr() for n, t in out.items()}, loss=loss.data_ptr(), tags=tags.data_ptr(), dtrans=dtr.data_ptr()))
        torch.cuda.synchronize()
        check_dvgen(case + ' 24 tokens', out['dVgen'].cpu().numpy(), p, x, short, labels, 'tanh', farnn, 3.0)
    tc.close()


def test_train_step_random_configurations_soak():
    """Random shapes x gates x loss x nonlinearity x priority against the vectorised oracle
    (FARNN_TRAIN_SOAK_ITERS configurations, default 8; 1500 ran, incl. 300 through the four-sequence through-L2 kernels)."""
    from re2nn_seq_amd import _lib
    iters = int(os.environ.get('FARNN_TRAIN_SOAK_ITERS', '8'))
    badly_drawn = []
    rng = np.random.RandomState(int(os.environ.get('FARNN_TRAIN_SOAK_SEED', '123')))
    dev = torch.device('cuda')
    for it in range(iters):
        S, R = int(rng.randint(2, 140)), int(rng.randint(1, 90))
        crf = bool(rng.rand() < 0.4)
        K = int(rng.randint(4 if crf else 2, 90))
        V, B, L, D = int(rng.randint(3, 200)), int(rng.randint(1, 20)), int(rng.randint(1, 40)), 5
        farnn = int(rng.randint(0, 3))
        nl = ['none', 'relu', 'tanh', 'relutanh'][rng.randint(0, 4)]
        prio = bool(rng.rand() < 0.3)
        f = lambda *shape, sc=0.3: torch.from_numpy((rng.randn(*shape) * sc).astype(np.float32))   # noqa: E731
        Cm = np.zeros((K, S), np.float32)
        Cm[rng.randint(0, max(K - (2 if crf else 0), 1), size=S), np.arange(S)] = (rng.rand(S) < 0.8)
        fs = 0.7 / np.sqrt(max(S, R))              # contractive for every nonlinearity (a linear recurrence explodes otherwise)
        p = {'S1': f(S, R, sc=fs), 'S2': f(S, R, sc=fs), 'V_embed': f(V, R, sc=0.8),
             'embed_r_generalized': f(D, R), 'C_output_mat': torch.from_numpy(Cm + (rng.rand(K, S) * 0.02).astype(np.float32)),
             'wildcard_mat': torch.from_numpy(((rng.rand(S, S) < 1.0 / S) * 0.5).astype(np.float32)),
             'h0': f(S, sc=0.5), 'hT': f(S, sc=0.5), 'beta_vec': torch.full((R,), 0.7), 'embedding.weight': f(V, D),
             'priority_mat': torch.from_numpy((np.eye(K) + (rng.rand(K, K) < 0.05) * 0.3).astype(np.float32))}
        gate_names = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')[:3 * farnn]
        for n in gate_names:
            p[n] = f(1, S, sc=0.5) if n.startswith('bs') else (f(S, S, sc=0.5 / np.sqrt(S)) if n.startswith('Wss') else f(R, S, sc=0.5 / np.sqrt(R)))
        if crf:
            tr = (rng.randn(K, K) * 0.3).astype(np.float32)
            tr[:, K - 2] = -10000.0
            tr[K - 1, :] = -10000.0
            p['crf.transitions'] = torch.from_numpy(tr)
        lengths = rng.randint(0, L + 1, size=B).astype(np.int64)
        lengths[rng.randint(0, B)] = L
        x = rng.randint(0, V, size=(B, L)).astype(np.int64)
        labels = rng.randint(0, max(K - (2 if crf else 0), 1), size=(B, L)).astype(np.int64)
        xt, lt, lab = torch.from_numpy(x), torch.from_numpy(lengths), torch.from_numpy(labels)
        loss_ref, grads_ref, _ = to.train_step_batched(p, xt, lt, lab, nl=nl, use_priority=prio, farnn=farnn, sig_k=2.0)
        w = {'Vgen': to.generalized_table(p).to(dev), 'S1': p['S1'].to(dev), 'S2': p['S2'].to(dev), 'W': p['wildcard_mat'].to(dev),
             'C': p['C_output_mat'].to(dev), 'h0': p['h0'].to(dev), 'hT': p['hT'].to(dev)}
        w.update({n: p[n].to(dev).contiguous() for n in gate_names})
        P = p['priority_mat'].to(dev) if prio else None
        trd = p['crf.transitions'].to(dev) if crf else None
        tc = _lib.TrainContext(V, S, R, K, nl=nl, threshold=0.5, o_idx=0, use_crf=crf, farnn=farnn, sigmoid_exponent=2.0)
        out = {'d' + n: torch.full_like(t, 7.0) for n, t in w.items()}       # the library must zero them itself
        dtr = torch.empty_like(trd) if crf else None
        loss = torch.empty(1, device=dev)
        tags = torch.empty((B, L), dtype=torch.int32, device=dev)
        xd, ld, labd = xt.to(dev), lt.to(dev), lab.to(dev)
        tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None if P is None else P.data_ptr(),
                     crf_trans=None if trd is None else trd.data_ptr()),
                xd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, int(lengths.sum()),
                dict({n: t.data_ptr() for n, t in out.items()}, loss=loss.data_ptr(), tags=tags.data_ptr(),
                     dtrans=None if dtr is None else dtr.data_ptr()))
        torch.cuda.synchronize()
        # relu / relutanh have a kink at 0: a pre-activation within float noise of it flips a unit's derivative between
        # the two implementations (1 of 1200 configurations did), so those gradients get a coarser bar
        frac = 3e-2 if nl in ('relu', 'relutanh') else 2e-4
        tag = 'iteration {}: S={} R={} K={} V={} B={} L={} farnn={} crf={} nl={} prio={}'.format(it, S, R, K, V, B, L, farnn, crf, nl, prio)
        assert abs(float(loss) - float(loss_ref)) < 1e-4 * max(1.0, abs(float(loss_ref))), tag
        for n, key in (('S1', 'S1'), ('S2', 'S2'), ('W', 'wildcard_mat'), ('C', 'C_output_mat'), ('h0', 'h0'), ('hT', 'hT')) + \
                tuple((n, n) for n in gate_names):
            close(out['d' + n].cpu().numpy(), grads_ref[key].numpy().reshape(out['d' + n].shape), tag + ' d' + n, rtol=5e-3, frac=frac)
        if crf:
            close(dtr.cpu().numpy(), grads_ref['crf.transitions'].numpy(), tag + ' dtrans', rtol=5e-3, frac=frac)
        # dVgen under the gradient rule.  Its conditions on the two oracles (float32 within 1e-5 of float64 at the tensor's
        # scale, at most 1 % of the words beyond that at their own) fail for about one random configuration in twelve: a
        # relu kink within float noise, or a long CRF sequence.  That is decided from the oracles alone, before the
        # library's result is looked at; such a configuration keeps the comparisons above and is named at the end.
        ref32, ref64, present = dvgen_refs(p, x, lengths, labels, nl, farnn, 2.0, prio)
        try:
            assert_grad_path(ref32, ref32, ref64, slices=0, present=present)
        except AssertionError as e:
            badly_drawn.append('{}: {}'.format(tag, e))
        else:
            check_grad('soak ' + tag, 'dVgen', out['dVgen'].cpu().numpy(), ref32, ref64, slices=0, present=present)
        tc.close()
    print('soak: dVgen not held to the gradient rule in {} of {} configurations (badly drawn oracles): {}'.format(
        len(badly_drawn), iters, badly_drawn))
    assert len(badly_drawn) <= max(1, iters // 4), badly_drawn   # the soak must not quietly stop checking dVgen this way


@pytest.mark.parametrize('mode', ['1', '2', '1n4'])
@pytest.mark.parametrize('k', [0, 6, 8, 9])
def test_train_step_through_l2_kernels_match_reference(k, mode, monkeypatch):
    """The chain kernels that read their matrices through L2 (what large ranks use): FARNN_TRAIN_NOLDS=1 keeps the
    S x S matrices that fit in LDS, =2 none; 'n4' forces four sequences per workgroup (what batches of 512+ sequences
    use).  Same fixtures, same bar."""
    monkeypatch.setenv('FARNN_TRAIN_NOLDS', mode[0])
    if mode.endswith('n4'):
        monkeypatch.setenv('FARNN_TRAIN_NSEQ', '4')
    test_train_step_matches_reference_loss_and_gradients(k)


@pytest.mark.parametrize('R', [250, 300])
def test_train_step_rank_250_gated_crf_vs_batched_oracle(R):
    """The shipped configurations' shape (rank 250, gates, CRF) on a small batch: the instantiation bench.py times;
    rank 300 needs two rank slots per thread (2 R > 512 threads) but one state slot."""
    from re2nn_seq_amd import _lib
    rng = np.random.RandomState(R)
    V, S, K, B, L, D, farnn = 120, 104, 75, 6, 17, 8, 2
    f = lambda *shape, sc=0.3: torch.from_numpy((rng.randn(*shape) * sc).astype(np.float32))   # noqa: E731
    Cm = np.zeros((K, S), np.float32)
    Cm[rng.randint(0, K - 2, size=S), np.arange(S)] = (rng.rand(S) < 0.8)
    fs = 0.7 / np.sqrt(R)
    p = {'S1': f(S, R, sc=fs), 'S2': f(S, R, sc=fs), 'V_embed': f(V, R, sc=0.8), 'embed_r_generalized': f(D, R),
         'C_output_mat': torch.from_numpy(Cm + (rng.rand(K, S) * 0.02).astype(np.float32)),
         'wildcard_mat': torch.from_numpy(((rng.rand(S, S) < 1.0 / S) * 0.5).astype(np.float32)),
         'h0': f(S, sc=0.5), 'hT': f(S, sc=0.5), 'beta_vec': torch.full((R,), 0.7), 'embedding.weight': f(V, D),
         'priority_mat': torch.eye(K)}
    gate_names = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')
    for n in gate_names:
        p[n] = f(1, S, sc=0.5) if n.startswith('bs') else (f(S, S, sc=0.5 / np.sqrt(S)) if n.startswith('Wss') else f(R, S, sc=0.5 / np.sqrt(R)))
    tr = (rng.randn(K, K) * 0.3).astype(np.float32)
    tr[:, K - 2] = -10000.0
    tr[K - 1, :] = -10000.0
    p['crf.transitions'] = torch.from_numpy(tr)
    lengths = rng.randint(1, L + 1, size=B).astype(np.int64)
    lengths[0] = L
    x = rng.randint(0, V, size=(B, L)).astype(np.int64)
    labels = rng.randint(0, K - 2, size=(B, L)).astype(np.int64)
    xt, lt, lab = torch.from_numpy(x), torch.from_numpy(lengths), torch.from_numpy(labels)
    loss_ref, grads_ref, _ = to.train_step_batched(p, xt, lt, lab, nl='tanh', farnn=farnn, sig_k=3.0)
    dev = torch.device('cuda')
    w = {'Vgen': to.generalized_table(p).to(dev), 'S1': p['S1'].to(dev), 'S2': p['S2'].to(dev), 'W': p['wildcard_mat'].to(dev),
         'C': p['C_output_mat'].to(dev), 'h0': p['h0'].to(dev), 'hT': p['hT'].to(dev)}
    w.update({n: p[n].to(dev).contiguous() for n in gate_names})
    trd = p['crf.transitions'].to(dev)
    tc = _lib.TrainContext(V, S, R, K, nl='tanh', threshold=0.5, o_idx=1, use_crf=True, farnn=farnn, sigmoid_exponent=3.0)
    out = {'d' + n: torch.full_like(t, 7.0) for n, t in w.items()}           # the library must zero them itself
    dtr = torch.empty_like(trd)
    loss = torch.empty(1, device=dev)
    tags = torch.empty((B, L), dtype=torch.int32, device=dev)
    xd, ld, labd = xt.to(dev), lt.to(dev), lab.to(dev)
    tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None, crf_trans=trd.data_ptr()),
            xd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, int(lengths.sum()),
            dict({n: t.data_ptr() for n, t in out.items()}, loss=loss.data_ptr(), tags=tags.data_ptr(), dtrans=dtr.data_ptr()))
    torch.cuda.synchronize()
    assert abs(float(loss) - float(loss_ref)) < 1e-4 * max(1.0, abs(float(loss_ref)))
    for n, key in (('S1', 'S1'), ('S2', 'S2'), ('W', 'wildcard_mat'), ('C', 'C_output_mat'), ('h0', 'h0'), ('hT', 'hT')) + \
            tuple((n, n) for n in gate_names):
        close(out['d' + n].cpu().numpy(), grads_ref[key].numpy().reshape(out['d' + n].shape), 'd' + n, rtol=5e-3)
    close(dtr.cpu().numpy(), grads_ref['crf.transitions'].numpy(), 'dtrans', rtol=5e-3)
    check_dvgen('rank-{} farnn2 crf'.format(R), out['dVgen'].cpu().numpy(), p, x, lengths, labels, 'tanh', farnn, 3.0)
    tc.close()


def test_train_step_reports_out_of_range_labels_and_crf_size_limits():
    """a label outside 0..K-1 at a valid position is counted as label 0 in loss AND gradient (they stay
    consistent) and the NEXT call returns FARNN_EINVAL (torch's CrossEntropyLoss raises on such a target); a CRF tag
    set that cannot fit the LDS is refused before anything is enqueued."""
    from re2nn_seq_amd import _lib
    rng = np.random.RandomState(3)
    V, S, R, K, B, L = 30, 12, 6, 7, 4, 5
    dev = torch.device('cuda')
    f = lambda *shape: torch.from_numpy((rng.randn(*shape) * 0.3).astype(np.float32)).to(dev)   # noqa: E731
    w = {'Vgen': f(V, R), 'S1': f(S, R), 'S2': f(S, R), 'W': f(S, S), 'C': f(K, S), 'h0': f(S), 'hT': f(S)}
    out = {'d' + n: torch.zeros_like(t) for n, t in w.items()}
    loss = torch.zeros(1, device=dev)
    tags = torch.empty((B, L), dtype=torch.int32, device=dev)
    x = torch.from_numpy(rng.randint(0, V, size=(B, L))).to(dev)
    lengths = torch.tensor([5, 3, 1, 4], device=dev)
    good = torch.from_numpy(rng.randint(0, K, size=(B, L))).to(dev)
    bad = good.clone(); bad[1, 1] = K + 3
    zero = good.clone(); zero[1, 1] = 0
    padbad = good.clone(); padbad[1, 4] = -5            # a pad position: never read
    tc = _lib.TrainContext(V, S, R, K, nl='tanh')

    def step(lab):
        tc.step({n: t.data_ptr() for n, t in w.items()}, x.data_ptr(), lengths.data_ptr(), lab.data_ptr(), B, L, 13,
                dict({n: t.data_ptr() for n, t in out.items()}, loss=loss.data_ptr(), tags=tags.data_ptr()))
        torch.cuda.synchronize()
        return float(loss), {n: t.clone() for n, t in out.items()}

    l0, g0 = step(zero)
    step(padbad)                                        # fine: the next call does not raise
    l1, g1 = step(bad)
    # counted as label 0, consistently in the loss and in every gradient (equal up to the order of the float atomics)
    assert abs(l1 - l0) < 1e-5 * abs(l0)
    assert all(torch.allclose(g0[n], g1[n], rtol=1e-4, atol=1e-6) for n in g0)
    with pytest.raises(_lib.FarnnError, match='label outside'):
        step(good)
    step(good)                                          # the flag is reported once
    tc.close()
    # CRF size limits: K = 200 cannot keep exp(transitions) in LDS at all; K = 150 fails at L = 64 only
    with pytest.raises(_lib.FarnnError, match='4..190'):
        _lib.TrainContext(V, S, R, 200, nl='tanh', use_crf=True)
    tc = _lib.TrainContext(V, S, R, 150, nl='tanh', use_crf=True)
    w['C'] = f(150, S); out['dC'] = torch.zeros_like(w['C'])
    tr = f(150, 150); dtr = torch.zeros_like(tr)
    x64 = torch.from_numpy(rng.randint(0, V, size=(B, 64))).to(dev)
    lab64 = torch.zeros((B, 64), dtype=torch.int64, device=dev)
    with pytest.raises(_lib.FarnnError, match='too large'):
        tc.step(dict({n: t.data_ptr() for n, t in w.items()}, crf_trans=tr.data_ptr()), x64.data_ptr(), lengths.data_ptr(),
                lab64.data_ptr(), B, 64, 13, dict({n: t.data_ptr() for n, t in out.items()}, loss=loss.data_ptr(),
                                                  tags=tags.data_ptr(), dtrans=dtr.data_ptr()))
    tc.close()
