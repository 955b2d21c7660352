"""farnn_decomp_sf_train_step (the training step of the vector-input tagger FARNN_S_SF) on the GPU: the loss,
the tags, every weight gradient and d loss / d v against the training oracle (tests/sf_train_ref.py), the promises about the pad
rows and about reproducibility, consistency with the id step and with farnn_tag_vectors, every refusal, and the Python surface."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sf_train_ref as sr  # noqa: E402
from oracle import farnn_train_oracle as to  # noqa: E402
from util import check_grad, ns  # noqa: E402

pytestmark = pytest.mark.gpu
THRESHOLD, O_IDX = 0.5, 1
FILL = 7.0


def dev():
    return torch.device('cuda', 0)


def weights_on_device(p, case):
    w = {n: p[sr.ORACLE_KEY[n]].to(dev()).contiguous() for n in sr.grad_names(case)}
    if case['prio']:
        w['P'] = p['priority_mat'].to(dev()).contiguous()
    return w


def context(case, K):
    from re2nn_seq_amd import _lib
    return _lib.SfTrainContext(case['S'], case['R'], K, nl=case['nl'], threshold=THRESHOLD, o_idx=O_IDX, use_crf=case['crf'],
                               farnn=case['farnn'], sigmoid_exponent=sr.SIG_K)


def run_step(tc, w, case, v, lengths, labels, calls=1):
    """`calls` library steps on pre-filled outputs; returns (loss, {name: gradient, 'v': dv}, tags) as numpy."""
    B, L, R = v.shape
    vd = torch.from_numpy(np.ascontiguousarray(v)).to(dev())
    ld, labd = torch.from_numpy(np.asarray(lengths)).to(dev()), torch.from_numpy(labels).to(dev())
    out = {n: torch.full_like(w[n], FILL) for n in sr.grad_names(case)}
    # the pattern dv is handed over with: nothing the step could leave behind by accident, and no zero
    dv = (torch.arange(B * L * R, device=dev(), dtype=torch.float32).reshape(B, L, R) % 13) + 1.0
    loss = torch.full((1,), 3.0, device=dev())
    tags = torch.full((B, L), 99, dtype=torch.int32, device=dev())
    outputs = {('dtrans' if n == 'crf_trans' else 'd' + n): t.data_ptr() for n, t in out.items()}
    outputs.update(loss=loss.data_ptr(), tags=tags.data_ptr())
    for _ in range(calls):
        tc.step_vectors({n: t.data_ptr() for n, t in w.items()}, vd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L,
                        int(np.clip(lengths, 0, L).sum()), outputs, dv.data_ptr())
    torch.cuda.synchronize()
    got = {n: t.cpu().numpy() for n, t in out.items()}
    got['v'] = dv.cpu().numpy()
    return float(loss), got, tags.cpu().numpy()


@pytest.mark.parametrize('name', sr.CASE_IDS)
def test_step_against_the_oracle(name):
    """Loss, all weight gradients, the gates' gradients, dtrans and dv under check_grad (exact zeros at the pad rows of the
    pre-filled dv); the tags against farnn_tag_vectors' on the same weights wherever the float64 scores decide the position;
    further calls give the same bits in every output."""
    from re2nn_seq_amd import _lib
    case = sr.by_name(name)
    p, v, lengths, labels, ref32, ref64 = sr.refs(name)
    B, L, R = v.shape
    K = p['C_output_mat'].shape[0]
    w = weights_on_device(p, case)
    tc = context(case, K)
    loss, got, tags = run_step(tc, w, case, v, lengths, labels)
    sr.check_all(case, loss, got, ref32, ref64, lengths, check_grad)
    loss2, got2, tags2 = run_step(tc, w, case, v, lengths, labels, calls=2)
    assert np.float32(loss).tobytes() == np.float32(loss2).tobytes(), 'the loss differs between calls'
    for n in got:
        assert np.array_equal(got[n].view(np.uint32), got2[n].view(np.uint32)), 'd{} differs between calls'.format(n)
    assert np.array_equal(tags, tags2)
    mask = sr.valid_mask(lengths, L)
    assert (tags[~mask] == -1).all()
    # the tags: those of the tagging handle on the same weights and vectors, where the decode is determined
    tr = p['crf.transitions'].numpy() if case['crf'] else None
    decided = sr.decided_tags(ref64[2], lengths, L, THRESHOLD, tr)
    gates = {k: (p[k].reshape(-1) if k.startswith('bs') else p[k]).numpy() for k in sr.GATE_NAMES if k in p}
    h = _lib.create_decomp_sf(p['S1'].numpy(), p['S2'].numpy(), p['wildcard_mat'].numpy(), p['C_output_mat'].numpy(), p['h0'].numpy(),
                              p['hT'].numpy(), P=p['priority_mat'].numpy() if case['prio'] else None, farnn=case['farnn'], gates=gates,
                              sigmoid_exponent=sr.SIG_K, nl=case['nl'], semiring='sum', threshold=THRESHOLD, o_idx=O_IDX,
                              use_crf=case['crf'], crf_trans=tr, device=0)
    vd, ld = torch.from_numpy(v).to(dev()), torch.from_numpy(lengths).to(dev())
    ttags = torch.empty((B, L), dtype=torch.int32, device=dev())
    h.tag_vectors(vd.data_ptr(), ld.data_ptr(), B, L, _lib.MODE_LOCAL, ttags.data_ptr(), None, None,
                  torch.cuda.current_stream(dev()).cuda_stream)
    torch.cuda.synchronize()
    h.close()
    assert decided[mask].mean() >= 0.5                                    # (tests/test_sf_train_cpu.py holds every case to it)
    assert np.array_equal(tags[decided], ttags.cpu().numpy()[decided])
    tc.close()


@pytest.mark.parametrize('poison', [np.nan, np.inf])
@pytest.mark.parametrize('name', ['S9R7-B3L2-f1-tanh-P', 'S40R33-B5L9-f0-none-crf', 'S70R70-B5L9-f1-relutanh-crf',
                                  'S33R130-B5L9-f2-relutanh-crf', 'S33R130-B5L2-f1-tanh-P', 'S70R70-B5L2-f0-relutanh-P'])
def test_pad_rows_of_v_are_never_read(name, poison):
    """NaN (and separately Inf) in every pad row of v: every output is finite and bit-identical to the run with zeros there."""
    case = sr.by_name(name)
    p, v, lengths, labels, _, _ = sr.refs(name)
    B, L, R = v.shape
    mask = sr.valid_mask(lengths, L)
    assert (~mask).any()
    clean, bad = v.copy(), v.copy()
    clean[~mask] = 0.0
    bad[~mask] = poison
    w = weights_on_device(p, case)
    tc = context(case, p['C_output_mat'].shape[0])
    l0, g0, t0 = run_step(tc, w, case, clean, lengths, labels)
    l1, g1, t1 = run_step(tc, w, case, bad, lengths, labels)
    assert np.isfinite(l1) and np.float32(l0).tobytes() == np.float32(l1).tobytes()
    assert np.array_equal(t0, t1)
    for n in g0:
        assert np.isfinite(g1[n]).all(), n
        assert np.array_equal(g0[n].view(np.uint32), g1[n].view(np.uint32)), n
    assert not g1['v'][~mask].any()
    tc.close()


@pytest.mark.parametrize('name', ['S40R33-B5L9-f0-none-crf', 'S9R7-B5L9-f2-relutanh', 'S33R130-B5L2-f1-tanh-P'])
def test_consistent_with_the_id_step(name):
    """A batch whose vectors are rows of a table Vgen: the dv rows scatter-added by word id, and the id step's dVgen, both under
    check_grad against the same oracle (train_step on that table and those ids)."""
    from re2nn_seq_amd import _lib
    case = sr.by_name(name)
    p, _, lengths, labels, _, _ = sr.refs(name)
    B, L, S, R = case['B'], case['L'], case['S'], case['R']
    K = p['C_output_mat'].shape[0]
    V = 6                                                        # fewer words than positions: words repeat within and across sequences
    rng = np.random.RandomState(case['seed'] + 7)
    table = (rng.randn(V, R) * 0.8).astype(np.float32)
    x = rng.randint(0, V, size=(B, L)).astype(np.int64)
    v = table[x]
    ref = []
    for dtype in (torch.float32, torch.float64):
        q = {k: t.to(dtype) for k, t in p.items()}
        q.update({'V_embed': torch.from_numpy(table).to(dtype), 'beta_vec': torch.ones(R, dtype=dtype),
                  'embedding.weight': torch.zeros(V, 1, dtype=dtype), 'embed_r_generalized': torch.zeros(1, R, dtype=dtype)})
        _, g, _ = to.train_step(q, torch.from_numpy(x), torch.from_numpy(lengths), torch.from_numpy(labels), nl=case['nl'],
                                use_priority=case['prio'], farnn=case['farnn'], sig_k=sr.SIG_K)
        ref.append(g['V_embed'].numpy())
    mask = sr.valid_mask(lengths, L)
    present = np.zeros(V, bool)
    present[x[mask]] = True
    w = weights_on_device(p, case)
    tc = context(case, K)
    loss_sf, got, tags_sf = run_step(tc, w, case, v, lengths, labels)
    tc.close()
    scattered = np.zeros((V, R), np.float64)
    np.add.at(scattered, x[mask], got['v'][mask].astype(np.float64))
    check_grad(name, 'dv scattered by word', scattered, ref[0], ref[1], slices=0, present=present)
    # the id step on the same weights and that table
    ic = _lib.TrainContext(V, S, R, K, nl=case['nl'], threshold=THRESHOLD, o_idx=O_IDX, use_crf=case['crf'], farnn=case['farnn'],
                           sigmoid_exponent=sr.SIG_K)
    wi = dict(w, Vgen=torch.from_numpy(table).to(dev()))
    names = ('Vgen',) + sr.grad_names(case)
    out = {n: torch.full_like(wi[n], FILL) for n in names}
    loss = torch.full((1,), 3.0, device=dev())
    tags = torch.empty((B, L), dtype=torch.int32, device=dev())
    outputs = {('dtrans' if n == 'crf_trans' else 'd' + n): t.data_ptr() for n, t in out.items()}
    outputs.update(loss=loss.data_ptr(), tags=tags.data_ptr())
    xd, ld, labd = (torch.from_numpy(a).to(dev()) for a in (x, lengths, labels))
    ic.step({n: t.data_ptr() for n, t in wi.items()}, xd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, int(lengths.sum()), outputs)
    torch.cuda.synchronize()
    ic.close()
    check_grad(name, 'dVgen (id step)', out['Vgen'].cpu().numpy(), ref[0], ref[1], slices=0, present=present)
    assert abs(float(loss) - loss_sf) <= 1e-4 * (1.0 + abs(loss_sf))


def test_refusals_leave_the_outputs_untouched():
    """Every refusal of include/farnn.h for the vector-input step, each with pre-filled outputs that stay as they were."""
    from re2nn_seq_amd import _lib
    C = _lib.C
    case = sr.by_name('S9R7-B3L2-f1-tanh-P')
    p, v, lengths, labels, _, _ = sr.refs(case['name'])
    B, L, R = v.shape
    S, K = case['S'], p['C_output_mat'].shape[0]
    w = weights_on_device(p, case)
    vd, ld, labd = (torch.from_numpy(a).to(dev()) for a in (v, lengths, labels))
    names = sr.grad_names(case)
    out = {n: torch.full_like(w[n], FILL) for n in names}
    dv = torch.full((B, L, R), FILL, device=dev())
    dVgen = torch.full((B * L, R), FILL, device=dev())
    loss = torch.full((1,), FILL, device=dev())
    tags = torch.full((B, L), 99, dtype=torch.int32, device=dev())
    outputs = dict({'d' + n: t.data_ptr() for n, t in out.items()}, loss=loss.data_ptr(), tags=tags.data_ptr())
    wp = {n: t.data_ptr() for n, t in w.items()}
    ntok = int(lengths.sum())

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == FILL).all()) for t in list(out.values()) + [dv, dVgen, loss]) and bool((tags == 99).all())

    def refused(fn):
        with pytest.raises(_lib.FarnnError):
            fn()
        assert untouched()

    tc = context(case, K)
    refused(lambda: tc.set_semiring('max'))
    assert tc.semiring == 'sum'
    refused(lambda: tc.step(dict(wp, Vgen=vd.data_ptr()), labd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, ntok,
                            dict(outputs, dVgen=dVgen.data_ptr())))                           # the id entry
    re = torch.zeros((B, L, K), device=dev())
    for max_entry in (False, True):
        refused(lambda: tc.teacher_step(dict(wp, Vgen=vd.data_ptr()), labd.data_ptr(), ld.data_ptr(), labd.data_ptr(), re.data_ptr(), 'kd',
                                        1.0, 0.5, B, L, ntok, dict(outputs, dVgen=dVgen.data_ptr()), max_entry=max_entry))
    refused(lambda: tc.step_vectors(dict(wp, Vgen=vd.data_ptr()), vd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, ntok, outputs, dv.data_ptr()))
    refused(lambda: tc.step_vectors(wp, vd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, ntok, dict(outputs, dVgen=dVgen.data_ptr()),
                                    dv.data_ptr()))
    refused(lambda: tc.step_vectors(wp, None, ld.data_ptr(), labd.data_ptr(), B, L, ntok, outputs, dv.data_ptr()))
    refused(lambda: tc.step_vectors(wp, vd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, ntok, outputs, None))
    tc.step_vectors(wp, vd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, ntok, outputs, dv.data_ptr())     # and the context still works
    torch.cuda.synchronize()
    assert not untouched() and bool(torch.isfinite(dv).all())
    tc.close()
    # the vector entry on an id context
    for t in list(out.values()) + [dv, loss]:
        t.fill_(FILL)
    tags.fill_(99)
    ic = _lib.TrainContext(B * L, S, R, K, nl=case['nl'], threshold=THRESHOLD, o_idx=O_IDX, farnn=case['farnn'], sigmoid_exponent=sr.SIG_K)
    raw = ic._raw
    wst = _lib.TrainWeights(**{k: wp.get(k) for k, _ in _lib.TrainWeights._fields_})
    ost = _lib.TrainOutputs(**{k: outputs.get(k) for k, _ in _lib.TrainOutputs._fields_})
    rc = _lib.load().farnn_decomp_sf_train_step(raw, C.byref(wst), vd.data_ptr(), ld.data_ptr(), labd.data_ptr(), B, L, ntok, C.byref(ost),
                                                dv.data_ptr(), None)
    assert rc != 0 and untouched()
    ic.close()
    # creates: V = 0 stays refused by farnn_train_create, V != 0 by farnn_decomp_sf_train_create
    with pytest.raises(_lib.FarnnError):
        _lib.TrainContext(0, S, R, K)
    handle = C.c_void_p()
    dims = _lib.TrainDims(5, S, R, K, _lib.NL['none'], 0.5, 0, 0, 5.0, 0)
    assert _lib.load().farnn_decomp_sf_train_create(C.byref(dims), 0, C.byref(handle)) != 0 and not handle.value
    assert _lib.load().farnn_abi_version() == 2


class Encoder(torch.nn.Module):
    """a stand-in for the contextual encoder: token features [B, L, F] -> [B, L, D]"""
    def __init__(self, F, D):
        super().__init__()
        self.lin = torch.nn.Linear(F, D)

    def forward(self, bert_input, bert_attend_mask, bert_valid_mask, lengths):
        return torch.tanh(self.lin(bert_input))


def bert_model(monkeypatch, farnn, use_crf):
    import json
    from re2nn_seq_amd.farnn.model_decompose_single import FARNN_S_bert
    monkeypatch.setenv('RE2NN_SF_TRAIN', '1')
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'decomp_small.npz'))
    with open(os.path.join(ROOT, 'tests', 'golden', 'decomp_small.json')) as f:
        meta = json.load(f)
    torch.manual_seed(3)
    F, D = 5, g['E_in'].shape[1]
    enc = Encoder(F, D).to(dev())
    a = ns(independent=2, threshold=meta['threshold'], farnn=farnn, use_crf=use_crf, update_nonlinear='tanh', beta=0.6, xavier=1,
           bias_init=0.2, sigmoid_exponent=1, train_h0=1, train_hT=1, train_wildcard=1)
    m = FARNN_S_bert(V=g['V_in'], S1=g['S1_in'], S2=g['S2_in'], C_output_mat=g['O_in'], wildcard_mat=g['W_in'],
                     wildcard_output_vector=g['Ow_in'], final_vector=g['final_in'], start_vector=g['start_in'], static_embed=g['E_in'],
                     priority_mat=g['priority_in'], args=a, o_idx=meta['o_idx'], encoder=enc)
    m.embed.to(dev()).requires_grad_()
    x = torch.from_numpy(g['x'])
    lengths = torch.from_numpy(g['lengths'])
    B, L = x.shape
    feats = torch.randn(B, int(lengths.max()), F, device=dev())      # what an encoder returns: one vector per token of the longest sequence
    labels = torch.randint(0, g['O_in'].shape[0], (B, L))
    return m, a, x, feats, lengths, labels


@pytest.mark.parametrize('farnn,use_crf', [(0, 0), (2, 1)])
def test_python_surface_end_to_end(monkeypatch, farnn, use_crf):
    """FARNN_S_bert with a torch.nn.Linear-based encoder on the device, train=True under the switch, loss.backward(): the
    encoder's weight gradient and embed_r_generalized.grad against the same model evaluated wholly in torch on the CPU (the
    oracle's chain on top of the aggregator), by check_grad."""
    m, a, x, feats, lengths, labels = bert_model(monkeypatch, farnn, use_crf)
    loss, pred, true = m(x, feats, None, None, lengths, labels, train=True)
    assert pred.shape == true.shape == (int(lengths.sum()),)
    loss.backward()
    sf, agg, enc = m.slot_filler, m.embed, m.embed.encoder
    got = {'lin.weight': enc.lin.weight.grad.cpu().numpy(), 'embed_r_generalized': agg.embed_r_generalized.grad.cpu().numpy()}
    assert agg.V_embed.grad is None and agg.beta_vec.grad is None                      # train_V_embed = train_beta = 0
    named = dict(sf.named_parameters())
    assert all(t.grad is not None for t in named.values()) and {'S1', 'S2', 'h0', 'hT', 'wildcard_mat', 'C_output_mat'} <= set(named)
    Lmax = int(lengths.max())
    ref = []
    for dtype in (torch.float32, torch.float64):
        W = enc.lin.weight.detach().cpu().to(dtype).requires_grad_(True)
        G = agg.embed_r_generalized.detach().cpu().to(dtype).requires_grad_(True)
        emb = torch.tanh(feats.cpu().to(dtype) @ W.T + enc.lin.bias.detach().cpu().to(dtype))[:, :Lmax]
        xi = x[:, :Lmax]
        beta = agg.beta_vec.detach().cpu().to(dtype)
        v = agg.V_embed.detach().cpu().to(dtype)[xi] * beta + (emb @ G) * (1 - beta)
        B, L, R = v.shape
        tp = {k: t.detach().cpu().to(dtype) for k, t in sf._tp.items()}
        gates = {k: tp[k] for k in sr.GATE_NAMES if k in tp}
        s = to.chain_scores(v.reshape(B * L, R), tp['S1'], tp['S2'], tp['wildcard_mat'], tp['C_output_mat'], tp['h0'], tp['hT'],
                            torch.arange(B * L).reshape(B, L), lengths, a.update_nonlinear, None, gates=gates, farnn=farnn,
                            sig_k=float(a.sigmoid_exponent))
        if use_crf:
            ref_loss = to.crf_nll(s, lengths, labels[:, :Lmax], tp['crf.transitions'])
        else:
            ref_loss = torch.nn.functional.cross_entropy(s, torch.cat([labels[b, :int(lengths[b])] for b in range(B)]))
        ref_loss.backward()
        ref.append({'lin.weight': W.grad.numpy(), 'embed_r_generalized': G.grad.numpy(), 'loss': float(ref_loss.detach())})
    assert abs(float(loss.detach()) - ref[1]['loss']) <= 1e-4 * (1 + abs(ref[1]['loss']))
    for n in got:
        check_grad('bert-f{}-crf{}'.format(farnn, use_crf), n, got[n], ref[0][n], ref[1][n])


def test_three_adam_steps_reduce_the_loss(monkeypatch):
    """A fixed tiny batch, the aggregator's leaves, the encoder and the automaton under one optimizer; eval() afterwards tags
    with the trained weights."""
    m, a, x, feats, lengths, labels = bert_model(monkeypatch, 1, 0)
    m.slot_filler.enable_training()
    opt = torch.optim.Adam(list(m.parameters()), lr=0.02)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss, _, _ = m(x, feats, None, None, lengths, labels, train=True)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    assert all(np.isfinite(losses)) and losses[3] < losses[0], losses
    m.slot_filler.eval()
    with torch.no_grad():
        none, pred, true = m(x, feats, None, None, lengths, labels, train=False)
    assert none is None and pred.shape == true.shape
