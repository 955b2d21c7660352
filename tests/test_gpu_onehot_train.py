"""The HIP training step of the onehot i-FST (FARNN_S_O_I_S) against the loss / gradient /
predictions captured from the reference's forward_local(train=True) + loss.backward(), against the torch restatement
(tests/onehot_train_ref.py) at the headline shape and at larger state counts, and through the command line."""
import os

import numpy as np
import pytest
import torch

import onehot_train_ref as otr
from test_onehot_train_cpu import N_CASES, case
from util import GOLDEN, assert_float_path, check_grad, ns, present_words

pytestmark = pytest.mark.gpu


def _model(inp, cfg_nl, up, threshold):
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I_S
    S = inp['T'].shape[1]
    pri = inp['P'][:-1, :-1] if up else np.eye(inp['O'].shape[0] - 1)
    a = ns(update_nonlinear=cfg_nl, use_priority=up, threshold=threshold)
    return FARNN_S_O_I_S(inp['T'], inp['O'], inp['W'], np.zeros(S), inp['hT'], inp['h0'], pri, a, o_idx=inp['o_idx'])


@pytest.mark.parametrize('k', range(N_CASES))
def test_model_mirror_matches_the_reference_capture(k):
    cfg, inp, ref = case(k)
    m = _model(inp, cfg['update_nonlinear'], cfg['use_priority'], inp['threshold'])
    x, lt, lab = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths']), torch.from_numpy(inp['labels'])
    m.train()
    loss, pred, true = m.forward_local(x, lab, lt, train=True)
    loss.backward()
    named = dict(m.named_parameters())
    assert set(named) == {'language_tensor'}
    l64, g64, _ = otr.step(dtype=torch.float64, **inp)
    assert_float_path(float(loss.detach()), ref['loss'], l64, err_msg='loss')
    assert_float_path(named['language_tensor'].grad.cpu().numpy(), ref['dT'], g64, err_msg='dT')
    assert np.array_equal(pred.cpu().numpy(), ref['flat_pred'])
    assert true.shape == pred.shape


def _run_step(T, W, O, h0, hT, P, x, lengths, labels, nl='none', threshold=0.5, o_idx=0, tc=None):
    from re2nn_seq_amd import _lib
    from re2nn_seq_amd.farnn.train_step import onehot_ifst_train_step
    dev = torch.device('cuda', 0)
    V, S, _ = T.shape
    if tc is None:
        tc = _lib.OnehotTrainContext(V, S, O.shape[0], nl=nl, threshold=threshold, o_idx=o_idx, device=0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    Tt = d(T).requires_grad_(True)
    loss, tags = onehot_ifst_train_step(tc, Tt, d(W), d(O), d(h0), d(hT), None if P is None else d(P),
                                        torch.from_numpy(x), torch.from_numpy(lengths), torch.from_numpy(labels))
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), Tt.grad.cpu().numpy(), tags.cpu().numpy(), tc


def run_step_c_abi(c, nl='none'):
    """farnn_onehot_ifst_train_step called directly on pre-filled outputs (the autograd wrapper of _run_step allocates dT
    with torch.empty_like, which says nothing about entries the library leaves alone); returns (loss, dT)"""
    from re2nn_seq_amd import _lib
    dev = torch.device('cuda', 0)
    V, S, _ = c['T'].shape
    tc = _lib.OnehotTrainContext(V, S, c['O'].shape[0], nl=nl, threshold=0.5, o_idx=0, device=0)
    try:
        w = {n: torch.from_numpy(np.ascontiguousarray(c[n], dtype=np.float32)).to(dev) for n in ('T', 'W', 'O', 'h0', 'hT')}
        P = None if c['P'] is None else torch.from_numpy(np.ascontiguousarray(c['P'], dtype=np.float32)).to(dev)
        x, lengths, labels = (torch.from_numpy(np.ascontiguousarray(c[n])).to(dev) for n in ('x', 'lengths', 'labels'))
        B, L = c['x'].shape
        dT = torch.full_like(w['T'], 7.0)                    # the library must zero it itself
        loss = torch.full((1,), 3.0, device=dev)
        tags = torch.empty((B, L), dtype=torch.int32, device=dev)
        tc.step(dict({n: t.data_ptr() for n, t in w.items()}, P=None if P is None else P.data_ptr()), x.data_ptr(),
                lengths.data_ptr(), labels.data_ptr(), B, L, int(np.clip(c['lengths'], 0, L).sum()),
                dict(loss=loss.data_ptr(), dT=dT.data_ptr(), tags=tags.data_ptr()))
        torch.cuda.synchronize()
        return float(loss), dT.cpu().numpy()
    finally:
        tc.close()


def _random_case(V, S, C, B, L, seed, priority=False):
    from re2nn_seq_amd import synth
    rng = np.random.RandomState(seed)
    T, W, O, h0, hT = synth.random_ifst_tensors(V, S, C, rng)
    x, lengths = synth.random_batch(V, B, L, rng)
    labels = rng.randint(0, C, size=(B, L)).astype(np.int64)
    P = None
    if priority:
        P = np.eye(C, dtype=np.float32)
        P[rng.randint(0, C, 8), rng.randint(0, C, 8)] = -1.0
    return dict(T=T, W=W, O=O, h0=h0, hT=hT, P=P, x=x, lengths=lengths, labels=labels)


def _check_against_restatement(c, nl='none', case='onehot'):
    """loss and dT by the ONE rule through the autograd wrapper; dT also by the gradient rule (tests/util.py:assert_grad_path)
    through the C-ABI on a pre-filled buffer: at the tensor's own scale, block by block at each present word's scale,
    exactly zero for the words that occur at no valid position"""
    loss, dT, _, tc = _run_step(nl=nl, **c)
    tc.close()
    l32, g32, _ = otr.step(dtype=torch.float32, nl=nl, **c)
    l64, g64, _ = otr.step(dtype=torch.float64, nl=nl, **c)
    assert_float_path(loss, l32, l64, err_msg='loss')
    assert_float_path(dT, g32, g64, err_msg='dT')
    loss2, dT2 = run_step_c_abi(c, nl)
    assert_float_path(loss2, l32, l64, err_msg='loss (C-ABI)')
    check_grad(case, 'dT', dT2, g32, g64, slices=0, present=present_words(c['x'], c['lengths'], dT2.shape[0]))


def test_headline_shape_against_the_restatement():
    """V = 950, S = 71, C = 128, B = 256, L = 64 with ragged lengths and one full-length row (bench.py's ifst shape)."""
    c = _random_case(950, 71, 128, 256, 64, seed=11)
    assert c['lengths'].max() == 64 and c['lengths'].min() < 64
    _check_against_restatement(c, case='onehot headline')


@pytest.mark.parametrize('S,B,L,nl,up', [(104, 64, 40, 'tanh', True), (104, 7, 9, 'relu', False),
                                         (128, 48, 33, 'none', False), (128, 3, 70, 'relutanh', True),
                                         (14, 5, 1, 'none', False), (64, 17, 12, 'tanh', False)])
def test_other_state_counts_and_geometries(S, B, L, nl, up):
    c = _random_case(300, S, 20, B, L, seed=S + B + L, priority=up)
    _check_against_restatement(c, nl=nl, case='onehot S{} B{} L{} {}'.format(S, B, L, nl))


def test_two_steps_are_bit_identical():
    c = _random_case(950, 71, 128, 256, 64, seed=12)
    l1, g1, t1, tc = _run_step(**c)
    l2, g2, t2, _ = _run_step(tc=tc, **c)
    assert l1 == l2 and np.array_equal(g1, g2) and np.array_equal(t1, t2)


def test_an_empty_sequence_changes_nothing():
    c = _random_case(200, 40, 12, 9, 15, seed=13)
    l1, g1, _, _ = _run_step(**c)
    e = dict(c)
    e['x'] = np.concatenate([c['x'][:4], np.full((1, 15), 199), c['x'][4:]])
    e['lengths'] = np.concatenate([c['lengths'][:4], [0], c['lengths'][4:]])
    e['labels'] = np.concatenate([c['labels'][:4], np.zeros((1, 15), np.int64), c['labels'][4:]])
    l2, g2, t2, _ = _run_step(**e)
    assert l1 == l2 and np.array_equal(g1, g2)
    assert (t2[4] == -1).all()


@pytest.mark.parametrize('k', [0, 1, 2, 3, 4, 5, 6, 7])
def test_train_tags_equal_the_tagging_path(k):
    """on the 0/1 ifst_small configurations: the train step's decode == forward_local(train=False) on the same weights"""
    cfg, inp, _ = case(k)
    assert cfg['base'] == 'ifst_small'
    m = _model(inp, cfg['update_nonlinear'], cfg['use_priority'], inp['threshold'])
    x, lt, lab = torch.from_numpy(inp['x']), torch.from_numpy(inp['lengths']), torch.from_numpy(inp['labels'])
    _, tag_pred, _ = m.forward_local(x, lab, lt, train=False)
    _, train_pred, _ = m.forward_local(x, lab, lt, train=True)
    assert np.array_equal(train_pred.cpu().numpy(), tag_pred.cpu().numpy())


def _synthetic_automaton(seed=4):
    from re2nn_seq_amd import synth
    dset, automaton = synth.make_dataset(60, 4, 20, seed)[:2]
    return dset, automaton


def test_edge_built_and_dense_models_train_alike():
    """bit-identical gradients from the edge-built and the dense-built model; three Adam steps match the restatement's,
    and the tagging that follows reads the trained weights."""
    from re2nn_seq_amd import synth
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I_S
    from re2nn_seq_amd.wfa import fsa_to_tensor as f2t
    dset, automaton = _synthetic_automaton()
    t2i = dict(dset['t2i']); t2i['<pad>'] = len(t2i)
    s2i = dset['s2i']
    V = len(t2i)
    a = ns(update_nonlinear='tanh')
    me = FARNN_S_O_I_S.from_automaton(automaton, t2i, s2i, None, a, o_idx=s2i['o'])
    T, _, W, O, Ow, fin, sta, _ = f2t.dfa_to_tensor_slot_single_wildcard(automaton, t2i, s2i)
    md = FARNN_S_O_I_S(T, O, W, Ow, fin, sta, None, a, o_idx=s2i['o'])
    rng = np.random.RandomState(3)
    batches = []
    for _ in range(3):
        x, lengths = synth.random_batch(V, 8, 10, rng, min_len=2)
        batches.append((x, lengths, rng.randint(0, O.shape[0], size=x.shape).astype(np.int64)))
    grads = []
    for m in (me, md):
        m.enable_training()
        x, lengths, labels = batches[0]
        loss, _, _ = m.forward_local(torch.from_numpy(x), torch.from_numpy(labels), torch.from_numpy(lengths))
        loss.backward()
        grads.append(dict(m.named_parameters())['language_tensor'].grad.cpu().numpy())
    assert np.array_equal(grads[0], grads[1])
    sd0 = md.state_dict()
    opt = torch.optim.Adam(list(me.parameters()), lr=0.05, weight_decay=0)
    for x, lengths, labels in batches:
        opt.zero_grad()
        loss, _, _ = me.forward_local(torch.from_numpy(x), torch.from_numpy(labels), torch.from_numpy(lengths))
        loss.backward()
        opt.step()
    me.eval()
    assert getattr(me, 'edges', None) is None
    got = me.state_dict()['language_tensor']
    kw = dict(W=sd0['wildcard_mat'], O=sd0['output_mat'], h0=sd0['h0'], hT=sd0['hT'], P=None, batches=batches,
              nl='tanh', lr=0.05)
    r32 = otr.adam_steps(sd0['language_tensor'], dtype=torch.float32, **kw)
    r64 = otr.adam_steps(sd0['language_tensor'], dtype=torch.float64, **kw)
    assert_float_path(got, r32, r64, err_msg='language_tensor after 3 Adam steps')
    # tagging with train=False now uses the trained weights: the same tags as a fresh model built from them
    x, lengths, labels = batches[0]
    _, p1, _ = me.forward_local(torch.from_numpy(x), torch.from_numpy(labels), torch.from_numpy(lengths), train=False)
    fresh = FARNN_S_O_I_S(got, O, W, Ow, fin, sta, None, a, o_idx=s2i['o'])
    _, p2, _ = fresh.forward_local(torch.from_numpy(x), torch.from_numpy(labels), torch.from_numpy(lengths), train=False)
    assert np.array_equal(p1.numpy(), p2.numpy())


def test_onehot_cli_trains_for_two_epochs(tmp_path):
    """--method onehot --independent 2 --epoch 2: the reference's epoch loop (train_onehot.py:156-206) on the HIP step"""
    from re2nn_seq_amd import main as cli
    from re2nn_seq_amd import synth
    tree = synth.write_dataset_tree(str(tmp_path / 'data'), dataset='ATIS-BIO', seed=4)
    argv = ['--dataset', 'ATIS-BIO', '--method', 'onehot', '--independent', '2',
            '--automata_path', tree['paths']['ID2'], '--normalize_automata', 'none', '--rand_constant', '0',
            '--update_nonlinear', 'tanh', '--bz', '9', '--seq_max_len', '12', '--epoch', '2', '--lr', '0.01',
            '--train_portion', '1.0', '--data_dir', tree['paths']['data_dir'], '--model_dir', str(tmp_path / 'm')]
    results, stats, res_path = cli.main(argv)
    steps = stats['train_step']
    assert len(steps) == 2 and all(s['tokens'] > 0 and s['tokens_per_s'] > 0 for s in steps)
    assert os.path.exists(res_path)
    saved = cli.load_res(res_path)
    losses = [float(line.split('LOSS:')[1]) for line in saved['logger'].record if 'LOSS:' in line]
    assert len(losses) == 2 and losses[1] < losses[0]
