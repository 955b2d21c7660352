"""The KD / PR teacher step of the decomposed i-FST without a GPU: the restatement (tests/decomp_teacher_train_ref.py)
reproduces the reference's captures, every planted fault is seen, and the model mirror's refusals come before any device work.

Bars: the loss within 2e-5 max(1, |ref|) and every gradient at the close() bar of tests/test_gpu_train_max.py -- the bars
tests/test_gpu_decomp_teacher_train.py applies to the library."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import decomp_teacher_train_ref as dtr  # noqa: E402
from util import GOLDEN, ns  # noqa: E402

PARAMS = ('S1', 'S2', 'V_embed', 'embed_r_generalized', 'C_output_mat', 'wildcard_mat', 'h0', 'hT', 'beta_vec',
          'embedding.weight')
GATES = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')
N_CONFIGS = 12


def load():
    with open(os.path.join(GOLDEN, 'decomp_train_teacher_small.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, 'decomp_train_teacher_small.npz')), np.load(os.path.join(GOLDEN, 'decomp_small.npz'))


META, G, BASE = load()


def bar(ref, rtol=2e-3, atol=2e-6, frac=2e-4):
    """what tests/test_gpu_train_max.py::close accepts at each entry of ref"""
    return atol + frac * max(float(np.abs(ref).max()), 1e-6) + rtol * np.abs(ref)


def names_of(k):
    pre = 'c{}.'.format(k)
    return PARAMS + tuple(n for n in ('crf.transitions',) + GATES if pre + 'w.' + n in G.files)


def restate(k, dtype=torch.float64, fault=None):
    cfg = META['configs'][k]
    pre = 'c{}.'.format(k)
    p = {n: G[pre + 'w.' + n] for n in names_of(k)}
    p['priority_mat'] = G[pre + 'w.priority_mat']
    return dtr.train_step(p, BASE['x'], BASE['lengths'], G['labels'], G['re_tags'], cfg['marryup_type'], cfg['c1_kdpr'],
                          cfg['c2_kdpr'], cfg.get('c3_pr', 1.0), nl=cfg['update_nonlinear'],
                          additional_nonlinear=cfg.get('additional_nonlinear', 'none'), use_priority=bool(cfg.get('use_priority')),
                          farnn=cfg['farnn'], sig_k=float(cfg.get('sigmoid_exponent', 5)), dtype=dtype, fault=fault)


def worst_miss(k, loss, grads):
    """the largest (difference / bar) over the loss and every stored gradient of configuration k"""
    pre = 'c{}.'.format(k)
    ref_loss = float(G[pre + 'loss'])
    w = abs(loss - ref_loss) / (2e-5 * max(1.0, abs(ref_loss)))
    for n in names_of(k):
        ref = G[pre + 'g.' + n]
        w = max(w, float((np.abs(grads[n].reshape(ref.shape) - ref) / bar(ref)).max()))
    return w


def test_the_fixtures_can_see_the_pad_path():
    lengths = BASE['lengths']
    assert (lengths.max() - lengths >= 2).any()
    assert G['re_tags'].shape[1] > lengths.max()
    assert len(META['configs']) == N_CONFIGS
    pr = [c for c in META['configs'] if c['marryup_type'] == 'pr']
    assert any(c['c3_pr'] < c['c2_kdpr'] for c in pr) and any(c['c3_pr'] > c['c2_kdpr'] for c in pr)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('k', range(N_CONFIGS))
def test_restatement_reproduces_the_reference(k, dtype):
    loss, grads = restate(k, dtype)
    assert set(grads) == set(names_of(k))
    assert worst_miss(k, loss, grads) <= 1.0


def applies(fault, cfg):
    if fault in ('detach_pr', 'pi_c2'):
        return cfg['marryup_type'] == 'pr' and (fault == 'detach_pr' or cfg['c3_pr'] > cfg['c2_kdpr'])
    if fault == 'no_T2':
        return cfg['marryup_type'] == 'kd' and cfg['c1_kdpr'] != 1.0
    return fault in ('mask_pads', 'divisor_valid')       # 'tail_reversed': the fixtures' pad tokens are all the pad word (below)


@pytest.mark.parametrize('fault', ['mask_pads', 'divisor_valid', 'detach_pr', 'no_T2', 'pi_c2'])
def test_planted_faults_miss_every_fixture_they_apply_to(fault):
    hit = 0
    for k, cfg in enumerate(META['configs']):
        if not applies(fault, cfg):
            continue
        hit += 1
        loss, grads = restate(k, torch.float64, fault)
        assert worst_miss(k, loss, grads) > 1.0, (fault, k)
    assert hit >= 2, fault


def drawn_case(seed, S=9, R=7, K=5, V=13, B=4, L=6, farnn=1, crf=False, prio=True):
    from test_gpu_train_max import draw
    w, x, lengths, labels = draw(S, R, K, V, B, L, 'tanh', farnn, crf, prio, seed=seed)
    lengths[:] = [L, 0, 1, L - 3][:B]
    re = (np.random.RandomState(seed).rand(B, L, K) * 1.0).astype(np.float32)
    return w, x, lengths, labels, re


@pytest.mark.parametrize('mode', ['kd', 'pr'])
def test_a_reversed_tail_is_seen_on_distinct_pad_tokens(mode):
    """The fixtures pad with one word, so the order of the backward chain's tail cannot show there; on a drawn batch whose pad
    positions hold distinct words it moves gradients by far more than the bar of tests/util.py::check_grad (1e-4 of the scale)."""
    w, x, lengths, labels, re = drawn_case(3)
    assert len(set(x[3, 3:])) > 1
    _, good, _ = dtr.step_on_table(w, x, lengths, labels, re, mode, 2.0, 0.3, nl='tanh', farnn=1)
    _, bad, _ = dtr.step_on_table(w, x, lengths, labels, re, mode, 2.0, 0.3, nl='tanh', farnn=1, fault='tail_reversed')
    assert max(float(np.abs(bad[n] - good[n]).max() / np.abs(good[n]).max()) for n in good) > 1e-2


def test_pad_word_rows_of_dvgen_are_not_zero():
    w, x, lengths, labels, re = drawn_case(4)
    valid = np.arange(x.shape[1])[None, :] < lengths[:, None]
    only_pad = sorted(set(x[~valid]) - set(x[valid]))
    assert only_pad
    _, g, _ = dtr.step_on_table(w, x, lengths, labels, re, 'kd', 2.0, 0.3, nl='tanh', farnn=1)
    assert all(np.abs(g['Vgen'][t]).max() > 0 for t in only_pad)
    _, g1, _ = dtr.step_on_table(w, x, lengths, labels, re, 'kd', 2.0, 1.0, nl='tanh', farnn=1)      # pi = 1: the plain step
    assert all(np.abs(g1['Vgen'][t]).max() == 0 for t in only_pad)


# ---- the mirror's refusals: before any device work, so they need no GPU ----------------------------------------------------
def mirror(**kw):
    from re2nn_seq_amd.farnn.model_decompose_single import FARNN_S_D_W_I_S
    torch.manual_seed(0)
    return FARNN_S_D_W_I_S(V=BASE['V_in'], S1=BASE['S1_in'], S2=BASE['S2_in'], C_output_mat=BASE['O_in'], wildcard_mat=BASE['W_in'],
                           wildcard_output_vector=BASE['Ow_in'], final_vector=BASE['final_in'], start_vector=BASE['start_in'],
                           pretrained_word_embed=BASE['E_in'], priority_mat=BASE['priority_in'], args=ns(**kw), o_idx=META['o_idx'])


def batch():
    return (torch.from_numpy(BASE['x']), torch.from_numpy(G['labels']), torch.from_numpy(BASE['lengths']),
            torch.from_numpy(G['re_tags']))


TODAY = 'no KD/PR teachers (DESIGN.md, row f3)'


@pytest.mark.parametrize('kw,with_re', [(dict(marryup_type='kd'), True), (dict(marryup_type='pr'), True),
                                        (dict(marryup_type='kd'), False), (dict(), True)])
def test_without_the_switch_the_refusal_is_todays(kw, with_re, monkeypatch):
    monkeypatch.delenv('RE2NN_DECOMP_TEACHER_TRAIN', raising=False)
    x, lab, lengths, re = batch()
    with pytest.raises(NotImplementedError) as e:
        mirror(**kw).forward_local(x, lab, lengths, train=True, re_tags=re if with_re else None)
    assert str(e.value) == ('the HIP training step covers the sum and max semirings and the CE1 loss (with or without the CRF), '
                            + TODAY)


def test_with_the_switch_the_checks_come_before_any_device_work(monkeypatch):
    monkeypatch.setenv('RE2NN_DECOMP_TEACHER_TRAIN', '1')
    x, lab, lengths, re = batch()
    with pytest.raises(ValueError, match='needs the RE teacher'):
        mirror(marryup_type='kd').forward_local(x, lab, lengths, train=True)
    with pytest.raises(ValueError, match='re_tags were given'):
        mirror().forward_local(x, lab, lengths, train=True, re_tags=re)
    with pytest.raises(NotImplementedError, match='row f3'):
        mirror(marryup_type='pr', train_mode='max').forward_local(x, lab, lengths, train=True, re_tags=re)
    with pytest.raises(NotImplementedError, match=TODAY.replace('(', r'\(').replace(')', r'\)')):
        mirror(marryup_type='input').forward_local(x, lab, lengths, train=True)


def test_the_mirror_pads_cuts_and_weighs_as_the_reference():
    x, lab, lengths, re = batch()
    Lmax = int(lengths.max())
    for crf in (0, 1):
        m = mirror(marryup_type='pr', use_crf=crf, c1_kdpr=2.0, c2_kdpr=0.3, c3_pr=0.8)
        r, mode, c1, pi = m._teacher(re, Lmax)
        assert tuple(r.shape) == (x.shape[0], Lmax, m.C) and mode == 'pr' and c1 == 2.0 and pi == 0.8
        assert np.array_equal(r.numpy(), dtr.pad_and_cut(G['re_tags'], bool(crf), Lmax))
    assert mirror(marryup_type='pr', c2_kdpr=0.3, c3_pr=0.1)._teacher(re, Lmax)[3] == 0.3
    assert mirror(marryup_type='kd', c2_kdpr=0.3, c3_pr=0.9)._teacher(re, Lmax)[3] == 0.3
