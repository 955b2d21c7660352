"""CPU checks of the decomposed FST's training step in the max semiring (FARNN_S_D_W, --train_mode max): the
torch restatement (tests/decomp0_max_train_ref.py) against the loss / gradients / predictions captured from the reference
(tests/golden/decomp0_train_max_small), the arg-max gap rule on every capture and on every drawn GPU case, the planted faults the
captures must see, the new exported symbol, the unchanged struct layouts, and the passes and refusals of
RE2NN_DECOMP_FST_MAX_TRAIN before any device work."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import decomp0_max_train_cases as cases
import decomp0_max_train_ref as d0m
import test_decomp0_train_cpu as sum_cpu
from test_decomp0_train_cpu import PARAMS, WORD_ROWS, check_all_grads
from util import GOLDEN, assert_float_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CASES = 13
SYMBOL = 'farnn_decomp_fst_train_set_semiring'


def _golden():
    with open(os.path.join(GOLDEN, 'decomp0_train_max_small.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, 'decomp0_train_max_small.npz'))


def case(k):
    """(configuration, restatement keywords, captured dict) of captured configuration k, as test_decomp0_train_cpu.case"""
    meta, g = _golden()
    cfg = meta['configs'][k]
    pre = 'c{}.'.format(k)
    names = PARAMS + d0m.gate_keys(cfg['farnn']) + ((d0m.TRANS,) if cfg['use_crf'] else ())
    p = {n: g[pre + 'p.' + n].astype(np.float32) for n in names}
    trans = p.pop(d0m.TRANS, None)
    inp = dict(p=p, P=g[pre + 'priority'].astype(np.float32) if cfg['use_priority'] else None, x=g['x'], lengths=g['lengths'],
               labels=g['labels'], nl=cfg['update_nonlinear'], add_nl=cfg['additional_nonlinear'], farnn=cfg['farnn'], k=5.0,
               threshold=float(meta['threshold']), o_idx=int(meta['o_idx']), trans=trans)
    grads = {}
    for n in names:
        gr = g[pre + 'g.' + n]
        if n in WORD_ROWS:
            full = np.zeros(p[n].shape, np.float32)
            full[g[pre + 'words']] = gr
            gr = full
        grads[n] = gr
    return cfg, inp, dict(loss=float(g[pre + 'loss']), grads=grads, words=g[pre + 'words'], flat_pred=g[pre + 'flat_pred'])


def present_of(inp, ref):
    present = np.zeros(inp['p']['V_embed'].shape[0], bool)
    present[ref['words']] = True
    return present


def test_the_captures_cover_the_configurations():
    cfgs = _golden()[0]['configs']
    assert len(cfgs) == N_CASES and all(c['train_mode'] == 'max' for c in cfgs)
    assert {(c['farnn'], c['use_crf'], c['use_priority']) for c in cfgs[:12]} == {(f, c, u) for f in (0, 1, 2) for c in (0, 1) for u in (0, 1)}
    assert {c['update_nonlinear'] for c in cfgs} == {'none', 'relu', 'tanh', 'relutanh'}
    assert cfgs[12].get('additional_states') == 2
    assert os.path.getsize(os.path.join(GOLDEN, 'decomp0_train_max_small.npz')) <= os.path.getsize(os.path.join(GOLDEN, 'decomp0_train_small.npz'))


@pytest.mark.parametrize('k', range(N_CASES))
def test_restatement_matches_the_reference_capture(k):
    """the gap rule on the capture; the float32 and float64 restatement against the float32 reference: the loss by
    assert_float_path, every gradient at util.check_grad's default bar, the predictions by equality"""
    cfg, inp, ref = case(k)
    d0m.check_gap(**{q: v for q, v in inp.items() if q not in ('labels', 'o_idx')})
    loss64, g64, pred = d0m.step(dtype=torch.float64, **inp)
    loss32, g32, pred32 = d0m.step(dtype=torch.float32, **inp)
    assert_float_path(ref['loss'], loss32, loss64, err_msg='loss')
    assert set(ref['grads']) == set(g64)
    for n in g64:
        assert np.abs(ref['grads'][n]).max() > 0, n
    check_all_grads('decomp0-max-ref-c{}'.format(k), ref['grads'], g32, g64, present_of(inp, ref))
    assert np.array_equal(pred, ref['flat_pred']) and np.array_equal(pred32, ref['flat_pred'])


@pytest.mark.parametrize('fault', d0m.FAULTS)
def test_a_planted_fault_breaks_a_capture(fault):
    """each wrong statement of the restatement misses the captured gradients on at least one configuration it applies to"""
    seen = 0
    for k in range(N_CASES):
        cfg, inp, ref = case(k)
        if fault == 'gates_v' and not cfg['farnn']:
            continue
        g32, g64 = (d0m.step(dtype=dt, fault=fault, **inp)[1] for dt in (torch.float32, torch.float64))
        try:
            check_all_grads('planted {} c{}'.format(fault, k), ref['grads'], g32, g64, present_of(inp, ref))
        except AssertionError:
            seen += 1
    assert seen > 0, fault


@pytest.mark.parametrize('name', cases.ALL_NAMES)
def test_every_gpu_case_is_found_and_keeps_the_gap_rule(name):
    """the case finder finds every case of the GPU tests within MAX_DRAWS = 20 draws (it raises otherwise: nothing is skipped),
    and the case it returns keeps the gap rule and has a live gradient in every tensor"""
    assert cases.MAX_DRAWS <= 20
    c, draws = cases.get_case(name)
    assert 1 <= draws <= cases.MAX_DRAWS
    d0m.check_gap(**{q: c[q] for q in ('p', 'P', 'x', 'lengths', 'nl', 'farnn', 'k', 'trans')})
    for n, g in c['g64'].items():
        assert np.abs(g).max() > 0, n


def test_the_word_cases_sit_on_both_sides_of_the_chunk_constant():
    """d0max_wgrad_kernel takes D0M_WCH = 16 distinct words per chunk (csrc/decomp0_train_max.hip.h)"""
    with open(os.path.join(ROOT, 're2nn-seq_amd', 'csrc', 'decomp0_train_max.hip.h')) as f:
        assert 'constexpr int D0M_WCH = 16;' in f.read()
    for name, n in (('words15', 15), ('words16', 16), ('words17', 17), ('words33', 33), ('one-word', 1)):
        c = cases.get_case(name)[0]
        assert int(c['present'].sum()) == n, name
    c = cases.get_case('V-far')[0]
    assert c['p']['Vgen'].shape[0] >= 100 * int(c['present'].sum())


def test_the_library_exports_the_set_semiring_symbol():
    from re2nn_seq_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, 'include', 'farnn.h')) as f:
        hdr = f.read()
    assert SYMBOL in _lib.SIGNATURES
    assert getattr(lib, SYMBOL) is not None
    assert SYMBOL + '(' in hdr and 'model_decompose.py:269-276' in hdr
    assert _lib.DecompFstTrainContext._set_semiring == SYMBOL
    assert 'set_semiring' not in vars(_lib.DecompFstTrainContext)          # the override that raised is gone


def test_the_struct_layouts_are_unchanged(tmp_path):
    sum_cpu.test_ctypes_layouts_of_the_decomp_fst_train_structs(tmp_path)
    from re2nn_seq_amd import _lib
    assert ctypes.sizeof(_lib.DecompFstTrainDims) == 44
    assert (ctypes.sizeof(_lib.DecompFstTrainWeights), ctypes.sizeof(_lib.DecompFstTrainOutputs)) == (18 * 8, 19 * 8)


def test_the_switch_is_in_the_opt_in_table():
    with open(os.path.join(ROOT, 're2nn-seq_amd', 'farnn', '_native.py')) as f:
        assert '#   DECOMP_FST_MAX_TRAIN ' in f.read()


@pytest.mark.parametrize('kw', [dict(), dict(farnn=1), dict(farnn=2), dict(use_crf=1), dict(use_priority=1),
                                dict(update_nonlinear='relutanh')])
def test_with_both_switches_max_passes_the_check_before_device_work(monkeypatch, kw):
    from re2nn_seq_amd import _lib
    monkeypatch.setenv('RE2NN_DECOMP_FST_TRAIN', '1')
    monkeypatch.setenv('RE2NN_DECOMP_FST_MAX_TRAIN', '1')
    m = sum_cpu.model(train_mode='max', **kw)
    sum_cpu._no_device(monkeypatch)
    m._check_trainable()
    with pytest.raises(_lib.FarnnError, match='no MI355X visible'):
        m.enable_training()


def test_with_the_first_switch_only_max_is_refused_in_the_old_words(monkeypatch):
    from re2nn_seq_amd.train_onehot import check_trainable
    monkeypatch.setenv('RE2NN_DECOMP_FST_TRAIN', '1')
    monkeypatch.delenv('RE2NN_DECOMP_FST_MAX_TRAIN', raising=False)
    m = sum_cpu.model(train_mode='max')
    sum_cpu._no_device(monkeypatch)
    x = torch.zeros((2, 3), dtype=torch.int64)
    want = ('training the decomposed FST covers farnn 0 / 1 / 2, the sum semiring and the CE1 loss (with or without the CRF) on one '
            'GPU; the max semiring (--train_mode max) is not built (DESIGN.md, row f11)')
    for call in (m.enable_training, lambda: check_trainable(m), lambda: m.forward_local(x, x, torch.tensor([3, 2]), train=True)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == want


def test_the_second_switch_alone_opens_nothing(monkeypatch):
    monkeypatch.delenv('RE2NN_DECOMP_FST_TRAIN', raising=False)
    monkeypatch.setenv('RE2NN_DECOMP_FST_MAX_TRAIN', '1')
    m = sum_cpu.model(train_mode='max')
    sum_cpu._no_device(monkeypatch)
    with pytest.raises(NotImplementedError) as e:
        m.enable_training()
    assert str(e.value) == sum_cpu.REFUSAL


@pytest.mark.parametrize('kw,match', [(dict(marryup_type='kd'), 'marryup_type kd'), (dict(marryup_type='pr'), 'marryup_type pr'),
                                      (dict(local_loss_func='ML'), 'local_loss_func ML'), (dict(train_mode='min'), 'train_mode min')])
def test_what_stays_refused_under_max(monkeypatch, kw, match):
    monkeypatch.setenv('RE2NN_DECOMP_FST_TRAIN', '1')
    monkeypatch.setenv('RE2NN_DECOMP_FST_MAX_TRAIN', '1')
    m = sum_cpu.model(**dict(dict(train_mode='max'), **kw))
    sum_cpu._no_device(monkeypatch)
    with pytest.raises(NotImplementedError) as e:
        m.enable_training()
    assert match in str(e.value) and 'row f11' in str(e.value), str(e.value)


def test_two_ranks_stay_refused_under_max(monkeypatch):
    from re2nn_seq_amd import dist
    monkeypatch.setenv('RE2NN_DECOMP_FST_TRAIN', '1')
    monkeypatch.setenv('RE2NN_DECOMP_FST_MAX_TRAIN', '1')
    m = sum_cpu.model(train_mode='max')
    sum_cpu._no_device(monkeypatch)
    monkeypatch.setattr(dist, 'world', lambda: (0, 2))
    with pytest.raises(NotImplementedError, match='multi-GPU.*row f11'):
        m.enable_training()
