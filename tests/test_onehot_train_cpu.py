"""CPU checks of the onehot i-FST training step (FARNN_S_O_I_S): the torch restatement against the
loss / gradients / predictions captured from the reference, the C-ABI struct layouts, and the refusals that must come
before any device work."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import onehot_train_ref as otr
from util import GOLDEN, ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden():
    with open(os.path.join(GOLDEN, 'ifst_train_small.json')) as f:
        meta = json.load(f)
    return meta['configs'], np.load(os.path.join(GOLDEN, 'ifst_train_small.npz'))


def case(k):
    """(inputs dict, captured dict) of captured configuration k"""
    cfgs, g = _golden()
    cfg = cfgs[k]
    base = np.load(os.path.join(GOLDEN, cfg['base'] + '.npz'))
    C = base['O'].shape[0]
    pri = np.eye(C, dtype=np.float32)
    if cfg['use_priority']:
        sp = np.load(os.path.join(GOLDEN, 'ifst_small.npz'))['priority']
        pri[:sp.shape[0], :sp.shape[0]] = sp
    inp = dict(T=base['T'].astype(np.float32), W=base['W'].astype(np.float32), O=base['O'].astype(np.float32),
               h0=base['h0'].astype(np.float32), hT=base['hT'].astype(np.float32),
               P=pri if cfg['use_priority'] else None, x=base['x'], lengths=base['lengths'],
               labels=g[cfg['base'] + '.labels'], nl=cfg['update_nonlinear'], threshold=float(base['threshold']),
               o_idx=int(base['o_idx']))
    pre = 'c{}.'.format(k)
    ref = dict(loss=float(g[pre + 'loss']), dT=g[pre + 'g.language_tensor'], flat_pred=g[pre + 'flat_pred'])
    return cfg, inp, ref


N_CASES = 16


@pytest.mark.parametrize('k', range(N_CASES))
def test_restatement_matches_the_reference_capture(k):
    _, inp, ref = case(k)
    loss, dT, pred = otr.step(dtype=torch.float32, **inp)
    np.testing.assert_allclose(loss, ref['loss'], rtol=2e-6, atol=1e-7)
    scale = float(np.abs(ref['dT']).max())
    np.testing.assert_allclose(dT, ref['dT'], rtol=1e-5, atol=1e-6 * scale)
    assert np.array_equal(pred, ref['flat_pred'])


def test_ctypes_layouts_of_the_onehot_train_structs(tmp_path):
    from re2nn_seq_amd import _lib
    pairs = {'farnn_onehot_train_dims': _lib.OnehotTrainDims, 'farnn_onehot_train_weights': _lib.OnehotTrainWeights,
             'farnn_onehot_train_outputs': _lib.OnehotTrainOutputs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "farnn.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        lines.append('  printf("%s sizeof %zu\\n", "{0}", sizeof({0}));'.format(cname))
        for fname, _ in cls._fields_:
            lines.append('  printf("%s.%s %zu\\n", "{0}", "{1}", offsetof({0}, {1}));'.format(cname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = dict(line.rsplit(' ', 1) for line in out.strip().splitlines())
    for cname, cls in pairs.items():
        assert int(got[cname + ' sizeof']) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got['{}.{}'.format(cname, fname)]) == getattr(cls, fname).offset, (cname, fname)


def _no_device(monkeypatch):
    """from here on no GPU is visible and any use of the HIP library fails the test"""
    from re2nn_seq_amd import _lib

    def boom(*a, **k):
        raise AssertionError('device work before the refusal')
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    monkeypatch.setattr(_lib, 'OnehotTrainContext', boom)
    monkeypatch.setattr(_lib, 'load', boom)


def _ifst(**kw):
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I_S
    g = np.load(os.path.join(GOLDEN, 'ifst_small.npz'))
    S = g['T'].shape[1]
    return FARNN_S_O_I_S(g['T'], g['O'], g['W'], np.zeros(S), g['hT'], g['h0'], None, ns(**kw), o_idx=int(g['o_idx']))


def test_max_semiring_training_is_refused_before_device_work(monkeypatch):
    m = _ifst(train_mode='max')
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError, match='sum semiring'):
        m.enable_training()
    x = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(NotImplementedError, match='sum semiring'):
        m.forward_local(x, x, torch.tensor([3, 2]), train=True)


def test_crf_extension_training_is_refused_before_device_work(monkeypatch):
    m = _ifst().enable_crf()
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError, match='CRF'):
        m.enable_training()


@pytest.mark.parametrize('independent', [0, 1])
def test_onehot_fst_and_ind1_epochs_are_refused_before_device_work(tmp_path, monkeypatch, independent):
    from re2nn_seq_amd import main as cli
    from re2nn_seq_amd import synth
    tree = synth.write_dataset_tree(str(tmp_path / 'data'), dataset='ATIS-BIO', seed=4)
    argv = ['--dataset', 'ATIS-BIO', '--method', 'onehot', '--independent', str(independent),
            '--automata_path', tree['paths']['ID{}'.format(independent)], '--normalize_automata', 'none',
            '--rand_constant', '0', '--bz', '10', '--seq_max_len', '12', '--epoch', '1', '--train_portion', '1.0',
            '--data_dir', tree['paths']['data_dir'], '--model_dir', str(tmp_path)]
    _no_device(monkeypatch)
    with pytest.raises(NotImplementedError) as e:
        cli.main(argv)
    assert 'decomposed only' not in str(e.value) and '--epoch 0' in str(e.value)
