"""CPU checks of the max-semiring training step of the decomposed i-FST (--train_mode max): the torch
restatement against the loss and gradients captured from the reference, the C-ABI entry point that selects the semiring, and
the model mirror accepting train_mode = 'max' for training."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import decomp_max_train_ref as dmr
from util import GOLDEN, ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = ('S1', 'S2', 'V_embed', 'embed_r_generalized', 'C_output_mat', 'wildcard_mat', 'h0', 'hT', 'beta_vec',
          'embedding.weight')
GATES = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')


def load():
    with open(os.path.join(GOLDEN, 'decomp_train_max_small.json')) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, 'decomp_train_max_small.npz')), np.load(os.path.join(GOLDEN, 'decomp_small.npz'))


@pytest.mark.parametrize('k', range(10))
def test_restatement_matches_the_reference_capture(k):
    meta, g, base = load()
    cfg = meta['configs'][k]
    pre = 'c{}.'.format(k)
    p = {n: g[pre + 'w.' + n] for n in PARAMS}
    p['priority_mat'] = g[pre + 'w.priority_mat']
    for n in GATES + ('crf.transitions',):
        if pre + 'w.' + n in g.files:
            p[n] = g[pre + 'w.' + n]
    x, lengths = torch.from_numpy(base['x']), torch.from_numpy(base['lengths'])
    loss, grads = dmr.train_step(p, x, lengths, g['labels'], nl=cfg['update_nonlinear'],
                                 additional_nonlinear=cfg.get('additional_nonlinear', 'none'),
                                 use_priority=bool(cfg.get('use_priority', 0)), farnn=cfg['farnn'],
                                 sig_k=float(cfg.get('sigmoid_exponent', 5)), dtype=torch.float32,
                                 min_gap=meta['min_gap'])
    ref = float(g[pre + 'loss'])
    assert abs(loss - ref) < 1e-5 * max(1.0, abs(ref))
    for n in PARAMS + GATES + ('crf.transitions',):
        if pre + 'g.' + n not in g.files:
            continue
        want = g[pre + 'g.' + n]
        got = grads[n].reshape(want.shape)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * max(float(np.abs(want).max()), 1e-3), err_msg=n)


def test_set_semiring_is_declared_bound_and_exported():
    from re2nn_seq_amd import _lib
    with open(os.path.join(ROOT, 'include', 'farnn.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    assert re.search(r'\bint\s+farnn_train_set_semiring\s*\(\s*farnn_train_ctx\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)', text)
    assert 'farnn_train_set_semiring' in _lib.SIGNATURES
    assert os.path.exists(_lib.LIB_PATH), 'run __graft_entry__.build() first'
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'farnn_train_set_semiring')


def test_the_mirror_accepts_train_mode_max_for_training():
    """forward_local(train=True) with train_mode='max' passes _check_trainable; without a device the step then fails
    loudly with FarnnError (there is no CPU fallback)."""
    from re2nn_seq_amd import _lib
    from re2nn_seq_amd.farnn.model_decompose_single import FARNN_S_D_W_I_S
    meta, g, base = load()
    a = ns(**dict(meta['train_flags'], **{k: v for k, v in meta['configs'][0].items() if k != 'seed'}))
    torch.manual_seed(0)
    m = FARNN_S_D_W_I_S(V=base['V_in'], S1=base['S1_in'], S2=base['S2_in'], C_output_mat=base['O_in'],
                        wildcard_mat=base['W_in'], wildcard_output_vector=base['Ow_in'], final_vector=base['final_in'],
                        start_vector=base['start_in'], pretrained_word_embed=base['E_in'],
                        priority_mat=base['priority_in'], args=a, o_idx=meta['o_idx'])
    m._check_trainable(None)
    if torch.cuda.is_available():
        pytest.skip('a GPU is present: tests/test_gpu_train_max.py runs the step')
    x, lengths = torch.from_numpy(base['x']), torch.from_numpy(base['lengths'])
    with pytest.raises(_lib.FarnnError):
        m.forward_local(x, torch.from_numpy(g['labels']), lengths, train=True)
