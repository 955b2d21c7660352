#!/usr/bin/env python3
"""Golden fixture of the vector-input tagger's TRAINING step: the REFERENCE's FARNN_S_SF.forward(train=True) + loss.backward()
on the CPU, with input.requires_grad_().

Runs only where the reference checkout is mounted (like make_golden_sf.py); only data is stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sf_train.py

Automaton inputs: decomp_small.npz (the factors and automaton-derived matrices make_golden.py stored).  Configs: farnn 0 / 1 / 2 x
{plain, CRF, priority}, every trainable flag the class has switched on.  Inputs: dense random vectors [B, L, R], ragged lengths
that include 1 and L.  Stored per config: the weights as constructed, the loss, every parameter's gradient and input.grad.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, '/root/reference')

import torch  # noqa: E402

try:
    import transformers  # noqa: F401
except ImportError:
    sys.modules['transformers'] = types.SimpleNamespace(BertModel=None)
if 'src_seq.ptm.bert_utils' not in sys.modules:
    try:
        import src_seq.ptm.bert_utils  # noqa: F401
    except Exception:
        sys.modules.setdefault('src_seq.ptm', types.ModuleType('src_seq.ptm'))
        sys.modules['src_seq.ptm.bert_utils'] = types.SimpleNamespace(unflatten_with_lengths=None)

from src_seq.farnn.model_decompose_single import FARNN_S_SF  # noqa: E402
from util import ns  # noqa: E402

torch.set_num_threads(4)
B, L = 5, 6
LENGTHS = np.array([6, 1, 4, 6, 2], np.int64)
CONFIGS = [dict(farnn=f, xavier=1, bias_init=0.5, update_nonlinear=nl, **extra)
           for f, nl in ((0, 'tanh'), (1, 'relutanh'), (2, 'tanh'))
           for extra in (dict(), dict(use_crf=1, rand_constant=1e-2), dict(use_priority=1))]
TRAIN_ALL = dict(train_wildcard=1, train_h0=1, train_hT=1, train_c_output=1)
KEYS = ('S1', 'S2', 'C_output_mat', 'wildcard_mat', 'h0', 'hT', 'Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')


def main():
    g = np.load(os.path.join(HERE, 'decomp_small.npz'))
    with open(os.path.join(HERE, 'decomp_small.json')) as f:
        meta = json.load(f)
    R, C = g['S1_in'].shape[1], g['O_in'].shape[0]
    rng = np.random.RandomState(4242)
    v = (rng.randn(B, L, R) * 0.4).astype(np.float32)
    labels = rng.randint(0, C, size=(B, L)).astype(np.int64)
    blob = {'v': v, 'lengths': LENGTHS, 'labels': labels}
    for k, cfg in enumerate(CONFIGS):
        torch.manual_seed(900 + k)
        a = ns(independent=2, threshold=meta['threshold'], use_bert=0, **dict(TRAIN_ALL, **cfg))
        m = FARNN_S_SF(S1=g['S1_in'], S2=g['S2_in'], C_output_mat=g['O_in'], wildcard_mat=g['W_in'],
                       wildcard_output_vector=g['Ow_in'], final_vector=g['final_in'], start_vector=g['start_in'],
                       priority_mat=g['priority_in'], args=a, o_idx=meta['o_idx'], is_cuda=False)
        if a.use_crf:
            with torch.no_grad():
                m.crf.transitions += torch.randn_like(m.crf.transitions) * 0.3
        pre = 'c{}.'.format(k)
        sd = {kk: vv.detach().numpy().copy() for kk, vv in m.state_dict().items()}
        for kk in KEYS:
            if kk in sd:
                blob[pre + 'w.' + kk] = sd[kk]
        blob[pre + 'w.priority_mat'] = sd['priority_layer.priority_mat']
        if a.use_crf:
            blob[pre + 'w.crf.transitions'] = sd['crf.transitions']
        vt = torch.from_numpy(v).clone().requires_grad_()
        m.train()
        loss, pred, _ = m(vt, torch.from_numpy(labels), torch.from_numpy(LENGTHS), train=True)
        loss.backward()
        blob[pre + 'loss'] = np.float32(loss.item())
        blob[pre + 'flat_pred'] = pred.numpy()
        blob[pre + 'g.v'] = vt.grad.numpy().copy()
        named = dict(m.named_parameters())
        for kk in KEYS + ('crf.transitions',):
            if kk in named and named[kk].grad is not None:
                blob[pre + 'g.' + kk] = named[kk].grad.numpy().copy()
        print(k, cfg, 'loss', float(loss), 'gradients', sorted(n for n in blob if n.startswith(pre + 'g.')))
    np.savez_compressed(os.path.join(HERE, 'sf_train_small.npz'), **blob)
    with open(os.path.join(HERE, 'sf_train_small.json'), 'w') as f:
        json.dump({'configs': CONFIGS, 'train_flags': TRAIN_ALL, 'o_idx': int(meta['o_idx']), 'threshold': meta['threshold'],
                   'source': 'decomp_small'}, f, sort_keys=True)
    print('wrote sf_train_small.npz', os.path.getsize(os.path.join(HERE, 'sf_train_small.npz')), 'bytes')


if __name__ == '__main__':
    main()
