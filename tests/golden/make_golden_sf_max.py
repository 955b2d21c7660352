#!/usr/bin/env python3
"""Golden fixture of the vector-input tagger in the max semiring: the REFERENCE's FARNN_S_SF.forward(train=False) on the CPU
with train_mode='max' (model_decompose_single.py:435-442).

Runs only where the reference checkout is mounted (like make_golden_sf.py); only data is stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sf_max.py

Weights: entries of decomp_small.{json,npz}, each run with train_mode overridden to 'max' (FARNN_S_SF has FARNN_S_D_W_I_S's
parameters minus the word table, whatever the semiring).  The configs span farnn 0 / 1 / 2, every update_nonlinear, the CRF and
the priority layer.  Inputs: the v and lengths of sf_small.npz (B 7, L 9, lengths including 1 and L), scaled by V_SCALE: in the
max semiring a state is one product of L entries, not a sum of many, and the scores' margins shrink with it.
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
except ImportError:       # bert_embeddings.py imports BertModel at module level; FARNN_S_SF never touches it
    sys.modules['transformers'] = types.SimpleNamespace(BertModel=None)
if 'src_seq.ptm.bert_utils' not in sys.modules:
    try:
        import src_seq.ptm.bert_utils  # noqa: F401
    except Exception:
        sys.modules.setdefault('src_seq.ptm', types.ModuleType('src_seq.ptm'))
        sys.modules['src_seq.ptm.bert_utils'] = types.SimpleNamespace(unflatten_with_lengths=None)

from src_seq.farnn.model_decompose_single import FARNN_S_SF  # noqa: E402
from util import ns  # noqa: E402
import sf_tag_ref  # noqa: E402
import sf_max_tag_ref  # noqa: E402

torch.set_num_threads(4)
SF_KEYS = ('S1', 'S2', 'C_output_mat', 'wildcard_mat', 'wildcard_output_vector', 'h0', 'hT',
           'Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')
CONFIGS = [0, 1, 2, 4, 5, 6, 7, 8, 9]     # of decomp_small: farnn 0 / 1 / 2 x tanh / none / relu / relutanh, CRF (1, 5, 8), priority (8)
V_SCALE = float(os.environ.get('SF_MAX_V_SCALE', '1.0'))


def main():
    with open(os.path.join(HERE, 'decomp_small.json')) as f:
        meta = json.load(f)
    g = np.load(os.path.join(HERE, 'decomp_small.npz'))
    src = np.load(os.path.join(HERE, 'sf_small.npz'))
    v, lengths = (src['v'] * V_SCALE).astype(np.float32), src['lengths']
    B, L, _ = v.shape
    vt, lt = torch.from_numpy(v), torch.from_numpy(lengths)
    label = torch.zeros((B, L), dtype=torch.int64)
    blob = {'v': v, 'lengths': lengths}
    for k in CONFIGS:
        cfg = dict(meta['configs'][k], train_mode='max')
        a = ns(independent=2, threshold=meta['threshold'], use_bert=0, **cfg)
        torch.manual_seed(0)
        m = FARNN_S_SF(S1=g['S1_in'], S2=g['S2_in'], C_output_mat=g['O_in'], wildcard_mat=g['W_in'],
                       wildcard_output_vector=g['Ow_in'], final_vector=g['final_in'], start_vector=g['start_in'],
                       priority_mat=g['priority_in'], args=a, o_idx=meta['o_idx'], is_cuda=False)
        pre = 'c{}.'.format(k)
        with torch.no_grad():
            for kk in SF_KEYS:
                if pre + kk in g.files:
                    getattr(m, kk).copy_(torch.from_numpy(g[pre + kk]))
            if a.use_crf:
                m.crf.transitions.copy_(torch.from_numpy(g[pre + 'crf_transitions']))
        captured = {}
        orig = m.decode

        def spy(all_scores, flat, mask, lens, _c=captured, _o=orig):
            _c['scores'] = all_scores.detach().numpy().copy()
            return _o(all_scores, flat, mask, lens)
        m.decode = spy
        with torch.no_grad():
            _, pred, _ = m(vt, label, lt, train=False)
        blob[pre + 'scores'] = captured['scores']
        blob[pre + 'flat_pred'] = pred.numpy()
        # the inputs are chosen so that the reference itself stays inside the tests' cap on undecided positions
        decided = sf_max_tag_ref.decided_positions(g, k, cfg, meta, v, lengths)
        left_out = 1.0 - decided[np.arange(L)[None, :] < lengths[:, None]].mean()
        print('config', k, cfg, 'undecided valid positions: {:.1%}'.format(left_out),
              'max |score| {:.3g}'.format(np.abs(captured['scores']).max()))
        assert left_out <= sf_tag_ref.UNDECIDED_CAP, (k, left_out)
    np.savez_compressed(os.path.join(HERE, 'sf_max_small.npz'), **blob)
    with open(os.path.join(HERE, 'sf_max_small.json'), 'w') as f:
        json.dump({'configs': CONFIGS, 'source': 'decomp_small', 'inputs': 'sf_small', 'v_scale': V_SCALE, 'train_mode': 'max'},
                  f, sort_keys=True)
    print('wrote sf_max_small.npz', os.path.getsize(os.path.join(HERE, 'sf_max_small.npz')), 'bytes')


if __name__ == '__main__':
    main()
