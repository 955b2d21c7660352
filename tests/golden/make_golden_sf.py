#!/usr/bin/env python3
"""Golden fixture of the vector-input tagger: the REFERENCE's FARNN_S_SF.forward(train=False) on the CPU.

Runs only where the reference checkout is mounted (like make_golden.py); only data is stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sf.py

Weights and configs: the eleven sum-semiring entries of decomp_small.{json,npz} (FARNN_S_SF has FARNN_S_D_W_I_S's parameters
minus the word table).  Inputs: dense random vectors [B, L, R] that are rows of no table, ragged lengths that include 1 and L.
Also captured: EmbedAggregator.forward on decomp_small's word ids and static embeddings (per distinct (beta,
additional_nonlinear) pair), so that aggregate -> SF can be held to FARNN_S_D_W_I_S on the same ids.
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
except ImportError:       # bert_embeddings.py imports BertModel at module level; EmbedAggregator(use_bert=0) never touches it
    sys.modules['transformers'] = types.SimpleNamespace(BertModel=None)
if 'src_seq.ptm.bert_utils' not in sys.modules:
    try:
        import src_seq.ptm.bert_utils  # noqa: F401
    except Exception:
        sys.modules.setdefault('src_seq.ptm', types.ModuleType('src_seq.ptm'))
        sys.modules['src_seq.ptm.bert_utils'] = types.SimpleNamespace(unflatten_with_lengths=None)

from src_seq.farnn.model_decompose_single import FARNN_S_SF  # noqa: E402
from src_seq.farnn.bert_embeddings import EmbedAggregator  # noqa: E402
from util import ns  # noqa: E402
import sf_tag_ref  # noqa: E402

torch.set_num_threads(4)
SF_KEYS = ('S1', 'S2', 'C_output_mat', 'wildcard_mat', 'wildcard_output_vector', 'h0', 'hT',
           'Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')
B, L = 7, 9
LENGTHS = np.array([9, 1, 4, 9, 2, 6, 1], np.int64)


def main():
    with open(os.path.join(HERE, 'decomp_small.json')) as f:
        meta = json.load(f)
    g = np.load(os.path.join(HERE, 'decomp_small.npz'))
    R = g['S1_in'].shape[1]
    rng = np.random.RandomState(2024)
    v = (rng.randn(B, L, R) * 0.4).astype(np.float32)
    vt, lt = torch.from_numpy(v), torch.from_numpy(LENGTHS)
    label = torch.zeros((B, L), dtype=torch.int64)
    ks = [k for k, cfg in enumerate(meta['configs']) if cfg.get('train_mode', 'sum') == 'sum']
    assert len(ks) == 11
    blob = {'v': v, 'lengths': LENGTHS}
    for k in ks:
        cfg = meta['configs'][k]
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
        decided = sf_tag_ref.decided_positions(g, k, cfg, meta, v, LENGTHS)
        left_out = 1.0 - decided[np.arange(L)[None, :] < LENGTHS[:, None]].mean()
        print('config', k, cfg, 'undecided valid positions: {:.1%}'.format(left_out))
        assert left_out <= sf_tag_ref.UNDECIDED_CAP, (k, left_out)
    # EmbedAggregator.forward on decomp_small's ids
    x, lx = torch.from_numpy(g['x']), torch.from_numpy(g['lengths'])
    seen = {}
    for k in ks:
        cfg = meta['configs'][k]
        key = (cfg.get('beta', 1.0), cfg.get('additional_nonlinear', 'none'))
        if key in seen:
            continue
        seen[key] = k
        a = ns(independent=2, use_bert=0, **cfg)
        agg = EmbedAggregator(a, g['V_in'], g['E_in'])
        # (the reference's forward calls self.embed(inp) while WordEmbedding.forward(inp, lengths) wants both and ignores the
        #  second: as written it raises a TypeError.  The call is completed here; nothing it computes changes.)
        agg.embed.forward = lambda inp, lengths=None, _f=agg.embed.forward: _f(inp, lengths)
        with torch.no_grad():
            blob['agg{}.out'.format(k)] = agg(x, lx).numpy()
            blob['agg{}.embed_r_generalized'.format(k)] = agg.embed_r_generalized.detach().numpy()
    np.savez_compressed(os.path.join(HERE, 'sf_small.npz'), **blob)
    with open(os.path.join(HERE, 'sf_small.json'), 'w') as f:
        json.dump({'configs': ks, 'agg': {str(k): list(key) for key, k in seen.items()}, 'source': 'decomp_small'}, f, sort_keys=True)
    print('wrote sf_small.npz', os.path.getsize(os.path.join(HERE, 'sf_small.npz')), 'bytes')


if __name__ == '__main__':
    main()
