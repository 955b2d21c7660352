"""The tagging dispatch table: which kernels serve one farnn_tag call, per configuration.

    python tests/golden/make_golden_dispatch.py [out.json]

CONFIGS names one small model + one call per branch of the tagging dispatcher (csrc/farnn_hip.hip); record(cfg) creates
the handle under the configuration's FARNN_* switches (they are read at create), makes ONE farnn_tag call with profiling
on and returns what the library reports about it: kernel_name of the recurrence and score slots before and after the call,
the launch counts of the three timer slots, kernel_algorithmic_bytes of both slots at the call's token count, and a CRC of
the tags (with the number of distinct tags: a table of constant tags would pin little).  tests/golden/dispatch_table.json is
this script's output under the library as it stood BEFORE the dispatcher was split into plan + launch; tests/test_gpu_dispatch_table.py replays CONFIGS against the built library and requires every
field equal.  The entries marked ab=True need the A/B build (csrc/build.py --probes): run the script a second time with
FARNN_LIB pointing at it, and it adds them to the same file.
"""
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'dispatch_table.json')


def _ifst(S=23, C=9, V=60, seed=7, crf=False, P=False, inexact=False, **kw):
    from oracle import farnn_oracle as fo
    from re2nn_seq_amd import _lib, synth
    rng = np.random.RandomState(seed)
    T, W, O, h0, hT = synth.random_ifst_tensors(V, S, C, rng, edges_per_word=max(6.0, 0.7 * S), n_final=max(4, S // 3))      # dense enough that paths survive
    if inexact:
        T[0, 0, min(1, S - 1)] = 0.3            # no f16 holds it: the handle builds no 16-bit image
    Pm = (np.eye(C) + (rng.rand(C, C) < 0.1) * 0.5).astype(np.float32) if P else None
    tr = (fo.crf_default_transitions(C) + rng.randn(C + 2, C + 2).astype(np.float32) * 0.5) if crf else None
    return _lib.create_onehot_ifst(T, W, O, h0, hT, P=Pm, use_crf=crf, crf_trans=tr, o_idx=1, **kw), V


def _compact(**kw):
    h, V = _ifst(**kw)
    h.set_compact(True)
    return h, V


def _fst4(S=10, C=4, V=20, seed=3):
    from re2nn_seq_amd import _lib
    rng = np.random.RandomState(seed)
    T4 = (rng.rand(V, C, S, S) < 0.08).astype(np.float32)
    W4 = (rng.rand(C, S, S) < 0.05).astype(np.float32)
    h0 = np.eye(S, dtype=np.float32)[0]
    hT = (rng.rand(S) < 0.4).astype(np.float32)
    return _lib.create_onehot_fst4(T4, W4, h0, hT, o_idx=1), V


def _ind1(S=10, C=4, V=20, seed=4):
    from re2nn_seq_amd import _lib
    rng = np.random.RandomState(seed)
    T = (rng.rand(V, S, S) < 0.1).astype(np.float32)
    W = (rng.rand(S, S) < 0.08).astype(np.float32)
    Oten = (rng.rand(C, S, S) < 0.3).astype(np.float32)
    h0 = np.eye(S, dtype=np.float32)[0]
    hT = (rng.rand(S) < 0.4).astype(np.float32)
    return _lib.create_onehot_ind1(T, W, Oten, h0, hT, o_idx=1), V


def _decomp(S=24, R=20, farnn=0, crf=False, semiring='sum', V=80, C=9):
    from re2nn_seq_amd import _lib, synth
    V, q, gates, tr = synth.snips_sized_model(R, farnn, crf, seed=11, S=S, V=V, C=C)
    return _lib.create_decomp_ifst(q['Vgen'], q['S1'], q['S2'], q['W'], q['Cout'], q['h0'], q['hT'], farnn=farnn, gates=gates,
                                   sigmoid_exponent=5, nl='tanh', semiring=semiring, threshold=0.5, o_idx=0, use_crf=crf,
                                   crf_trans=tr, device=0), V


def _factors(S, R, K, RO, V, seed):
    rng = np.random.RandomState(seed)
    f = lambda *shape, sc=0.3: (rng.randn(*shape) * sc).astype(np.float32)      # noqa: E731
    return rng, f, {'Vgen': f(V, R), 'S1': f(S, R), 'S2': f(S, R), 'W': (rng.rand(S, S) < 0.1).astype(np.float32) * 0.3,
                    'h0': np.eye(S, dtype=np.float32)[0], 'hT': (rng.rand(S) < 0.3).astype(np.float32)}


def _crf_tr(K, rng):
    from oracle import farnn_oracle as fo
    tr = fo.crf_default_transitions(K - 2) + (rng.randn(K, K) * 0.1).astype(np.float32)
    tr[:, K - 2] = -10000.0
    tr[K - 1, :] = -10000.0
    return tr


def _decomp1(S=23, R=12, RO=30, K=9, V=60, farnn=0, crf=False, seed=11):
    from re2nn_seq_amd import _lib, synth
    rng, f, p = _factors(S, R, K, RO, V, seed)
    gates = synth.exact_case_gates(S, R, farnn, rng) if farnn else None
    return _lib.create_decomp_ind1(p['Vgen'], p['S1'], p['S2'], p['W'], f(K, RO, sc=0.5), f(S, RO, sc=0.2), f(S, RO, sc=0.2),
                                   p['h0'], p['hT'], farnn=farnn, gates=gates, nl='tanh', o_idx=2, use_crf=crf,
                                   crf_trans=_crf_tr(K, rng) if crf else None), V


def _decomp0(S=23, R=60, RW=20, K=9, V=60, crf=False, seed=12):
    from re2nn_seq_amd import _lib
    rng, f, p = _factors(S, R, K, RW, V, seed)
    return _lib.create_decomp_fst(p['Vgen'], f(K, R), p['S1'], p['S2'], f(K, RW, sc=0.2), f(S, RW, sc=0.2), f(S, RW, sc=0.2),
                                  p['W'], p['h0'], p['hT'], nl='tanh', o_idx=2, use_crf=crf,
                                  crf_trans=_crf_tr(K, rng) if crf else None), V


BUILDERS = {'ifst': _ifst, 'compact': _compact, 'fst4': _fst4, 'ind1': _ind1, 'decomp': _decomp, 'decomp1': _decomp1,
            'decomp0': _decomp0}


def _c(name, branch, model='ifst', env=None, B=16, L=12, mode='local', out='tf', ab=False, **kw):
    """out: which outputs the call asks for -- t(ags), f(lat tags), s(cores)"""
    return dict(name=name, branch=branch, model=model, env=dict(env or {}), B=B, L=L, mode=mode, out=out, ab=ab, kw=kw)


CONFIGS = [
    # ---- onehot i-FST, S <= 72, sum semiring, label map
    _c('ifst_default_f16', 'chain_regs<f16 blocks, row80> + label-map score: the two-launch default'),
    _c('ifst_default_f32', 'chain_regs (no 16-bit image: a weight no f16 holds) + label-map score', inexact=True),
    _c('ifst_fuse', 'FARNN_FUSE=1: chain_regs with the label-map scores beside the recurrence, one launch', env={'FARNN_FUSE': '1'}),
    _c('ifst_nohalf', 'FARNN_NOHALF=1: chain_regs on the f32 blocks + label-map score', env={'FARNN_NOHALF': '1'}),
    _c('ifst_nolabelmap', 'FARNN_NOLABELMAP=1: chain_regs with the matrix-form scores beside the recurrence', env={'FARNN_NOLABELMAP': '1'}),
    _c('ifst_scores', 'scores asked for: chain_regs fused, matrix-form score tiles', out='tfs'),
    _c('ifst_priority', 'a priority matrix: no label-map path, matrix-form scores beside the recurrence', P=True),
    _c('ifst_row80_too_long', 'L = 220: the row80 carve exceeds 80 KiB, f16 blocks with hist rows of SP floats', B=4, L=220),
    _c('ifst_tiles_do_not_fit', 'S = 71, L = 210, scores: the score tiles do not fit beside a second workgroup, recurrence only + score_tile',
       S=71, B=4, L=210, out='tfs'),
    _c('ifst_regs_do_not_fit', 'S = 71, L = 300: the register-fed carve itself exceeds 80 KiB, chain_kernel', S=71, B=4, L=300),
    _c('ifst_nofuse', 'FARNN_NOFUSE=1 with scores: recurrence only + score_tile', env={'FARNN_NOFUSE': '1'}, out='tfs'),
    _c('ifst_max', 'max semiring: chain_regs without the destination split', semiring='max'),
    _c('ifst_nl_tanh', 'tanh between the steps', nl='tanh'),
    # ---- wide form
    _c('wide_paired', '72 < S <= 128, label map: chain_wide paired', S=100),
    _c('wide_unpaired', 'FARNN_WIDE_UNPAIRED=1: chain_wide, one workgroup per compute unit', S=100, env={'FARNN_WIDE_UNPAIRED': '1'}),
    _c('wide_scores', 'scores asked for: chain_wide fused with matrix-form tiles (not paired)', S=100, out='tfs'),
    _c('wide_rq11', 'S = 128 (RQ = 11): chain_wide, never paired', S=128),
    # ---- chain_kernel
    _c('noregs_fq1', 'FARNN_NOREGS=1, S = 5: chain_kernel<1, FQ = 1>', S=5, env={'FARNN_NOREGS': '1'}),
    _c('noregs_fq2', 'FARNN_NOREGS=1, S = 40: chain_kernel<1, FQ = 2>', S=40, env={'FARNN_NOREGS': '1'}),
    _c('noregs_fq3', 'FARNN_NOREGS=1, S = 71: chain_kernel<1, FQ = 3>', S=71, env={'FARNN_NOREGS': '1'}),
    _c('chain_fq0', 'S = 200 (beyond the register-fed forms): chain_kernel<1, FQ = 0>', S=200, V=30, B=4, L=8),
    _c('chain_nch2', 'S = 300: chain_kernel<2>', S=300, V=20, B=4, L=8),
    _c('chain_nch4', 'S = 520: chain_kernel<4>', S=520, V=12, B=4, L=8),
    # ---- CRF
    _c('crf_fused', 'CRF, tags only: recurrence + viterbi_hist_kernel<fused scores>', crf=True),
    _c('crf_unfused', 'FARNN_VITERBI_UNFUSED=1: score_tile + viterbi_hist_kernel', crf=True, env={'FARNN_VITERBI_UNFUSED': '1'}),
    _c('crf_bp', 'FARNN_VITERBI_BP=1: score_tile + viterbi_kernel (stored back-pointers)', crf=True, env={'FARNN_VITERBI_BP': '1'}),
    _c('crf_scores', 'CRF with scores asked for: score_tile + viterbi_hist_kernel', crf=True, out='tfs'),
    _c('crf_k130', 'CRF, 128 labels (IB4 = 4, kch = 3)', crf=True, C=128, S=71, V=100),
    # ---- compact handle
    _c('compact_one_launch', 'compact_tag_kernel: one launch', model='compact'),
    _c('compact_nofuse', 'FARNN_NOFUSE=1: compact_chain + label-map score', model='compact', env={'FARNN_NOFUSE': '1'}),
    _c('compact_nw3_tanh', 'S = 71 (three bitmap words), tanh: compact_tag_kernel<3, 2>', model='compact', S=71, nl='tanh'),
    _c('compact_wide_rows', 'S = 130: beyond compact_tag, compact_chain + score_tile', model='compact', S=130, V=30),
    _c('compact_scores', 'scores asked for: compact_chain + score_tile', model='compact', out='tfs'),
    # ---- batch prep
    _c('prep_b2', 'B = 2: no launch order', B=2),
    _c('prep_b3', 'B = 3: the smallest batch that is ordered', B=3),
    _c('prep_forced', 'FARNN_PREP=1: batch_prep_small_kernel runs', env={'FARNN_PREP': '1'}),
    _c('prep_forced_tags_only', 'FARNN_PREP=1, tags only: the prep launch computes the order alone', env={'FARNN_PREP': '1'}, out='t'),
    _c('prep_nosort', 'FARNN_NOSORT=1', env={'FARNN_NOSORT': '1'}),
    _c('prep_nosort_forced_tags_only', 'FARNN_NOSORT=1 FARNN_PREP=1, tags only: nothing to prepare', env={'FARNN_NOSORT': '1', 'FARNN_PREP': '1'}, out='t'),
    _c('mode_full', 'FARNN_MODE_FULL', mode='full', out='ts'),
    _c('mode_re', 'FARNN_MODE_RE', mode='re', out='ts'),
    _c('flat_only', 'flat tags only', out='f'),
    _c('prep_b1030_flat', 'B = 1030 with a flat output: batch_prep_kernel, no one-launch forms without offsets', B=1030, L=8),
    _c('prep_b1030_fuse', 'B = 1030, FARNN_FUSE=1, flat output: the offsets come from the prep launch', B=1030, L=8, env={'FARNN_FUSE': '1'}),
    # ---- FST4 / IND1
    _c('fst4', 'chain + fst4_score_kernel', model='fst4', out='tfs'),
    _c('ind1', 'chain + ind1_score_kernel', model='ind1', out='tfs'),
    # ---- decomposed i-FST
    _c('decomp_regs_fused', 'farnn = 0, rank <= 64: decomp_regs fused', model='decomp', out='t'),
    _c('decomp_regs_scores', 'decomp_regs fused, scores and flat tags asked for', model='decomp', out='tfs'),
    _c('decomp_regs_crf', 'CRF: decomp_regs + viterbi fused', model='decomp', crf=True, out='t'),
    _c('decomp_regs_nofuse', 'FARNN_NOFUSE=1: decomp_regs + label-map score', model='decomp', env={'FARNN_NOFUSE': '1'}),
    _c('decomp_rows', 'rank 100: decomp_rows', model='decomp', R=100),
    _c('decomp_rows_gated', 'farnn = 2: decomp_rows', model='decomp', farnn=2, crf=True),
    _c('decomp_chain_gated_max', 'farnn = 1, max semiring: no packed rows, decomp_chain', model='decomp', farnn=1, semiring='max'),
    _c('decomp_noregs', 'FARNN_DECOMP_NOREGS=1: decomp_rows', model='decomp', env={'FARNN_DECOMP_NOREGS': '1'}),
    _c('decomp_rows_noregs', 'FARNN_ROWS_NOREGS=1, rank 100: decomp_rows without its register forms', model='decomp', R=100,
       env={'FARNN_ROWS_NOREGS': '1'}),
    _c('decomp_forced_prep', 'FARNN_PREP=1: decomp_regs behind a prep launch', model='decomp', env={'FARNN_PREP': '1'}),
    _c('decomp_dense', 'max semiring, farnn = 0: dense blocks', model='decomp', semiring='max'),
    _c('decomp_dense_crf', 'max semiring, CRF: dense blocks', model='decomp', semiring='max', crf=True),
    # ---- DECOMP0 / DECOMP1
    _c('decomp0', 'decomposed independent=0: recurrence + decomp0_score', model='decomp0', out='tfs'),
    _c('decomp0_crf', '... with the Viterbi tail', model='decomp0', crf=True),
    _c('decomp1_dense_bssp', 'decomposed independent=1, farnn = 0: dense blocks + the MFMA score', model='decomp1', out='tfs'),
    _c('decomp1_dense_plain', 'output rank 81: dense blocks + decomp1_score_kernel', model='decomp1', RO=81, out='tfs'),
    _c('decomp1_chain_bssp', 'farnn = 1: decomp_chain + the MFMA score, tags only (the offsets are still computed)', model='decomp1',
       farnn=1, out='t'),
    _c('decomp1_chain_full', 'farnn = 1, FARNN_MODE_FULL', model='decomp1', farnn=1, mode='full', out='ts'),
    _c('decomp1_crf', '... with the Viterbi tail', model='decomp1', crf=True),
    # ---- the forms of the A/B build
    _c('ab_cv_one', 'FARNN_CV_ONE=1: chain_viterbi, one launch', crf=True, C=40, env={'FARNN_CV_ONE': '1'}, ab=True),
    _c('ab_nodest', 'FARNN_NODEST=1: chain_regs without the destination split', env={'FARNN_NODEST': '1'}, ab=True),
]
assert len({c['name'] for c in CONFIGS}) == len(CONFIGS)


def record(cfg):
    """Create the handle under cfg's switches, make the one call, return the record."""
    import torch
    from re2nn_seq_amd import _lib, synth
    saved = {k: os.environ.get(k) for k in cfg['env']}
    os.environ.update(cfg['env'])
    try:
        h, V = BUILDERS[cfg['model']](**cfg['kw'])
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        B, L = cfg['B'], cfg['L']
        x, lengths = synth.random_batch(V, B, L, np.random.RandomState(B * 131 + L), min_len=1)
        n = int(lengths.sum())
        K = h.num_columns()
        dev = torch.device('cuda', 0)
        xd, ld = torch.from_numpy(x).to(dev), torch.from_numpy(lengths).to(dev)
        tags = torch.full((B, L), -7, dtype=torch.int32, device=dev)
        flat = torch.full((n,), -7, dtype=torch.int64, device=dev)
        scores = torch.zeros((B, L, K), dtype=torch.float32, device=dev)
        mode = {'local': _lib.MODE_LOCAL, 'full': _lib.MODE_FULL, 're': _lib.MODE_RE}[cfg['mode']]
        rec = {'branch': cfg['branch'],
               'before': [h.kernel_name(_lib.KERN_CHAIN), h.kernel_name(_lib.KERN_SCORE)]}
        h.set_profiling(1)
        h.tag(xd.data_ptr(), ld.data_ptr(), B, L, mode, tags.data_ptr() if 't' in cfg['out'] else None,
              flat.data_ptr() if 'f' in cfg['out'] else None, scores.data_ptr() if 's' in cfg['out'] else None,
              torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        rec['after'] = [h.kernel_name(_lib.KERN_CHAIN), h.kernel_name(_lib.KERN_SCORE)]
        rec['launches'] = [int(h.kernel_time(k)[1]) for k in (_lib.KERN_CHAIN, _lib.KERN_SCORE, _lib.KERN_PREP)]
        rec['bytes'] = [h.kernel_algorithmic_bytes(_lib.KERN_CHAIN, n), h.kernel_algorithmic_bytes(_lib.KERN_SCORE, n)]
        valid = (np.arange(L)[None, :] < lengths[:, None]) if cfg['mode'] == 'local' else np.ones((B, L), bool)
        got = tags.cpu().numpy()[valid] if 't' in cfg['out'] else flat.cpu().numpy().astype(np.int32)
        rec['tags_crc'] = zlib.crc32(np.ascontiguousarray(got).tobytes())
        rec['tags_distinct'] = int(np.unique(got).size)
        return rec
    finally:
        h.close()


def main():
    sys.path.insert(0, ROOT)
    from re2nn_seq_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    table = {}
    if os.path.exists(out):
        with open(out) as f:
            table = json.load(f)
    for cfg in CONFIGS:
        if cfg['ab'] != bool(_lib.ab_build()):
            continue
        table[cfg['name']] = record(cfg)
        print(cfg['name'], json.dumps(table[cfg['name']]), flush=True)
    with open(out, 'w') as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
