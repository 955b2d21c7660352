"""farnn_tag_vectors on a max-semiring handle (farnn_decomp_sf_max_create; FARNN_S_SF with train_mode='max' under
RE2NN_SF_MAX=1) on the GPU: token_blocks_kernel in front of the dense chain kernels (farnn 0) or the padded copy under
decomp_chain_kernel (farnn 1 / 2), against the reference's captured forward, against the id path bit for bit where the vectors
are rows of a word table, and against the float64 restatement (sf_max_tag_ref.py) at the edges of the new kernel's tile:
a workgroup owns a 128 x 128 tile of a token's block, ceil(S / 8)^2 of its threads 8 x 8 entries each, in rounds of 32 ranks."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import farnn_oracle as fo
from util import ns, assert_float_path
import sf_tag_ref as sr
import sf_max_tag_ref as smr

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
BLOCKS, TABLE = 'token_blocks_kernel', 'token_table_kernel'


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _outputs(B, L, K, total):
    return (torch.full((B, L), -7, dtype=torch.int32, device=DEV), torch.full((total,), -7, dtype=torch.int64, device=DEV),
            torch.full((B, L, K), np.nan, dtype=torch.float32, device=DEV))


def _call(fn, h, first, lengths, B, L):
    from re2nn_seq_amd import _lib
    ld = _d(lengths)
    tags, flat, scores = _outputs(B, L, h.num_columns(), int(np.clip(lengths, 0, L).sum()))
    fn(first.data_ptr(), ld.data_ptr(), B, L, _lib.MODE_LOCAL, tags.data_ptr(), flat.data_ptr(), scores.data_ptr(),
       torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize(DEV)
    return scores.cpu().numpy(), tags.cpu().numpy(), flat.cpu().numpy()


def tag_vectors(h, v, lengths):
    """(scores [B, L, K], tags [B, L], flat) of one farnn_tag_vectors call, as numpy"""
    return _call(h.tag_vectors, h, _d(v), lengths, v.shape[0], v.shape[1])


def tag_ids(h, x, lengths):
    return _call(h.tag, h, _d(x), lengths, x.shape[0], x.shape[1])


def model(R, farnn, S, crf=False, C=9, V=50, seed=3, priority=False):
    from re2nn_seq_amd import synth
    _, q, gates, tr = synth.snips_sized_model(R, farnn, crf, seed=seed, S=S, V=V, C=C)
    P = None
    if priority:
        K = q['Cout'].shape[0]
        P = np.eye(K, dtype=np.float32)
        P[1, 2] = -1.0
        P[3, 0] = -0.5
    return smr.as_max(q), gates, tr, P


def handles(q, gates, tr, P, ids=True):
    from re2nn_seq_amd import _lib
    kw = dict(P=P, farnn=q['farnn'], gates=gates, sigmoid_exponent=5, nl='tanh', threshold=0.5, o_idx=0,
              use_crf=tr is not None, crf_trans=tr, device=0)
    sf = _lib.create_decomp_sf_max(q['S1'], q['S2'], q['W'], q['Cout'], q['h0'], q['hT'], **kw)
    idh = _lib.create_decomp_ifst(q['Vgen'], q['S1'], q['S2'], q['W'], q['Cout'], q['h0'], q['hT'], semiring='max', **kw) if ids else None
    return sf, idh


def ragged(B, L, rng, kind='mixed'):
    if kind == 'ones':
        return np.ones(B, np.int64)
    if kind == 'full':
        return np.full(B, L, np.int64)
    ln = rng.randint(1, L + 1, size=B).astype(np.int64)
    ln[0] = L
    ln[-1] = 1 if B > 1 else L
    return ln


def check_against_restatement(q, tr, P, v, lengths, got, msg=''):
    """scores by the one float rule; tags equal the decode of the call's own scores (the decode is the same float32 expression)
    and the float64 decode wherever that is decided; -1 / zero rows at pads"""
    scores, tags, flat = got
    B, L, _ = v.shape
    Lm = int(lengths.max())
    valid = np.arange(L)[None, :] < lengths[:, None]
    s32, s64 = smr.restate(q, v, lengths, P), smr.restate(q, v, lengths, P, wide=True)
    assert_float_path(scores[:, :Lm][valid[:, :Lm]], s32[valid[:, :Lm]], s64[valid[:, :Lm]], tol=smr.TOL, err_msg=msg)
    assert np.all(tags[~valid] == -1) and np.all(scores[~valid] == 0.0), msg
    own = fo.decode_argmax(scores, 0.5, 0) if tr is None else fo.decode_crf(scores, lengths, tr, 0.5, 0)
    assert np.array_equal(own[valid], tags[valid].astype(np.int64)), msg
    assert np.array_equal(fo.flatten(tags, lengths).astype(np.int64), flat), msg
    ok = sr.decided(s64, lengths, 0.5, tr)
    ref = fo.decode_argmax(s64, 0.5, 0) if tr is None else fo.decode_crf(s64.astype(np.float32), lengths, tr, 0.5, 0)
    assert np.array_equal(tags[:, :Lm][ok].astype(np.int64), ref[ok]), msg


def route_of(farnn):
    return BLOCKS if farnn == 0 else TABLE


def check_route(sf, farnn, idh=None):
    from re2nn_seq_amd import _lib
    assert sf.kernel_name(_lib.KERN_TABLE) == route_of(farnn)
    if farnn:
        assert sf.kernel_name(_lib.KERN_CHAIN) == 'decomp_chain_kernel'
    else:
        assert 'decomp' not in sf.kernel_name(_lib.KERN_CHAIN) and sf.kernel_name(_lib.KERN_CHAIN).startswith('chain_')
    if idh is not None:
        assert idh.kernel_name(_lib.KERN_TABLE) == '' and idh.kernel_name(_lib.KERN_CHAIN) == sf.kernel_name(_lib.KERN_CHAIN)


# ---- (a) the reference's captured forward, through the Python mirror ------------------------------------------------------
@pytest.mark.parametrize('k', smr.configs())
def test_fixture_config(k, monkeypatch):
    from re2nn_seq_amd import _lib
    from re2nn_seq_amd.farnn.model_decompose_single import FARNN_S_SF
    monkeypatch.setenv('RE2NN_SF_MAX', '1')
    dmeta, _, g, f = smr.fixture()
    cfg = smr.config_of(dmeta, k)
    pre = 'c{}.'.format(k)
    m = FARNN_S_SF(S1=g['S1_in'], S2=g['S2_in'], C_output_mat=g['O_in'], wildcard_mat=g['W_in'], wildcard_output_vector=g['Ow_in'],
                   final_vector=g['final_in'], start_vector=g['start_in'], priority_mat=g['priority_in'],
                   args=ns(independent=2, threshold=dmeta['threshold'], **cfg), o_idx=dmeta['o_idx'])
    sd = {key[len(pre):]: g[key] for key in g.files if key.startswith(pre)}
    sd['priority_layer.priority_mat'] = sd.pop('priority_mat')
    if 'crf_transitions' in sd:
        sd['crf.transitions'] = sd.pop('crf_transitions')
    m.load_state_dict(sd)
    v, lengths = f['v'], f['lengths']
    B, L, _ = v.shape
    r = m.run_vectors(torch.from_numpy(v), torch.from_numpy(lengths), want_tags=True, want_flat=True, want_scores=True)
    torch.cuda.synchronize(DEV)
    scores, tags, flat = r['scores'].cpu().numpy(), r['tags'].cpu().numpy(), r['flat'].cpu().numpy()
    assert m.handle.kernel_name(_lib.KERN_TABLE) == route_of(cfg.get('farnn', 0))
    p = smr.params_from_fixture(g, k, cfg)
    P = g[pre + 'priority_mat'] if cfg.get('use_priority', 0) else None
    s32, s64 = smr.restate(p, v, lengths, P), smr.restate(p, v, lengths, P, wide=True)
    valid = np.arange(L)[None, :] < lengths[:, None]
    assert_float_path(scores[valid], s32[valid], s64[valid], tol=smr.TOL)
    assert_float_path(scores[valid], f[pre + 'scores'][valid], s64[valid], tol=smr.TOL)
    tr = g[pre + 'crf_transitions'] if cfg.get('use_crf', 0) else None
    ok = sr.decided(s64, lengths, dmeta['threshold'], tr)
    assert 1.0 - ok[valid].mean() <= smr.UNDECIDED_CAP
    keep = sr.flat_mask(ok, lengths)
    assert np.array_equal(flat[keep], f[pre + 'flat_pred'][keep])
    assert np.array_equal(fo.flatten(tags, lengths).astype(np.int64), flat)
    assert np.all(tags[~valid] == -1) and np.all(scores[~valid] == 0.0)
    # the mirror's own call: a longer, non-contiguous, float64 input is handled on the host
    wide = np.zeros((B, L + 3, 2 * v.shape[2]))
    wide[:, :L, ::2] = v
    label = torch.zeros((B, L + 3), dtype=torch.int64)
    loss, pred, true = m(torch.from_numpy(wide)[:, :, ::2], label, torch.from_numpy(lengths), train=False)
    assert loss is None and np.array_equal(pred.numpy(), flat) and true.shape == pred.shape
    with pytest.raises(NotImplementedError, match='f14'):
        m(torch.from_numpy(v), label[:, :L], torch.from_numpy(lengths), train=True)


# ---- (b) v = Vgen[x]: bit for bit the id path ------------------------------------------------------------------------------
IDENTITY = {
    'dense_regs':     dict(R=40, farnn=0, S=33),
    'dense_wide':     dict(R=70, farnn=0, S=104),
    'dense_chain':    dict(R=33, farnn=0, S=160),          # beyond the register-fed kernels: chain_kernel, two tiles a side
    'dense_crf':      dict(R=70, farnn=0, S=20, crf=True),
    'dense_priority': dict(R=40, farnn=0, S=33, priority=True),
    'gated1':         dict(R=70, farnn=1, S=20),
    'gated2':         dict(R=100, farnn=2, S=71),
    'gated1_crf':     dict(R=40, farnn=1, S=33, crf=True),
    'gated2_crf':     dict(R=70, farnn=2, S=20, crf=True),
}


def identity_case(q, gates, tr, P, B, L, seed, kind='mixed', msg=''):
    from re2nn_seq_amd import synth
    sf, idh = handles(q, gates, tr, P)
    rng = np.random.RandomState(seed)
    V = q['Vgen'].shape[0]
    x, _ = synth.random_batch(V, B, L, rng, min_len=1)
    lengths = ragged(B, L, rng, kind)
    v = q['Vgen'][x]                                      # pads: the pad word's row -- never read
    a, b = tag_vectors(sf, v, lengths), tag_ids(idh, x, lengths)
    for got, ref, what in zip(a, b, ('scores', 'tags', 'flat tags')):
        assert np.array_equal(got, ref), '{}: {} differ from farnn_tag'.format(msg, what)
    check_route(sf, q['farnn'], idh)
    sf.close(); idh.close()
    return v, lengths, a


@pytest.mark.parametrize('case', sorted(IDENTITY))
def test_identity_with_the_id_path(case):
    q, gates, tr, P = model(**IDENTITY[case])
    _, _, a = identity_case(q, gates, tr, P, 5, 13, 11, msg=case)
    assert np.abs(a[0]).max() > 0.0


# ---- (c) edges of the new kernel and its hand-over ----------------------------------------------------------------------
# S: both sides of 8 k (a thread row more), of 64 / 72 (the register-fed kernels' widths) and of the 128-wide tile; R: both sides of
# the 32-rank round.  Each case: rows of a table against the id path bit for bit and the restatement, then vectors of no table
# against the restatement.
def _edge(R, S, farnn, B, L, kind, seed=0, crf=False):
    q, gates, tr, P = model(R=R, farnn=farnn, S=S, crf=crf, seed=5 + seed)
    msg = str((R, S, farnn, B, L, kind))
    v, lengths, got = identity_case(q, gates, tr, P, B, L, 100 + seed, kind, msg)
    check_against_restatement(q, tr, P, v, lengths, got, msg)
    sf, _ = handles(q, gates, tr, P, ids=False)
    rng = np.random.RandomState(200 + seed)
    v = (rng.randn(B, L, R) * float(np.abs(q['Vgen']).std()) * 1.5).astype(np.float32)
    check_against_restatement(q, tr, P, v, lengths, tag_vectors(sf, v, lengths), msg)
    check_route(sf, farnn)
    sf.close()


@pytest.mark.parametrize('R', [1, 5, 31, 32, 33, 65])
@pytest.mark.parametrize('S', [3, 33, 64, 65, 72, 73, 127, 128, 129])
def test_edges_rank_and_states(R, S):
    _edge(R, S, 0, B=3, L=5, kind='mixed', seed=R + S)


@pytest.mark.parametrize('S', [3, 33])
def test_edges_rank_and_states_gated(S):
    for R in (1, 5, 32, 33, 65):
        for farnn in (1, 2):
            _edge(R, S, farnn, B=3, L=5, kind='mixed', seed=R + S + farnn)


@pytest.mark.parametrize('L', [1, 5, 64, 65])
@pytest.mark.parametrize('B', [1, 2, 37])
def test_edges_batch_and_length(B, L):
    _edge(33, 33, 0, B, L, 'mixed', seed=B + L)
    _edge(5, 3, 2, B, L, 'mixed', seed=B + L + 1)


@pytest.mark.parametrize('kind', ['ones', 'full', 'mixed'])
def test_edges_length_patterns(kind):
    _edge(65, 73, 0, 37, 5, kind)
    _edge(32, 3, 0, 3, 65, kind, crf=True)
    _edge(33, 33, 1, 37, 5, kind)


# ---- (d) pad rows of v are never read -------------------------------------------------------------------------------------
@pytest.mark.parametrize('farnn', [0, 2])
def test_nan_in_pad_rows(farnn):
    q, gates, tr, P = model(R=33, farnn=farnn, S=33)
    sf, _ = handles(q, gates, tr, P, ids=False)
    rng = np.random.RandomState(8)
    B, L = 37, 9
    lengths = ragged(B, L, rng)
    valid = np.arange(L)[None, :] < lengths[:, None]
    v0 = (rng.randn(B, L, 33) * 0.3).astype(np.float32)
    v0[~valid] = 0.0
    v1 = v0.copy()
    v1[~valid] = np.nan
    a = tag_vectors(sf, v0, lengths)
    b = tag_vectors(sf, v1, lengths)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)                       # (pads included: -1 tags, zero score rows)
    assert np.isfinite(b[0]).all()
    # a handle whose FIRST call brings the NaNs (nothing left behind by a clean one)
    fresh, _ = handles(q, gates, tr, P, ids=False)
    for x, y in zip(a, tag_vectors(fresh, v1, lengths)):
        assert np.array_equal(x, y)
    sf.close(); fresh.close()


# ---- (e) reserve, calls within the bounds, regrowth; the same call twice ---------------------------------------------------
@pytest.mark.parametrize('farnn', [0, 2])
def test_reserve_and_regrowth(farnn):
    q, gates, tr, P = model(R=33, farnn=farnn, S=33)
    rng = np.random.RandomState(9)
    calls = []
    for B, L in ((7, 11), (4, 20), (40, 33)):
        lengths = ragged(B, L, rng)
        calls.append(((rng.randn(B, L, 33) * 0.3).astype(np.float32), lengths))
    fresh = []
    for v, lengths in calls:
        h, _ = handles(q, gates, tr, P, ids=False)
        fresh.append(tag_vectors(h, v, lengths))
        h.close()
    h, _ = handles(q, gates, tr, P, ids=False)
    h.reserve(8, 20)
    torch.cuda.synchronize(DEV)
    free0 = torch.cuda.mem_get_info(DEV)[0]
    got = [tag_vectors(h, *calls[0]), tag_vectors(h, *calls[1])]
    assert torch.cuda.mem_get_info(DEV)[0] == free0, 'a call within the reserved bounds allocated device memory'
    got.append(tag_vectors(h, *calls[2]))                 # larger than anything before: the workspace regrows
    got.append(tag_vectors(h, *calls[0]))                 # and a smaller call again, on the regrown workspace
    for g_, f_ in zip(got, fresh + [fresh[0]]):
        for x, y in zip(g_, f_):
            assert np.array_equal(x, y)
    check_route(h, farnn)
    h.close()


@pytest.mark.parametrize('farnn', [0, 1])
def test_the_same_call_twice_gives_the_same_bits(farnn):
    q, gates, tr, P = model(R=65, farnn=farnn, S=73)
    sf, _ = handles(q, gates, tr, P, ids=False)
    rng = np.random.RandomState(10)
    lengths = ragged(37, 9, rng)
    v = (rng.randn(37, 9, 65) * 0.3).astype(np.float32)
    a, b = tag_vectors(sf, v, lengths), tag_vectors(sf, v, lengths)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    sf.close()


# ---- (f) refusals ---------------------------------------------------------------------------------------------------------
def _raw_create(entry, q, V=0, vgen=None, semiring='max'):
    from re2nn_seq_amd import _lib
    a = {k: _lib.f32(q[k]) for k in ('S1', 'S2', 'W', 'Cout', 'h0', 'hT')}
    vg = None if vgen is None else _lib.f32(vgen)
    S, R = a['S1'].shape
    d = _lib.DecompIfstDesc(V, S, R, a['Cout'].shape[0], _lib.ptr(vg), _lib.ptr(a['S1']), _lib.ptr(a['S2']), _lib.ptr(a['W']),
                            _lib.ptr(a['Cout']), _lib.ptr(a['h0']), _lib.ptr(a['hT']), None, 0, None, None, None, None, None, None,
                            5.0, _lib.NL['tanh'], _lib.SEMIRING[semiring], 0.5, 0, 0, None, 0)
    out = C.c_void_p()
    rc = getattr(_lib.load(), entry)(C.byref(d), 0, C.byref(out))
    assert rc != 0 and not out.value
    return rc


def test_refusals():
    from re2nn_seq_amd import _lib
    q, gates, tr, P = model(R=33, farnn=0, S=33)
    assert _raw_create('farnn_decomp_sf_max_create', q, semiring='sum') == -22
    assert _raw_create('farnn_decomp_sf_max_create', q, V=q['Vgen'].shape[0]) == -22
    assert _raw_create('farnn_decomp_sf_max_create', q, vgen=q['Vgen']) == -22
    assert _raw_create('farnn_decomp_sf_max_create', q, V=q['Vgen'].shape[0], vgen=q['Vgen']) == -22
    assert _raw_create('farnn_decomp_sf_create', q, semiring='max') == -22            # the sum entry still refuses max
    with pytest.raises(_lib.FarnnError, match='code -22.*max semiring'):
        _lib.create_decomp_sf(q['S1'], q['S2'], q['W'], q['Cout'], q['h0'], q['hT'], farnn=0, semiring='max')
    sf, idh = handles(q, gates, tr, P)
    B, L = 2, 4
    v, x, ln = _d(np.zeros((B, L, 33), np.float32)), _d(np.zeros((B, L), np.int64)), _d(np.array([4, 2], np.int64))
    tags = torch.zeros((B, L), dtype=torch.int32, device=DEV)
    for mode in (_lib.MODE_FULL, _lib.MODE_RE):
        with pytest.raises(_lib.FarnnError, match='code -22.*LOCAL'):
            sf.tag_vectors(v.data_ptr(), ln.data_ptr(), B, L, mode, tags.data_ptr())
    with pytest.raises(_lib.FarnnError, match='code -22.*farnn_tag_vectors'):
        sf.tag(x.data_ptr(), ln.data_ptr(), B, L, _lib.MODE_LOCAL, tags.data_ptr())
    with pytest.raises(_lib.FarnnError, match='code -22.*farnn_tag'):
        idh.tag_vectors(v.data_ptr(), ln.data_ptr(), B, L, _lib.MODE_LOCAL, tags.data_ptr())
    with pytest.raises(_lib.FarnnError, match='code -22'):
        sf.tag_vectors(None, ln.data_ptr(), B, L, _lib.MODE_LOCAL, tags.data_ptr())
    sf.close(); idh.close()
