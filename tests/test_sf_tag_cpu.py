"""The vector-input tagger (FARNN_S_SF) without a device: the restatement through the existing oracle (sf_tag_ref.py) against
the reference's captured forward, the EmbedAggregator mirror against its captured output, the refusals that need no device, and
the ctypes signatures of the two new entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import farnn_oracle as fo
from util import ns, assert_float_path
import sf_tag_ref as sr


@pytest.mark.parametrize('k', sr.sf_configs())
def test_restatement_matches_the_reference(k):
    dmeta, _, g, f = sr.fixture()
    cfg = dmeta['configs'][k]
    pre = 'c{}.'.format(k)
    v, lengths = f['v'], f['lengths']
    p = sr.params_from_fixture(g, k, cfg)
    P = g[pre + 'priority_mat'] if cfg.get('use_priority', 0) else None
    s32, s64 = sr.restate(p, v, lengths, P), sr.restate(p, v, lengths, P, wide=True)
    ref = f[pre + 'scores']
    assert ref.shape == s32.shape == (v.shape[0], int(lengths.max()), p['Cout'].shape[0])
    assert_float_path(ref, s32, s64, tol=sr.TOL, err_msg='config {}'.format(k))
    tr = g[pre + 'crf_transitions'] if cfg.get('use_crf', 0) else None
    ok = sr.decided(s64, lengths, dmeta['threshold'], tr)
    valid = np.arange(v.shape[1])[None, :] < lengths[:, None]
    assert 1.0 - ok[valid].mean() <= sr.UNDECIDED_CAP
    tags = fo.forward_local_tags(s32, lengths, dmeta['threshold'], dmeta['o_idx'], tr)
    keep = sr.flat_mask(ok, lengths)
    assert np.array_equal(tags[keep], f[pre + 'flat_pred'][keep])


def test_inputs_are_ragged_and_rows_of_no_table():
    dmeta, _, g, f = sr.fixture()
    v, lengths = f['v'], f['lengths']
    assert lengths.min() == 1 and lengths.max() == v.shape[1] and len(set(lengths.tolist())) > 2
    table = fo.generalized_vocab_table(g['c0.V_embed'], g['c0.embedding'], g['c0.embed_r_generalized'], g['c0.beta_vec'])
    assert v.shape[2] == table.shape[1]
    d = np.abs(v.reshape(-1, 1, v.shape[2]) - table[None]).max(-1)
    assert d.min() > 0.1


def _aggregator(g, cfg):
    from re2nn_seq_amd.farnn.embed_aggregator import EmbedAggregator
    return EmbedAggregator(ns(independent=2, **cfg), g['V_in'], g['E_in'])


def test_embed_aggregator_matches_the_reference():
    dmeta, smeta, g, f = sr.fixture()
    x, lx = torch.from_numpy(g['x']), torch.from_numpy(g['lengths'])
    assert len(smeta['agg']) >= 4
    for k in map(int, smeta['agg']):
        agg = _aggregator(g, dmeta['configs'][k])
        np.testing.assert_allclose(agg.embed_r_generalized.numpy(), f['agg{}.embed_r_generalized'.format(k)], rtol=1e-4, atol=1e-5)
        out = agg(x, lx).numpy()
        ref = f['agg{}.out'.format(k)]
        assert out.shape == ref.shape == (x.shape[0], int(lx.max()), g['V_in'].shape[1])
        np.testing.assert_allclose(out, ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('k', sr.sf_configs())
def test_aggregate_then_sf_is_the_id_model(k):
    """EmbedAggregator.forward on word ids, then the vector-input model, equals FARNN_S_D_W_I_S on those ids (the reference's
    captured scores of decomp_small): the two taggers differ in where the vector comes from, nothing else."""
    dmeta, _, g, _ = sr.fixture()
    cfg = dmeta['configs'][k]
    pre = 'c{}.'.format(k)
    x, lengths = g['x'], g['lengths']
    agg = _aggregator(g, cfg)
    agg.embed_r_generalized = torch.from_numpy(g[pre + 'embed_r_generalized'])     # the captured model's own bridge
    v = agg(torch.from_numpy(x), torch.from_numpy(lengths)).numpy()
    p = sr.params_from_fixture(g, k, cfg)
    P = g[pre + 'priority_mat'] if cfg.get('use_priority', 0) else None
    np.testing.assert_allclose(sr.restate(p, v, lengths, P), g[pre + 'scores'], rtol=1e-4, atol=1e-4)


def test_forward_bert_takes_any_callable():
    dmeta, _, g, _ = sr.fixture()
    from re2nn_seq_amd.farnn.embed_aggregator import EmbedAggregator
    x, lx = torch.from_numpy(g['x']), torch.from_numpy(g['lengths'])
    E = torch.from_numpy(g['E_in']).float()
    seen = []

    def encoder(bert_input, attend, valid, lengths):
        seen.append((bert_input, attend, valid))
        return E[x[:, :int(lengths.max())]]
    a = ns(independent=2, **dmeta['configs'][7])
    agg = EmbedAggregator(a, g['V_in'], g['E_in'], encoder=encoder)
    out = agg.forward_bert(x, 'ids', 'attend', 'valid', lx)
    assert seen == [('ids', 'attend', 'valid')]
    assert torch.equal(out, agg(x, lx))                    # an encoder that returns the static embeddings: forward itself
    with pytest.raises(ValueError):
        EmbedAggregator(a, g['V_in'], g['E_in']).forward_bert(x, None, None, None, lx)


def _sf(g, cfg, **kw):
    from re2nn_seq_amd.farnn.model_decompose_single import FARNN_S_SF
    return FARNN_S_SF(S1=g['S1_in'], S2=g['S2_in'], C_output_mat=g['O_in'], wildcard_mat=g['W_in'], wildcard_output_vector=g['Ow_in'],
                      final_vector=g['final_in'], start_vector=g['start_in'], priority_mat=g['priority_in'],
                      args=ns(independent=2, **dict(cfg, **kw)), o_idx=0)


def test_mirror_builds_the_reference_parameter_set():
    dmeta, _, g, _ = sr.fixture()
    for k in sr.sf_configs():
        cfg = dmeta['configs'][k]
        m = _sf(g, cfg)
        pre = 'c{}.'.format(k)
        for key in m._param_keys:
            assert hasattr(m, key) == (pre + key in g.files), (k, key)
            if hasattr(m, key):
                assert tuple(getattr(m, key).shape) == g[pre + key].shape, (k, key)
        assert not hasattr(m, 'V_embed') and not hasattr(m, 'embed_r_generalized')


def test_refusals_without_a_device(monkeypatch):
    dmeta, _, g, f = sr.fixture()
    m = _sf(g, dmeta['configs'][0])
    v, ln = torch.from_numpy(f['v']), torch.from_numpy(f['lengths'])
    with pytest.raises(NotImplementedError, match='f14'):
        m.forward(v, torch.zeros(v.shape[:2], dtype=torch.int64), ln, train=True)
    with pytest.raises(NotImplementedError, match='max'):
        _sf(g, dmeta['configs'][0], train_mode='max')
    from re2nn_seq_amd import main, init_params
    import argparse
    with pytest.raises(NotImplementedError, match=r'FARNN_S_bert\(encoder='):
        main.dispatch(argparse.Namespace(method='decompose', use_bert=1))
    import inspect
    assert 'FARNN_S_bert(encoder=' in inspect.getsource(init_params)
    for fn in (m.forward_RE, m.forward_score, m.submit_local):
        with pytest.raises(NotImplementedError):
            fn()


def test_bert_composition_constructs():
    from re2nn_seq_amd.farnn.model_decompose_single import FARNN_S_bert, FARNN_S_SF
    from re2nn_seq_amd.farnn.embed_aggregator import EmbedAggregator
    dmeta, _, g, _ = sr.fixture()
    m = FARNN_S_bert(V=g['V_in'], S1=g['S1_in'], S2=g['S2_in'], C_output_mat=g['O_in'], wildcard_mat=g['W_in'],
                     wildcard_output_vector=g['Ow_in'], final_vector=g['final_in'], start_vector=g['start_in'],
                     static_embed=g['E_in'], priority_mat=g['priority_in'], args=ns(independent=2, **dmeta['configs'][4]),
                     encoder=lambda *a: None)
    assert isinstance(m.embed, EmbedAggregator) and isinstance(m.slot_filler, FARNN_S_SF)


def test_ctypes_signatures():
    from re2nn_seq_amd import _lib
    vp = C.c_void_p
    assert _lib.SIGNATURES['farnn_decomp_sf_create'] == (C.c_int, [C.POINTER(_lib.DecompIfstDesc), C.c_int, C.POINTER(vp)])
    assert _lib.SIGNATURES['farnn_tag_vectors'] == (C.c_int, [vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp])
    assert _lib.SIGNATURES['farnn_tag_vectors'] == _lib.SIGNATURES['farnn_tag']      # same shape of call, v in place of x
    assert _lib.KERN_TABLE == 3
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, 'farnn_decomp_sf_create') and hasattr(lib, 'farnn_tag_vectors')
    assert callable(_lib.create_decomp_sf) and callable(_lib.Handle.tag_vectors)
