"""The vector-input tagger in the max semiring (FARNN_S_SF, train_mode='max') without a device: the oracle restatement
(sf_max_tag_ref.py) against the reference's captured forward, the fixture's own cap on undecided positions, the opt-in switch
RE2NN_SF_MAX of the Python mirror and the ctypes signature of the new entry point."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import farnn_oracle as fo
from util import ns, assert_float_path
import sf_tag_ref as sr
import sf_max_tag_ref as smr


@pytest.mark.parametrize('k', smr.configs())
def test_restatement_matches_the_reference(k):
    dmeta, _, g, f = smr.fixture()
    cfg = smr.config_of(dmeta, k)
    pre = 'c{}.'.format(k)
    v, lengths = f['v'], f['lengths']
    p = smr.params_from_fixture(g, k, cfg)
    assert p['semiring'] == fo.SEMIRING_MAX
    P = g[pre + 'priority_mat'] if cfg.get('use_priority', 0) else None
    s32, s64 = smr.restate(p, v, lengths, P), smr.restate(p, v, lengths, P, wide=True)
    ref = f[pre + 'scores']
    assert ref.shape == s32.shape == (v.shape[0], int(lengths.max()), p['Cout'].shape[0])
    assert_float_path(ref, s32, s64, tol=smr.TOL, err_msg='config {}'.format(k))
    tr = g[pre + 'crf_transitions'] if cfg.get('use_crf', 0) else None
    ok = sr.decided(s64, lengths, dmeta['threshold'], tr)
    tags = fo.forward_local_tags(s32, lengths, dmeta['threshold'], dmeta['o_idx'], tr)
    keep = sr.flat_mask(ok, lengths)
    assert np.array_equal(tags[keep], f[pre + 'flat_pred'][keep])
    # the max semiring is not the sum semiring on these inputs: the fixture would catch a handle that ran the wrong one
    sum_scores = sr.restate(dict(p, semiring=fo.SEMIRING_SUM), v, lengths, P, wide=True)
    assert np.abs(sum_scores - s64).max() > 100 * smr.TOL


@pytest.mark.parametrize('k', smr.configs())
def test_fixture_stays_under_the_undecided_cap(k):
    """the generator's own check, re-run on the committed files"""
    dmeta, _, g, f = smr.fixture()
    v, lengths = f['v'], f['lengths']
    ok = smr.decided_positions(g, k, smr.config_of(dmeta, k), dmeta, v, lengths)
    valid = np.arange(v.shape[1])[None, :] < lengths[:, None]
    assert not ok[~valid].any()
    assert 1.0 - ok[valid].mean() <= smr.UNDECIDED_CAP


def test_fixture_spans_the_model_family():
    dmeta, smeta, _, f = smr.fixture()
    cfgs = [dmeta['configs'][k] for k in smeta['configs']]
    assert len(cfgs) >= 6 and smeta['train_mode'] == 'max'
    assert {c.get('farnn', 0) for c in cfgs} == {0, 1, 2}
    assert {c.get('update_nonlinear', 'none') for c in cfgs} == {'none', 'relu', 'tanh', 'relutanh'}
    assert any(c.get('use_crf', 0) for c in cfgs) and any(c.get('use_priority', 0) for c in cfgs)
    lengths = f['lengths']
    assert f['v'].shape[:2] == (7, 9) and lengths.min() == 1 and lengths.max() == 9


def _sf(g, cfg, **kw):
    from re2nn_seq_amd.farnn.model_decompose_single import FARNN_S_SF
    return FARNN_S_SF(S1=g['S1_in'], S2=g['S2_in'], C_output_mat=g['O_in'], wildcard_mat=g['W_in'], wildcard_output_vector=g['Ow_in'],
                      final_vector=g['final_in'], start_vector=g['start_in'], priority_mat=g['priority_in'],
                      args=ns(independent=2, **dict(cfg, **kw)), o_idx=0)


def test_switch_opens_the_constructor_and_training_stays_refused(monkeypatch):
    dmeta, _, g, f = smr.fixture()
    monkeypatch.setenv('RE2NN_SF_MAX', '1')
    m = _sf(g, dmeta['configs'][0], train_mode='max')
    assert m.args.train_mode == 'max'
    v, ln = torch.from_numpy(f['v']), torch.from_numpy(f['lengths'])
    label = torch.zeros(v.shape[:2], dtype=torch.int64)
    with pytest.raises(NotImplementedError, match='f14'):
        m.forward(v, label, ln, train=True)
    monkeypatch.setenv('RE2NN_SF_TRAIN', '1')              # the sum semiring's training switch does not open it either
    with pytest.raises(NotImplementedError, match='f14'):
        m.forward(v, label, ln, train=True)


def test_bert_composition_passes_the_mode_through(monkeypatch):
    from re2nn_seq_amd.farnn.model_decompose_single import FARNN_S_bert
    dmeta, _, g, _ = smr.fixture()
    kw = dict(V=g['V_in'], S1=g['S1_in'], S2=g['S2_in'], C_output_mat=g['O_in'], wildcard_mat=g['W_in'],
              wildcard_output_vector=g['Ow_in'], final_vector=g['final_in'], start_vector=g['start_in'],
              static_embed=g['E_in'], priority_mat=g['priority_in'],
              args=ns(independent=2, **dict(dmeta['configs'][4], train_mode='max')), encoder=lambda *a: None)
    monkeypatch.delenv('RE2NN_SF_MAX', raising=False)
    with pytest.raises(NotImplementedError, match='max'):
        FARNN_S_bert(**kw)
    monkeypatch.setenv('RE2NN_SF_MAX', '1')
    assert FARNN_S_bert(**kw).slot_filler.args.train_mode == 'max'


@pytest.mark.parametrize('value', [None, '', '0', 'true'])
def test_without_the_switch_the_constructor_raises_as_before(monkeypatch, value):
    dmeta, _, g, _ = smr.fixture()
    if value is None:
        monkeypatch.delenv('RE2NN_SF_MAX', raising=False)
    else:
        monkeypatch.setenv('RE2NN_SF_MAX', value)
    with pytest.raises(NotImplementedError) as e:
        _sf(g, dmeta['configs'][0], train_mode='max')
    assert str(e.value) == ('FARNN_S_SF: --train_mode max needs an S x S block per token; the vector-input tagger exists '
                            'in the sum semiring only (DESIGN.md, row f14)')


def test_ctypes_signature_and_export():
    from re2nn_seq_amd import _lib
    assert _lib.SIGNATURES['farnn_decomp_sf_max_create'] == _lib.SIGNATURES['farnn_decomp_sf_create']
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, 'farnn_decomp_sf_max_create')
    assert callable(_lib.create_decomp_sf_max)
    with pytest.raises(TypeError):                         # the max entry takes no semiring: it is its own
        _lib.create_decomp_sf_max(None, None, None, None, None, None, semiring='sum')
