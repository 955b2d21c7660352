"""The five trainable mirrors at one tiny shape, for tests/test_trainable_surface_cpu.py and tests/test_gpu_trainable_surface.py:
V = 5 words, S = 4 states, C = 3 labels, and for the decomposed models rank R = 3, output rank R_O = 2, embedding width D = 4."""
import numpy as np
import torch

from util import ns

V, S, C, R, R_O, D = 5, 4, 3, 3, 2, 4
KINDS = ('onehot_ifst', 'onehot_fst', 'onehot_ind1', 'decomp_ifst', 'decomp_ind1')
# each model's own opt-in (the onehot and the decomposed i-FST train without one)
SWITCH = {'onehot_fst': 'RE2NN_ONEHOT_FST_TRAIN', 'onehot_ind1': 'RE2NN_ONEHOT_IND1_TRAIN', 'decomp_ind1': 'RE2NN_DECOMP_IND1_TRAIN'}
ALL_SWITCHES = ('RE2NN_ONEHOT_MAX_TRAIN', 'RE2NN_ONEHOT_FST_TRAIN', 'RE2NN_ONEHOT_IND1_TRAIN', 'RE2NN_BUCKETED_MAX_TRAIN',
                'RE2NN_DECOMP_IND1_TRAIN', 'RE2NN_DECOMP_IND1_CRF_TRAIN', 'RE2NN_DECOMP_TEACHER_TRAIN',
                'RE2NN_DECOMP_TEACHER_MAX_TRAIN', 'RE2NN_NATIVE_OPTIM')


def cls_of(kind):
    from re2nn_seq_amd.farnn import model_decompose_independent, model_decompose_single, model_onehot
    return {'onehot_ifst': model_onehot.FARNN_S_O_I_S, 'onehot_fst': model_onehot.FARNN_S_O, 'onehot_ind1': model_onehot.FARNN_S_O_I,
            'decomp_ifst': model_decompose_single.FARNN_S_D_W_I_S, 'decomp_ind1': model_decompose_independent.FARNN_S_D_W_I}[kind]


def build(kind, seed=0, **kw):
    """The model of that kind on random weights in (0.1, 0.9); kw are fields of `args` (tests/util.py ns).  beta = 0.7 (so that
    embed_r_generalized and embedding.weight have a gradient) and bias_init = 0 (gates that are not saturated) unless kw says otherwise."""
    kw = dict(dict(beta=0.7, bias_init=0.0), **kw)
    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)                              # the gates of --farnn 1 / 2 are drawn by the constructor
    u = lambda *shape: rng.uniform(0.1, 0.9, size=shape).astype(np.float32)      # noqa: E731
    h0, hT = u(S), u(S)
    cls = cls_of(kind)
    if kind == 'onehot_ifst':
        return cls(u(V, S, S), u(C, S), u(S, S), np.zeros(S), hT, h0, None, ns(**kw), o_idx=0)
    if kind == 'onehot_fst':
        return cls(u(V, C, S, S), u(C, S, S), np.zeros((S, S)), hT, h0, None, ns(independent=0, **kw), o_idx=0)
    if kind == 'onehot_ind1':
        return cls(u(V, S, S), u(C, S, S), u(S, S), None, hT, h0, None, ns(independent=1, **kw), o_idx=0)
    common = dict(V=u(V, R), S1=u(S, R), S2=u(S, R), wildcard_mat=u(S, S), final_vector=hT, start_vector=h0,
                  pretrained_word_embed=u(V, D), priority_mat=None, o_idx=0)
    if kind == 'decomp_ifst':
        return cls(C_output_mat=u(C, S), wildcard_output_vector=np.zeros(S, np.float32), args=ns(**kw), **common)
    return cls(C_output=u(C, R_O), S1_output=u(S, R_O), S2_output=u(S, R_O), wildcard_output=None,
               args=ns(independent=1, **kw), **common)


def build_edge_ifst(**kw):
    """FARNN_S_O_I_S as from_automaton leaves it: the automaton's edges (word -1: a wildcard edge) and no dense tensor"""
    from re2nn_seq_amd.farnn.model_onehot import FARNN_S_O_I_S, _OnehotBase
    m = FARNN_S_O_I_S.__new__(FARNN_S_O_I_S)
    _OnehotBase.__init__(m, ns(**kw), 0, C, None, False)
    m.S, m.V = S, V
    m.h0, m.hT = np.eye(S, dtype=np.float32)[0], np.ones(S, np.float32)
    i32 = lambda *a: np.array(a, np.int32)               # noqa: E731
    m.edges = (i32(0, 1, 2, 3, 4, -1, -1), i32(0, 1, 2, 0, 1, 3, 0), i32(1, 2, 3, 2, 3, 0, 0), i32(1, 2, 1, 2, 1, 0, 0))
    m.use_crf, m.crf_transitions = False, None
    return m
