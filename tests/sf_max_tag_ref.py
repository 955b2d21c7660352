"""The vector-input tagger in the max semiring (FARNN_S_SF, train_mode='max'; reference model_decompose_single.py:435-442)
restated through the existing oracle: sf_tag_ref.restate with 'semiring': fo.SEMIRING_MAX -- the oracle's decomp_ifst_scores
has the max branch (Tr = S1 diag(v) S2^T + W, h' = max_j hbar[j] Tr[j, s]).  The decided-position rule, TOL and UNDECIDED_CAP are
sf_tag_ref's."""
import json
import os

import numpy as np

from oracle import farnn_oracle as fo
from util import GOLDEN
import sf_tag_ref as sr

TOL = sr.TOL
UNDECIDED_CAP = sr.UNDECIDED_CAP


def fixture():
    """(meta of decomp_small.json, meta of sf_max_small.json, decomp_small.npz, sf_max_small.npz)"""
    with open(os.path.join(GOLDEN, 'decomp_small.json')) as f:
        dmeta = json.load(f)
    with open(os.path.join(GOLDEN, 'sf_max_small.json')) as f:
        smeta = json.load(f)
    return dmeta, smeta, np.load(os.path.join(GOLDEN, 'decomp_small.npz')), np.load(os.path.join(GOLDEN, 'sf_max_small.npz'))


def configs():
    with open(os.path.join(GOLDEN, 'sf_max_small.json')) as f:
        return json.load(f)['configs']


def config_of(dmeta, k):
    """config k of decomp_small, run in the max semiring"""
    return dict(dmeta['configs'][k], train_mode='max')


def params_from_fixture(g, k, cfg):
    return dict(sr.params_from_fixture(g, k, cfg), semiring=fo.SEMIRING_MAX)


def as_max(p):
    """an oracle parameter dict, in the max semiring"""
    return dict(p, semiring=fo.SEMIRING_MAX)


def restate(p, v, lengths, P=None, wide=False):
    return sr.restate(as_max(p), v, lengths, P, wide=wide)


def decided_positions(g, k, cfg, meta, v, lengths):
    pre = 'c{}.'.format(k)
    P = g[pre + 'priority_mat'] if cfg.get('use_priority', 0) else None
    s64 = restate(params_from_fixture(g, k, cfg), v, lengths, P, wide=True)
    tr = g[pre + 'crf_transitions'] if cfg.get('use_crf', 0) else None
    return sr.decided(s64, lengths, meta['threshold'], tr)
