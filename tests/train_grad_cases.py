"""Test infrastructure: the draws and the float32 / float64 references of the gradient-scale tests, shared by
tests/test_train_grad_faults.py (CPU: the references alone must satisfy assert_grad_path's conditions on its inputs) and
tests/test_gpu_train_grad_scale.py (the HIP steps on the same draws).

A case is a dict: step ('sum' | 'max' | 'onehot'), the step's inputs, and V.  refs(case) gives the two oracle evaluations
as (loss, {library output name without the 'd': gradient}) -- Vgen, S1, S2, W, C, h0, hT, the gates, trans; T for the
onehot step.  WORD_SLICED names the gradients indexed by word id along axis 0.

Planted word counts: the onehot dT kernel works on runs of 32 positions of one word, its counting sort on chunks of 256 flat
positions b L + i, the max step's word-gradient kernel on 64 chunks of the distinct words; COUNTS are the occurrence
counts on both sides of those boundaries."""
import numpy as np
import torch

import decomp_max_train_ref as dmr
import onehot_train_ref as otr
from test_gpu_train_envelope import GATES, GRADS, sum_case, sum_oracle
from test_gpu_train_max import MIN_GAP, draw as max_draw
from util import present_words

WORD_SLICED = ('Vgen', 'T')
COUNTS = (1, 31, 32, 33, 63, 64, 65, 257)
PROD = dict(V=11000, S=104, R=250, B=256, L=64)      # the production shape of the decomposed tagger
# the max step at the production vocabulary and rank: a batch of B x L tokens has B L 2 S maxima that must each clear the
# restatement's MIN_GAP, which bounds the batch and not V: 32 x 16 has a gapped draw, 32 x 24 and beyond have none in 60 seeds
PROD_MAX = dict(V=11000, S=104, R=250, B=32, L=16)


# ---- batches -----------------------------------------------------------------------------------------------------------
def planted_batch(V, seed, B=32, L=40):
    """x, lengths, info: words 0 .. 7 occur at exactly COUNTS valid positions (and word 2 also behind sequence ends, which
    must not count); word 8 only at the last valid position of the last non-empty sequence; word 9 only behind sequence
    ends; an empty sequence in the middle and two at the end; both sides of flat position 256 valid."""
    rng = np.random.RandomState(seed)
    assert V >= 40
    lengths = rng.randint(L // 2, L + 1, size=B).astype(np.int64)
    lengths[0] = L
    lengths[3] = 0
    lengths[B - 2:] = 0
    lengths[256 // L] = L                                    # flat positions 255 and 256 are valid
    mask = np.arange(L)[None, :] < lengths[:, None]
    n = int(mask.sum())
    toks = np.concatenate([np.full(c, w, np.int64) for w, c in enumerate(COUNTS)])
    assert n > len(toks) + 1
    fill = rng.randint(10, V, size=n - 1 - len(toks)).astype(np.int64)
    body = rng.permutation(np.concatenate([toks, fill]))
    x = np.full((B, L), 9, np.int64)                         # word 9 everywhere behind the ends ...
    x[~mask & (rng.rand(B, L) < 0.3)] = 2                    # ... and word 2 at some of them
    x[mask] = np.concatenate([body, [8]])                    # row-major: the last valid position of the last non-empty row
    last_row = int(np.nonzero(lengths)[0][-1])
    info = dict(counts={w: c for w, c in enumerate(COUNTS)}, last_word=8, last_pos=(last_row, int(lengths[last_row]) - 1),
                absent_word=9)
    return x, lengths, info


def assert_planted(x, lengths, info):
    """the properties planted_batch promises, counted from the batch itself"""
    B, L = x.shape
    mask = np.arange(L)[None, :] < lengths[:, None]
    cnt = np.bincount(x[mask], minlength=10)
    for w, c in info['counts'].items():
        assert cnt[w] == c, (w, cnt[w], c)
    b, i = info['last_pos']
    assert cnt[info['last_word']] == 1 and x[b, i] == info['last_word']
    assert not lengths[b + 1:].any() and i == lengths[b] - 1 and b < B - 1
    assert cnt[info['absent_word']] == 0 and (x[~mask] == info['absent_word']).any()
    assert (x[~mask] == 2).any()                              # a counted word also sits behind an end
    flat = mask.reshape(-1)
    assert any(flat[m - 1] and flat[m] for m in range(256, B * L, 256))
    assert (lengths == 0).sum() >= 3 and lengths.max() == L


def distinct_words_batch(V, n_words, seed, L=12):
    """a batch in which exactly n_words distinct words occur at valid positions (each at least once)"""
    rng = np.random.RandomState(seed)
    B = max(2, (2 * n_words + L - 1) // L + 2)
    lengths = rng.randint(L // 2, L + 1, size=B).astype(np.int64)
    lengths[0] = L
    lengths[1] = 0
    mask = np.arange(L)[None, :] < lengths[:, None]
    n = int(mask.sum())
    assert n >= n_words and V > n_words
    words = rng.permutation(V - 1)[:n_words]
    body = np.concatenate([words, words[rng.randint(0, n_words, size=n - n_words)]])
    x = np.full((B, L), V - 1, np.int64)
    x[mask] = rng.permutation(body)
    assert len(np.unique(x[mask])) == n_words
    return x, lengths


def zipf_batch(V, B, L, seed):
    from re2nn_seq_amd import synth
    return synth.random_batch(V, B, L, np.random.RandomState(seed))


# ---- cases -------------------------------------------------------------------------------------------------------------
def sum_step_case(S, R, K, V, B, L, farnn, crf, nl, seed, batch=None):
    """the envelope module's draw (test_gpu_train_envelope.sum_case), optionally on another batch"""
    p, x, lengths, labels = sum_case(S, R, K, V, B, L, farnn, crf, seed)
    if batch is not None:
        x, lengths = batch
        assert x.shape == (B, L)
    return dict(step='sum', p=p, x=x, lengths=lengths, labels=labels, nl=nl, farnn=farnn, crf=crf, sig_k=3.0, V=V)


def max_step_case(S, R, K, V, B, L, nl, farnn, crf, seed0, batch=None, tries=40):
    """test_gpu_train_max's draw, optionally on another batch (a function of the seed): the first seed whose float64
    restatement has no maximum decided by less than MIN_GAP.  The float64 reference comes with the case."""
    for seed in range(seed0, seed0 + tries):
        w, x, lengths, labels = max_draw(S, R, K, V, B, L, nl, farnn, crf, False, seed=seed)
        if batch is not None:
            x, lengths = batch(seed)
            assert x.shape == (B, L)
        try:
            r64 = dmr.step_on_table(w, torch.from_numpy(x), torch.from_numpy(lengths), labels, nl=nl, farnn=farnn,
                                    dtype=torch.float64, min_gap=MIN_GAP)
        except dmr.GapError:
            continue
        return dict(step='max', w=w, x=x, lengths=lengths, labels=labels, nl=nl, farnn=farnn, crf=crf, V=V, seed=seed,
                    ref64=(r64[0], r64[1]))
    raise AssertionError('no draw without a near tie in {} seeds from {}'.format(tries, seed0))


def onehot_sparse_case(V, S, C, B, L, seed, nl='none', batch=None):
    """test_gpu_onehot_train._random_case: a 0/1 automaton"""
    from test_gpu_onehot_train import _random_case
    c = _random_case(V, S, C, B, L, seed)
    if batch is not None:
        c['x'], c['lengths'] = batch
        c['labels'] = np.random.RandomState(seed + 1).randint(0, C, size=c['x'].shape).astype(np.int64)
    return dict(step='onehot', c=c, nl=nl, V=V)


def onehot_dense_case(V, S, C, B, L, seed, nl, batch=None):
    """T and W small positive floats, every row of T[w] + W summing below 1 (contractive), one label per state, dense
    positive h0 / hT: every lane of the chain and dT kernels carries a non-zero."""
    rng = np.random.RandomState(seed)
    T = (rng.rand(V, S, S) * (0.7 / S)).astype(np.float32)
    W = (rng.rand(S, S) * (0.7 / S)).astype(np.float32)
    assert float((T + W).sum(2).max()) < 1.0
    O = np.zeros((C, S), np.float32)
    O[rng.randint(0, C, size=S), np.arange(S)] = 1.0
    h0 = (0.2 + 0.8 * rng.rand(S)).astype(np.float32)
    hT = (0.2 + 0.8 * rng.rand(S)).astype(np.float32)
    x, lengths = batch if batch is not None else zipf_batch(V, B, L, seed + 1)
    labels = rng.randint(0, C, size=x.shape).astype(np.int64)
    return dict(step='onehot', nl=nl, V=V, c=dict(T=T, W=W, O=O, h0=h0, hT=hT, P=None, x=x, lengths=lengths, labels=labels))


def batch_of(case):
    c = case['c'] if case['step'] == 'onehot' else case
    return c['x'], c['lengths']


def present_of(case):
    x, lengths = batch_of(case)
    return present_words(x, lengths, case['V'])


def with_batch(case, x=None, lengths=None, order=None):
    """the case on other lengths, or with its batch rows in another order"""
    case = dict(case)
    inner = dict(case['c']) if case['step'] == 'onehot' else case
    if lengths is not None:
        inner['lengths'] = np.asarray(lengths, np.int64)
    if order is not None:
        for k in ('x', 'lengths', 'labels'):
            inner[k] = np.ascontiguousarray(inner[k][order])
    if case['step'] == 'onehot':
        case['c'] = inner
    case.pop('ref64', None)
    return case


# ---- references --------------------------------------------------------------------------------------------------------
def reference(case, dtype):
    """(loss, {name: gradient as float64 numpy in the library's layout}) of one oracle evaluation in `dtype`"""
    if case['step'] == 'sum':
        loss, g, _ = sum_oracle(case['p'], case['x'], case['lengths'], case['labels'], case['nl'], case['farnn'],
                                case['sig_k'], dtype)
        names = GRADS + tuple((n, n) for n in GATES[:3 * case['farnn']]) + ((('trans', 'crf.transitions'),) if case['crf'] else ())
        return float(loss), {n: g[key].numpy().reshape(case['p'][key].shape).astype(np.float64) for n, key in names}
    if case['step'] == 'max':
        if dtype == torch.float64 and 'ref64' in case:
            loss, g = case['ref64']
        else:
            loss, g, _ = dmr.step_on_table(case['w'], torch.from_numpy(case['x']), torch.from_numpy(case['lengths']),
                                           case['labels'], nl=case['nl'], farnn=case['farnn'], dtype=dtype)
        return float(loss), {n: np.asarray(v, np.float64) for n, v in g.items()}
    loss, g, _ = otr.step(dtype=dtype, nl=case['nl'], **case['c'])
    return float(loss), {'T': np.asarray(g, np.float64)}


def dense_share(case, ref64):
    """the share of non-zero entries in the float64 dT blocks of the present words"""
    return float((ref64[1]['T'][present_of(case)] != 0).mean())


def refs(case):
    return reference(case, torch.float32), reference(case, torch.float64)


def check_all(name, got, ref32, ref64, present, check):
    """`check` (util.check_grad or util.assert_grad_path with a leading case name) on every gradient of the step"""
    out = {}
    for n in ref64[1]:
        sl = n in WORD_SLICED
        out[n] = check(name, 'd' + n, np.asarray(got[n]).reshape(ref64[1][n].shape), ref32[1][n], ref64[1][n],
                       slices=0 if sl else None, present=present if sl else None)
    return out


# ---- the cases the GPU module runs: id -> builder -------------------------------------------------------------------------
def _prod_sum(farnn, crf, seed):
    d = PROD
    return lambda: sum_step_case(d['S'], d['R'], 75 if crf else 73, d['V'], d['B'], d['L'], farnn, crf, 'tanh', seed=seed,
                                 batch=zipf_batch(d['V'], d['B'], d['L'], seed + 100))


def _prod_max():
    d = PROD_MAX
    return max_step_case(d['S'], d['R'], 75, d['V'], d['B'], d['L'], 'tanh', 2, True, seed0=400,
                         batch=lambda seed: zipf_batch(d['V'], d['B'], d['L'], seed))


def _planted(step):
    def build():
        if step == 'sum':
            x, lengths, info = planted_batch(300, 5)
            c = sum_step_case(40, 24, 12, 300, x.shape[0], x.shape[1], 1, False, 'tanh', seed=6, batch=(x, lengths))
        elif step == 'max':
            holder = {}

            def batch(seed):
                holder['b'] = planted_batch(300, seed)
                return holder['b'][:2]
            c = max_step_case(24, 20, 9, 300, 32, 40, 'tanh', 0, False, seed0=700, batch=batch, tries=200)
            info = holder['b'][2]
        else:
            x, lengths, info = planted_batch(300, 7)
            c = onehot_dense_case(300, 40, 12, x.shape[0], x.shape[1], 8, 'tanh', batch=(x, lengths))
        c['info'] = info
        return c
    return build


def _distinct(n_words):
    return lambda: max_step_case(20, 70, 6, 200, max(2, (2 * n_words + 11) // 12 + 2), 12, 'tanh', 1, False, seed0=900 + n_words,
                                 batch=lambda seed: distinct_words_batch(200, n_words, seed), tries=200)


def _dense(S, nl):
    return lambda: onehot_dense_case(300, S, 20, 24, 20, S + (nl == 'tanh'), nl)


GPU_CASES = {'prod-sum-farnn0-ce1': _prod_sum(0, False, 31), 'prod-sum-farnn2-crf': _prod_sum(2, True, 51), 'prod-max-farnn2-crf': _prod_max,
             'planted-sum': _planted('sum'), 'planted-max': _planted('max'), 'planted-onehot': _planted('onehot')}
GPU_CASES.update({'max-{}-words'.format(n): _distinct(n) for n in (63, 64, 65, 129)})
GPU_CASES.update({'dense-onehot-S{}-{}'.format(S, nl): _dense(S, nl) for S in (32, 72, 96, 128) for nl in ('none', 'tanh')})
