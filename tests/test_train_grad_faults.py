"""The gradient rule (tests/util.py:assert_grad_path) tested on the CPU, from the oracles alone.

For one small case per training step a catalogue of WRONG gradients is built from the float32 reference and the rule must
reject every one of them; it must accept the float32 reference itself and the same reference evaluated with the batch rows
in another order (another summation order of the same arithmetic).  The faults that rescale or drop a contribution are
also put to the older rule (assert_float_path, 1e-4 (1 + |ref|)); how many of them it lets through is printed (run with
-s) and recorded in DESIGN.md section 7.

The second half holds every draw of tests/test_gpu_train_grad_scale.py to the rule's conditions on its inputs (the float32
oracle within tol / 10 of float64 at each tensor's scale, at most 1 % of the present words ill-conditioned), so that a
badly drawn case is found here and not on a GPU."""
import numpy as np
import pytest
import torch

import train_grad_cases as tg
from util import assert_float_path, assert_grad_path


def _sum_small():
    return tg.sum_step_case(24, 16, 9, 40, 6, 10, 2, True, 'tanh', seed=3)          # farnn 2 + CRF


def _sum_k256():
    S, R, K, V, B, L, farnn, crf, nl = 256, 64, 256, 50, 6, 12, 0, False, 'tanh'      # the envelope module's K256, as drawn there
    return tg.sum_step_case(S, R, K, V, B, L, farnn, crf, nl, seed=S + 3 * R + K + farnn)


def _max_small():
    return tg.max_step_case(23, 30, 9, 50, 6, 9, 'tanh', 2, False, seed0=60)


def _onehot_small():
    return tg.onehot_sparse_case(300, 40, 20, 9, 15, seed=13, nl='tanh')


CASES = {'sum-farnn2-crf': _sum_small, 'sum-K256': _sum_k256, 'max': _max_small, 'onehot': _onehot_small}
_cache = {}


def _case(name):
    if name not in _cache:
        c = CASES[name]()
        _cache[name] = (c,) + tg.refs(c)
    return _cache[name]


def _is_mean(case):
    """CE1 is a mean over the valid tokens; the CRF loss is a sum over the sequences (no token count in it)"""
    return not case.get('crf', False)


def _judge(case, got, ref32, ref64):
    tg.check_all('', got, ref32, ref64, tg.present_of(case),
                 lambda c, n, g, a, b, **kw: assert_grad_path(g, a, b, err_msg=n, **kw))


def _rejected(case, got, ref32, ref64):
    try:
        _judge(case, got, ref32, ref64)
    except AssertionError:
        return True
    return False


def _old_rule_accepts(got, ref32, ref64):
    try:
        for n in ref64[1]:
            assert_float_path(np.asarray(got[n]).reshape(ref64[1][n].shape), ref32[1][n], ref64[1][n], err_msg=n)
    except AssertionError:
        return False
    return True


def _victim(case):
    """a sequence of more than one token that is neither the first nor the longest"""
    _, lengths = tg.batch_of(case)
    cand = [b for b in range(1, len(lengths)) if lengths[b] > 1]
    return cand[len(cand) // 2]


def _scaled(g, f):
    return {n: v * f for n, v in g.items()}


def _faults(name):
    """(label, wrong gradients, also put to the old rule) built from float32 evaluations only"""
    case, ref32, _ = _case(name)
    g = ref32[1]
    x, lengths = tg.batch_of(case)
    valid = int(lengths.sum())
    out = []
    for n in g:                                                                           # 1
        out.append(('d{} x 0.99'.format(n), dict(g, **{n: g[n] * 0.99}), True))
        out.append(('d{} x 0.9'.format(n), dict(g, **{n: g[n] * 0.9}), True))
    b = _victim(case)
    less = lengths.copy()
    less[b] = 0                                                                           # 2
    f = (valid - int(lengths[b])) / valid if _is_mean(case) else 1.0
    out.append(('sequence {} left out'.format(b), _scaled(tg.reference(tg.with_batch(case, lengths=less), torch.float32)[1], f), True))
    less = lengths.copy()
    less[b] -= 1                                                                          # 3
    f = (valid - 1) / valid if _is_mean(case) else 1.0
    out.append(('last token of sequence {} left out'.format(b), _scaled(tg.reference(tg.with_batch(case, lengths=less), torch.float32)[1], f), True))
    word = [n for n in g if n in tg.WORD_SLICED][0]                                       # 4
    present = tg.present_of(case)
    mask = np.arange(x.shape[1])[None, :] < lengths[:, None]
    cnt = np.bincount(x[mask], minlength=case['V']).astype(float)
    cnt[~present | (np.abs(g[word]).reshape(case['V'], -1).max(1) == 0)] = np.inf          # a word whose slice is not zero anyway
    rare = int(cnt.argmin())
    z = g[word].copy()
    z[rare] = 0.0
    out.append(('d{}[rarest word {}] zeroed'.format(word, rare), dict(g, **{word: z}), False))
    absent = int(np.nonzero(~present)[0][0])
    z = g[word].copy()
    z[absent] = 1e-6
    out.append(('d{}[absent word {}] stale'.format(word, absent), dict(g, **{word: z}), False))
    for n in ('W', 'trans'):                                                              # 5
        if n in g:
            out.append(('d{} transposed'.format(n), dict(g, **{n: g[n].T.copy()}), False))
    if 'T' in g:
        out.append(('dT blocks transposed', dict(g, T=g['T'].transpose(0, 2, 1).copy()), False))
    if _is_mean(case):                                                                    # 6
        out.append(('mean over B L', _scaled(g, valid / float(x.size)), True))
    if 'bs2' in g:                                                                        # 7
        out.append(('dbs1 <-> dbs2', dict(g, bs1=g['bs2'], bs2=g['bs1']), False))
        out.append(('dWss1 <-> dWss2', dict(g, Wss1=g['Wss2'], Wss2=g['Wss1']), False))
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_the_float32_reference_is_accepted_in_either_row_order(name):
    case, ref32, ref64 = _case(name)
    _judge(case, ref32[1], ref32, ref64)
    x, _ = tg.batch_of(case)
    order = np.random.RandomState(1).permutation(x.shape[0])
    assert not np.array_equal(order, np.arange(x.shape[0]))
    _judge(case, tg.reference(tg.with_batch(case, order=order), torch.float32)[1], ref32, ref64)


@pytest.mark.parametrize('name', list(CASES))
def test_every_planted_fault_is_rejected(name):
    case, ref32, ref64 = _case(name)
    faults = _faults(name)
    labels = ' | '.join(f[0] for f in faults)
    for kind in ('x 0.99', 'left out', 'last token', 'rarest', 'stale') + (('mean over',) if _is_mean(case) else ()) + \
            (('<->', 'dtrans transposed') if name == 'sum-farnn2-crf' else ()) + (('dT blocks',) if name == 'onehot' else ('dW transposed',)):
        assert kind in labels, (kind, labels)
    missed = [label for label, got, _ in faults if not _rejected(case, got, ref32, ref64)]
    assert not missed, 'the gradient rule accepts: {}'.format(missed)
    old = [label for label, got, both in faults if both and _old_rule_accepts(got, ref32, ref64)]
    print('\n{}: the gradient rule rejects all {} faults; assert_float_path accepts {} of the {} put to it: {}'.format(
        name, len(faults), len(old), sum(1 for f in faults if f[2]), old))


def test_the_old_rule_accepts_a_scaled_tensor_and_a_missing_sequence_at_K256():
    """what the envelope's K256 case could not see before: dVgen or dhT scaled by 0.9, and the full-length sequence (12 of the
    34 valid tokens) missing from every gradient"""
    case, ref32, ref64 = _case('sum-K256')
    old = [label for label, got, both in _faults('sum-K256') if both and _old_rule_accepts(got, ref32, ref64)]
    assert 'dVgen x 0.9' in old and 'dhT x 0.9' in old, old
    _, lengths = tg.batch_of(case)
    valid = int(lengths.sum())
    assert lengths[0] == 12 and valid == 34
    less = lengths.copy()
    less[0] = 0
    got = _scaled(tg.reference(tg.with_batch(case, lengths=less), torch.float32)[1], (valid - 12) / valid)
    assert _old_rule_accepts(got, ref32, ref64)
    assert _rejected(case, got, ref32, ref64)
    for n in ref64[1]:                                        # and the gradient rule sees it in every tensor on its own
        with pytest.raises(AssertionError):
            assert_grad_path(got[n], ref32[1][n], ref64[1][n])


@pytest.mark.parametrize('name', list(tg.GPU_CASES))
def test_gpu_draws_meet_the_conditions_on_the_references(name):
    """assert_grad_path's conditions on its inputs hold for the draw (it asserts them), and so does what the GPU test asserts
    about the batch before it calls the library"""
    case = tg.GPU_CASES[name]()
    ref32, ref64 = tg.refs(case)
    _judge(case, ref32[1], ref32, ref64)
    x, lengths = tg.batch_of(case)
    if 'info' in case:
        tg.assert_planted(x, lengths, case['info'])
    if name.startswith('dense'):
        assert tg.dense_share(case, ref64) > 0.5
