"""CPU checks of the device-side scorer (farnn_score_*, metrics/device.py): the counting rule's numpy
restatement against metrics.py (exact equality, the per_class key order included), the entry points in the header, the binding
and the built library, the counts struct's layout, create's refusals, and the switch in the two loops that take the scorer."""
import argparse
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('farnn_score_create', 'farnn_score_add', 'farnn_score_read', 'farnn_score_reset', 'farnn_score_destroy')

# two ids with one spelling (1 and 7), a pad label, three types; lower and upper case prefixes (metrics.py upper-cases)
I2S = {0: 'o', 1: 'B-a', 2: 'I-a', 3: 'B-b', 4: 'i-b', 5: 'B-c', 6: 'I-c', 7: 'B-a', 8: '<pad>'}
O, Ba, Ia, Bb, Ib, Bc, Ic, Ba2, PAD = range(9)


def _both(pred, gold, i2s=I2S, o_idx=0):
    from re2nn_seq_amd.metrics import device as D
    from re2nn_seq_amd.metrics.metrics import eval_seq_token, get_ner_fmeasure
    pred, gold = np.asarray(pred, np.int64), np.asarray(gold, np.int64)
    c = D.counts_from_flat(pred, gold, D.label_tables(i2s, o_idx))
    got = (D.token_level(c), D.entity_level(c, all_class=True), D.entity_level(c))
    want = (eval_seq_token(pred, gold, o_idx=o_idx), get_ner_fmeasure(gold, pred, i2s=i2s, all_class=True),
            get_ner_fmeasure(gold, pred, i2s=i2s))
    return c, got, want


def _assert_equal(got, want):
    assert got == want
    assert list(got[1][4]) == list(want[1][4])              # dict equality ignores the key order: it is part of the contract
    for g, w in zip(got[0] + got[1][:4], want[0] + want[1][:4]):
        assert type(g) is type(w), (g, w)                    # the 0 and -1 conventions are ints, as metrics.py's


CASES = {
    'two ids with one spelling': ([Ba, Ia, O, Ba2, Ia], [Ba2, Ia, O, Ba, Ia]),
    'a pad label': ([Ba, PAD, PAD, Bb], [Ba, O, PAD, Bb]),
    'I- without B-': ([O, Ia, Ia, O, Ib], [O, Ia, O, O, Ib]),
    'I- of another type': ([Ba, Ib, Ib, O], [Ba, Ia, Ib, O]),
    'adjacent B-': ([Ba, Ba, Bb, Bb, Ib], [Ba, Ba, Bb, Ba, Ia]),
    'the stream ends inside a jointly open span': ([O, Bc, Ic, Ic], [O, Bc, Ic, Ic]),
    'no pred spans': ([O, O, Ia, PAD], [Ba, Ia, O, Bb]),
    'no gold spans': ([Ba, Ia, O, Bb], [O, O, Ia, PAD]),
    'no spans at all': ([O, O], [O, PAD]),
    'a candidate dies where one span goes on': ([Ba, Ia, Ia, O], [Ba, Ia, O, O]),
    'gold-only types follow pred types in per_class': ([Bc, O, O, O, Bb], [Ba, O, Bb, O, Bc]),
}


@pytest.mark.parametrize('name', sorted(CASES))
def test_planted_cases_equal_metrics_py(name):
    pred, gold = CASES[name]
    c, got, want = _both(pred, gold)
    _assert_equal(got, want)
    if name == 'no pred spans':
        assert got[1][1:4] == (-1, 0.0, -1) and c.pred_spans == 0
    if name == 'no gold spans':
        assert got[1][1:4] == (0.0, -1, -1) and c.gold_spans == 0
    if name == 'the stream ends inside a jointly open span':
        assert c.matches == 1 and got[1][4] == {'C': [1.0, 1.0, 1.0]}
    if name == 'two ids with one spelling':
        assert c.canon_same == 5 and c.same == 3
    if name == 'gold-only types follow pred types in per_class':
        assert list(got[1][4]) == ['C', 'B', 'A']


@pytest.mark.parametrize('seed', range(6))
def test_random_streams_equal_metrics_py(seed):
    """500 streams per seed: sparse and dense B-/I- mixes, agreement between pred and gold from 30 % to 95 %."""
    rng = np.random.RandomState(seed)
    for _ in range(500):
        n = int(rng.randint(1, 60))
        w = rng.dirichlet(np.ones(9) * rng.choice([0.3, 1.0, 3.0]))
        gold = rng.choice(9, size=n, p=w)
        pred = np.where(rng.rand(n) < rng.choice([0.3, 0.7, 0.95]), gold, rng.choice(9, size=n, p=w))
        _, got, want = _both(pred, gold)
        _assert_equal(got, want)


def test_ids_outside_the_tables_count_as_kind_0_and_as_errors():
    from re2nn_seq_amd.metrics import device as D
    T = D.label_tables(I2S, 0)
    c = D.counts_from_flat([Ba, 99, Ia, -3], [Ba, Ia, Ia, O], T)
    assert c.errors == 2 and c.n == 4 and c.same == 2 and c.pred_spans == 1 and c.gold_spans == 1
    assert c.matches == 0                                     # pred's span ends at the stray id, gold's runs on


def test_a_label_map_the_host_scores_with_strings_is_not_supported():
    from re2nn_seq_amd.metrics import device as D
    assert D.DeviceScore.supported(I2S)
    assert not D.DeviceScore.supported({0: 'o', 1: 'B-'})
    assert D.label_tables({0: 'o', 1: 'B-'}, 0) is None


def test_entry_points_are_declared_bound_and_exported():
    from re2nn_seq_amd import _lib
    with open(os.path.join(ROOT, 'include', 'farnn.h')) as f:
        text = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    declared = set(re.findall(r'\b(farnn_[a-z0-9_]+)\s*\(', text))
    assert os.path.exists(_lib.LIB_PATH), 'run __graft_entry__.build() first'
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in declared, name + ' is not declared in include/farnn.h'
        assert name in _lib.SIGNATURES, name + ' is not bound in _lib.SIGNATURES'
        assert hasattr(lib, name), name + ' is not exported by the built library'


def test_the_header_says_the_adds_are_ordered_on_one_stream():
    with open(os.path.join(ROOT, 'include', 'farnn.h')) as f:
        text = ' '.join(f.read().replace(' * ', ' ').split())
    assert re.search(r'adds \(and resets\) of one handle must be ordered on ONE stream', text)


def test_ctypes_layout_of_the_counts_struct(tmp_path):
    from re2nn_seq_amd import _lib
    cname, cls = 'farnn_score_counts', _lib.ScoreCounts
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "farnn.h"', 'int main(void) {',
             '  printf("sizeof %zu\\n", sizeof({}));'.format(cname)]
    for fname, _ in cls._fields_:
        lines.append('  printf("{1} %zu\\n", offsetof({0}, {1}));'.format(cname, fname))
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(line.rsplit(' ', 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    assert int(got['sizeof']) == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[fname]) == getattr(cls, fname).offset, fname


def test_binding_constants_match_the_kernel():
    from re2nn_seq_amd import _lib
    with open(os.path.join(ROOT, 're2nn-seq_amd', 'csrc', 'farnn_score.hip')) as f:
        text = f.read()
    assert int(re.search(r'constexpr int SC_WAVES = (\d+);', text).group(1)) == _lib.SCORE_WAVES
    assert 'SC_T_FIRSTG, SC_T_ROWS' in text and _lib.SCORE_TYPE_ROWS == 5


def test_create_refuses_bad_arguments_without_a_device():
    """farnn_score_create checks its arguments before it touches a device: FARNN_EINVAL, each with a message"""
    from re2nn_seq_amd import _lib
    lib = _lib.load()
    out = ctypes.c_void_p()
    arr = lambda *v: (ctypes.c_int32 * len(v))(*v)
    kind, typ, canon = arr(0, 1, 2), arr(-1, 0, 0), arr(0, 1, 2)

    def create(k=kind, t=typ, c=canon, n=3, nt=1):
        rc = lib.farnn_score_create(ctypes.byref(out), k, t, c, n, nt, 0, 0)
        assert not out.value
        return rc, lib.farnn_last_error()
    for kw, word in ((dict(k=None), b'null'), (dict(t=None), b'null'), (dict(c=None), b'null'), (dict(n=0), b'n_labels'),
                     (dict(n=-1), b'n_labels'), (dict(nt=-1), b'n_types'), (dict(k=arr(0, 3, 2)), b'kind'),
                     (dict(k=arr(0, -1, 2)), b'kind'), (dict(t=arr(-1, 1, 0)), b'type'), (dict(t=arr(-2, 0, 0)), b'type'),
                     (dict(c=arr(0, 3, 2)), b'canon')):
        rc, msg = create(**kw)
        assert rc == -22 and word in msg, (kw, rc, msg)
    assert lib.farnn_score_create(None, kind, typ, canon, 3, 1, 0, 0) == -22
    assert lib.farnn_score_add(None, None, None, None, 1, 1, None, None) == -22
    assert lib.farnn_score_read(None, None, None) == -22 and lib.farnn_score_reset(None, None) == -22
    lib.farnn_score_destroy(None)
    if not torch.cuda.is_available():                        # good arguments get as far as the device: there is none
        rc, _ = create()
        assert rc == -19


class _Stop(Exception):
    pass


def _made(monkeypatch, module):
    made = []
    real = module.DeviceScore.supported

    class Recorder:
        supported = staticmethod(real)

        def __init__(self, i2s, o_idx, device):
            made.append((dict(i2s), o_idx, str(device)))
            raise _Stop('scorer')
    monkeypatch.setattr(module, 'DeviceScore', Recorder)
    return made


class _FakeModel:
    training = False

    def __init__(self):
        self.p = torch.zeros(3, requires_grad=True)

    def enable_training(self):
        return self

    def parameters(self):
        return iter([self.p])

    def train(self):
        raise _Stop('epoch')                                 # the loop got as far as its first epoch without a scorer

    def eval(self):
        return self

    def _dev(self):
        return torch.device('cuda', 0)

    handle = None

    def run(self, *a, **k):
        raise AssertionError('tagged before the scorer was made')

    def forward_local(self, *a, **k):
        raise _Stop('host')


@pytest.mark.parametrize('env', [None, '0', 'true', '1'])
@pytest.mark.parametrize('i2s', [I2S, {0: 'o', 1: 'B-'}], ids=['tables', 'strings'])
def test_the_epoch_loop_takes_the_scorer_only_when_asked(monkeypatch, env, i2s):
    """RE2NN_DEVICE_METRICS=1 and a label map with integer tables: train_epochs makes a DeviceScore on the model's device;
    anything else: it does not, and the host lists run as before"""
    from re2nn_seq_amd import train_onehot
    from re2nn_seq_amd.metrics import device
    monkeypatch.delenv('RE2NN_NATIVE_OPTIM', raising=False)
    if env is None:
        monkeypatch.delenv('RE2NN_DEVICE_METRICS', raising=False)
    else:
        monkeypatch.setenv('RE2NN_DEVICE_METRICS', env)
    made = _made(monkeypatch, device)
    args = argparse.Namespace(optimizer='ADAM', lr=0.25, epoch=1, bz=4, method='onehot')
    with pytest.raises(_Stop) as e:
        train_onehot.train_epochs(_FakeModel(), {}, args, {'o': 0}, i2s, None, None, {})
    if env == '1' and i2s is I2S:
        assert str(e.value) == 'scorer' and made == [(I2S, 0, 'cuda:0')]
    else:
        assert str(e.value) == 'epoch' and made == []


@pytest.mark.parametrize('env', [None, '1'])
@pytest.mark.parametrize('asked', [False, True])
@pytest.mark.parametrize('i2s', [I2S, {0: 'o', 1: 'B-'}], ids=['tables', 'strings'])
def test_the_evaluation_takes_the_scorer_only_when_its_caller_asks(monkeypatch, env, asked, i2s):
    """evaluation on the device measured slower than the pinned-buffer pipeline: the switch alone leaves
    val_onehot on the host path; device_metrics=True takes the scorer where the label map has integer tables"""
    from re2nn_seq_amd import val
    if env is None:
        monkeypatch.delenv('RE2NN_DEVICE_METRICS', raising=False)
    else:
        monkeypatch.setenv('RE2NN_DEVICE_METRICS', env)
    made = _made(monkeypatch, val)
    z = torch.zeros((1, 2), dtype=torch.int64)
    batches = [{'x': z, 's': z, 'l': torch.ones(1, dtype=torch.int64)}]
    with pytest.raises(_Stop) as e:
        val.val_onehot(batches, _FakeModel(), argparse.Namespace(bz=4), 0, i2s, device_metrics=asked)
    if asked and i2s is I2S:
        assert str(e.value) == 'scorer' and made == [(I2S, 0, 'cuda:0')]
    else:
        assert str(e.value) == 'host' and made == []


def test_the_switch_is_listed_beside_the_others():
    with open(os.path.join(ROOT, 're2nn-seq_amd', 'farnn', '_native.py')) as f:
        head = f.read().split('def opted_in')[0]
    assert re.search(r'#\s+DEVICE_METRICS\s', head)
