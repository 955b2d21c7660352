"""CPU checks of the library's optimizer step (farnn_optim_*): the entry points in the header, the
binding and the built library, the descriptor's layout, the restatement (tests/native_optim_ref.py) against torch's own
optimizers, and what must happen before any device work."""
import argparse
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import native_optim_ref as nor
from util import assert_float_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('farnn_optim_create', 'farnn_optim_step', 'farnn_optim_set_lr', 'farnn_optim_steps', 'farnn_optim_set_steps',
                'farnn_optim_destroy')


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


def test_the_header_says_the_step_is_not_to_be_captured():
    with open(os.path.join(ROOT, 'include', 'farnn.h')) as f:
        text = ' '.join(f.read().split())
    assert re.search(r'farnn_optim_step must NOT be captured into a HIP graph', text)


def test_ctypes_layout_of_the_optimizer_descriptor(tmp_path):
    from re2nn_seq_amd import _lib
    pairs = {'farnn_optim_desc': _lib.OptimDesc}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "farnn.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        lines.append('  printf("%s sizeof %zu\\n", "{0}", sizeof({0}));'.format(cname))
        for fname, _ in cls._fields_:
            lines.append('  printf("%s.%s %zu\\n", "{0}", "{1}", offsetof({0}, {1}));'.format(cname, fname))
    lines += ['  printf("kinds %d %d\\n", FARNN_OPTIM_SGD, FARNN_OPTIM_ADAM);', '  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert out[-1] == 'kinds {} {}'.format(_lib.OPTIM_SGD, _lib.OPTIM_ADAM)
    got = dict(line.rsplit(' ', 1) for line in out[:-1])
    for cname, cls in pairs.items():
        assert int(got[cname + ' sizeof']) == ctypes.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got['{}.{}'.format(cname, fname)]) == getattr(cls, fname).offset, (cname, fname)


def test_binding_constants_match_the_kernel_header():
    from re2nn_seq_amd import _lib
    with open(os.path.join(ROOT, 're2nn-seq_amd', 'csrc', 'optim.hip.h')) as f:
        text = f.read()
    assert int(re.search(r'constexpr int OPT_CHUNK = (\d+);', text).group(1)) == _lib.OPTIM_CHUNK
    assert int(re.search(r'constexpr int OPT_MAX_TENSORS = (\d+);', text).group(1)) == _lib.OPTIM_MAX_TENSORS


SHAPES = [(1,), (3,), (7, 5), (2, 3, 4), (129,)]


def _draw(seed, steps=3):
    rng = np.random.RandomState(seed)
    params = [rng.randn(*s).astype(np.float32) for s in SHAPES]
    grads = [[(rng.randn(*s) * 10.0 ** rng.randint(-3, 2)).astype(np.float32) for s in SHAPES] for _ in range(steps)]
    return params, grads


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_restatement_agrees_with_torch_on_the_cpu(kind):
    """three steps; in the second one tensor has no gradient (torch skips it and does not advance its step)"""
    params, grads = _draw(5)
    grads[1][2] = None
    tp = [torch.from_numpy(p.copy()).requires_grad_(True) for p in params]
    if kind == 'adam':
        opt = torch.optim.Adam(tp, lr=0.05, weight_decay=0)
        r32, r64 = nor.AdamRef(params, lr=0.05, dtype=np.float32), nor.AdamRef(params, lr=0.05, dtype=np.float64)
    else:
        opt = torch.optim.SGD(tp, lr=0.05, weight_decay=0)
        r32, r64 = nor.SgdRef(params, lr=0.05, dtype=np.float32), nor.SgdRef(params, lr=0.05, dtype=np.float64)
    for gs in grads:
        for p, g in zip(tp, gs):
            p.grad = None if g is None else torch.from_numpy(g.copy())
        opt.step()
        r32.step(gs)
        r64.step(gs)
    for i, p in enumerate(tp):
        assert r32.p[i].dtype == np.float32 and r64.p[i].dtype == np.float64
        assert_float_path(p.detach().numpy(), r32.p[i], r64.p[i], err_msg='{} tensor {}'.format(kind, i))
        if kind == 'adam':
            st = opt.state[p]
            assert int(st['step']) == r64.t[i] == (2 if i == 2 else 3)
            assert_float_path(st['exp_avg'].numpy(), r32.m[i], r64.m[i], err_msg='exp_avg {}'.format(i))
            assert_float_path(st['exp_avg_sq'].numpy(), r32.v[i], r64.v[i], err_msg='exp_avg_sq {}'.format(i))


def _no_library(monkeypatch):
    """from here on any use of the HIP library fails the test"""
    from re2nn_seq_amd import _lib

    def boom(*a, **k):
        raise AssertionError('device work before the refusal')
    monkeypatch.setattr(_lib, 'load', boom)
    monkeypatch.setattr(_lib, 'Optim', boom)


@pytest.mark.parametrize('name', ['Adam', 'SGD'])
def test_cpu_parameters_are_refused_before_any_device_work(monkeypatch, name):
    from re2nn_seq_amd import _lib
    from re2nn_seq_amd.farnn import optim
    _no_library(monkeypatch)
    p = torch.zeros(5, requires_grad=True)
    with pytest.raises(_lib.FarnnError, match='no CPU fallback'):
        getattr(optim, name)([p], lr=0.05)


def test_weight_decay_is_refused():
    from re2nn_seq_amd.farnn import optim
    with pytest.raises(ValueError, match='weight_decay'):
        optim.Adam([torch.zeros(5, requires_grad=True)], lr=0.05, weight_decay=0.1)


def test_create_refuses_bad_arguments_without_a_device():
    """farnn_optim_create checks its arguments before it touches a device: FARNN_EINVAL for a numel of 0, for an unknown
    kind and for no tensors, each with a message"""
    from re2nn_seq_amd import _lib
    lib = _lib.load()
    out = ctypes.c_void_p()
    one = (ctypes.c_int64 * 2)(5, 0)
    good = _lib.OptimDesc(_lib.OPTIM_ADAM, 0.05, 0.9, 0.999, 1e-8)
    assert lib.farnn_optim_create(ctypes.byref(good), one, 2, 0, ctypes.byref(out)) == -22 and not out.value
    assert b'numel' in lib.farnn_last_error()
    assert lib.farnn_optim_create(ctypes.byref(_lib.OptimDesc(7, 0.05, 0.9, 0.999, 1e-8)), one, 1, 0, ctypes.byref(out)) == -22
    assert b'kind' in lib.farnn_last_error() and not out.value
    assert lib.farnn_optim_create(ctypes.byref(good), one, 0, 0, ctypes.byref(out)) == -22
    assert lib.farnn_optim_create(ctypes.byref(_lib.OptimDesc(_lib.OPTIM_ADAM, 0.05, 1.0, 0.999, 1e-8)), one, 1, 0,
                                  ctypes.byref(out)) == -22


class _Stop(Exception):
    pass


class _FakeModel:
    def __init__(self):
        self.p = torch.zeros(3, requires_grad=True)

    def enable_training(self):
        return self

    def parameters(self):
        return iter([self.p])


@pytest.mark.parametrize('name', ['ADAM', 'SGD'])
@pytest.mark.parametrize('env', [None, '0', '1'])
def test_the_epoch_loop_takes_the_library_optimizer_only_when_asked(monkeypatch, env, name):
    """RE2NN_NATIVE_OPTIM unset (or not 1): train_epochs constructs torch.optim.Adam / SGD as before; = 1: farnn.optim's"""
    from re2nn_seq_amd import train_onehot
    from re2nn_seq_amd.farnn import optim
    _no_library(monkeypatch)
    if env is None:
        monkeypatch.delenv('RE2NN_NATIVE_OPTIM', raising=False)
    else:
        monkeypatch.setenv('RE2NN_NATIVE_OPTIM', env)
    made = []

    def recorder(which):
        def make(params, lr, weight_decay):
            made.append((which, lr, weight_decay, len(list(params))))
            raise _Stop()
        return make
    for mod, tag in ((torch.optim, 'torch'), (optim, 'native')):
        monkeypatch.setattr(mod, 'Adam', recorder(tag + '.ADAM'))
        monkeypatch.setattr(mod, 'SGD', recorder(tag + '.SGD'))
    args = argparse.Namespace(optimizer=name, lr=0.25, epoch=1, bz=4)
    with pytest.raises(_Stop):
        train_onehot.train_epochs(_FakeModel(), {}, args, {}, {}, None, None, {})
    assert made == [(('native.' if env == '1' else 'torch.') + name, 0.25, 0, 1)]
