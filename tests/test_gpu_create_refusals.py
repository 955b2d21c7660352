"""A refused create leaves nothing behind: no handle, no device memory.  Every farnn_*_create holds the handle it builds in an
owner and its device temporaries in a scoped type (csrc/tag_host.hip.h), so each return frees both.  The returns behind a failing
HIP call cannot be provoked; the ones a caller can reach -- a refusal after the temporaries or the handle exist -- are held here."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import farnn_oracle as fo

pytestmark = pytest.mark.gpu

V, S, NC = 2000, 64, 3           # one dense T is V S S floats = 32 MB: a leak shows against the allocation granularity
ROUNDS = 20
EINVAL, ERANGE = -22, -34        # include/farnn.h


def _refused(fn_name, args, code, text):
    from re2nn_seq_amd import _lib
    lib = _lib.load()
    out = C.c_void_p(0xdead)     # the create must clear it
    rc = getattr(lib, fn_name)(*args, 0, C.byref(out))
    assert rc == code, (fn_name, rc, lib.farnn_last_error())
    assert text in lib.farnn_last_error().decode(), (fn_name, lib.farnn_last_error())
    assert not out.value, fn_name


def test_refused_creates_free_their_handle_and_temporaries():
    from re2nn_seq_amd import _lib, synth
    rng = np.random.RandomState(5)
    T, W, O, h0, hT = synth.random_ifst_tensors(V, S, NC, rng, edges_per_word=4.0)
    x, lengths = synth.random_batch(V, 4, 8, rng, min_len=1)

    def good_tags():
        h = _lib.create_onehot_ifst(T, W, O, h0, hT)
        xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(lengths).cuda()
        tags = torch.empty(x.shape, dtype=torch.int32, device='cuda')
        h.tag(xd.data_ptr(), ld.data_ptr(), x.shape[0], x.shape[1], _lib.MODE_FULL, tags.data_ptr())
        torch.cuda.synchronize()
        h.close()
        return tags.cpu().numpy().astype(np.int64)

    want = fo.decode_argmax(fo.onehot_ifst_scores(T, W, O, h0, hT, x, lengths), 0.5, 0)
    assert np.array_equal(good_tags(), want)          # (also: the library's code is on the device before memory is read)

    def base(n_cols, T_=None, W_=None, O_=None):
        return _lib.OnehotIfstDesc(V, S, n_cols, _lib.ptr(T_), _lib.ptr(W_), _lib.ptr(O_), _lib.ptr(h0), _lib.ptr(hT), None,
                                   _lib.NL['none'], _lib.SEMIRING['sum'], 0.5, 0, 0, None, 0)
    # one edge whose state index is out of range: refused after the dense T, W, O temporaries exist
    bad_state, keep1 = _lib._edge_list([0], [S + 5], [0], [-1], None)
    # one edge of weight 0.5: refused after the handle and its bitmaps exist
    half, keep2 = _lib._edge_list([0], [0], [1], [-1], np.array([0.5], np.float32))
    # 257 label columns: refused after the handle exists
    O257 = np.zeros((257, S), np.float32)
    d_edges, d_257 = base(NC), base(257, T, W, O257)
    # independent=1 over 201 states: (alpha beta^T) .* Tf[x_i] does not fit 160 KiB of LDS -- refused after the handle exists
    S1 = 201
    T1, W1, O1 = np.zeros((5, S1, S1), np.float32), np.zeros((S1, S1), np.float32), np.zeros((NC, S1, S1), np.float32)
    e1 = np.ones(S1, np.float32)
    d_ind1 = _lib.OnehotInd1Desc(5, S1, NC, _lib.ptr(T1), _lib.ptr(W1), _lib.ptr(O1), _lib.ptr(e1), _lib.ptr(e1), None,
                                 _lib.SEMIRING['sum'], 0, 0.5, 0, 0)

    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info()[0]
    for _ in range(ROUNDS):
        _refused('farnn_onehot_ifst_create_from_edges', (C.byref(d_edges), C.byref(bad_state)), EINVAL,
                 'from_edges: an edge has a word, state or label index out of range')
        _refused('farnn_onehot_ifst_create_compact', (C.byref(d_edges), C.byref(half)), EINVAL,
                 'onehot_ifst compact form: an edge is out of range or has a weight other than 1')
        _refused('farnn_onehot_ifst_create', (C.byref(d_257),), ERANGE, 'more than 256 label columns')
        _refused('farnn_onehot_ind1_create', (C.byref(d_ind1),), ERANGE, 'independent=1 scoring needs S*S*4 bytes of LDS')
    torch.cuda.synchronize()
    dropped = free_before - torch.cuda.mem_get_info()[0]
    print('device memory free before - after %d refused creates of each kind: %.1f MB' % (ROUNDS, dropped / 2.0 ** 20))
    assert dropped <= 64 * 2 ** 20                    # two creates' worth of T; twenty leaked creates are 640 MB or more

    assert np.array_equal(good_tags(), want)
    del keep1, keep2
