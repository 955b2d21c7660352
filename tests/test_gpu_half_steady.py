"""The steady-state step of the 16-bit recurrence (csrc/chain_dest.hip.h, H16: `chain_regs_kernel<f16 blocks>`).

The step loop of the f16 form has two bodies: an UNCHECKED one for every group of D steps with t0 + 2 D <= nsteps (no end-of-sequence
test, an unconditional issue of step t + D, a plain counted wait) and the CHECKED one for the rest of the sequence.  What can go
wrong is at the seams: the hand-over between the bodies, the drain of the last D - 1 steps, the reload of the 64-step address
window ((t + 1 + D) & 63 == 0 and t + 1 + D < nsteps: with D dividing 64 that is always a step of the UNCHECKED body, followed by
unchecked or by checked steps depending on the length).  So:

  * lengths 0, 1, D-1, D, D+1, 2D-1, 2D, 2D+1, 3D, 63, 64, 65, 127, 128, 129 in ONE batch (L = 129; D is read from
    csrc/chain_regs_params.hip.h, the constant the build uses), and a batch of one full-length sequence;
  * S = 1, 2, 71, 72, C = 5; 0/1 automata, and one with dyadic non-integer weights; nl = none, relu (the branch-free kernel) and
    tanh (the NLX one);
  * MODE_LOCAL and MODE_FULL, tags with and without the flat output; scores under FARNN_NOFUSE=1.
Tags and scores are BIT-IDENTICAL to the same library on the f32 blocks (FARNN_NOHALF=1: one child process that runs this file as a
script), tags equal the oracle's wherever the oracle is exact (float32 and float64 evaluations agree) and by the 2e-4 margin rule
elsewhere (tanh, dyadic weights).  The default dispatch stays the two launches by name.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from oracle import farnn_oracle as fo                    # noqa: E402
from util import NO_SWITCH, in_float64                   # noqa: E402

pytestmark = pytest.mark.gpu


def ring_depth():
    """RD_D of csrc/chain_regs_params.hip.h: the ring depth the library is built with"""
    with open(os.path.join(ROOT, 're2nn-seq_amd', 'csrc', 'chain_regs_params.hip.h')) as f:
        m = re.search(r'constexpr\s+int\s+RD_D\s*=\s*(\d+)\s*;', f.read())
    assert m, 'RD_D not found in chain_regs_params.hip.h'
    return int(m.group(1))


D = ring_depth()
V, C, L = 12, 5, 129
LENGTHS = [0, 1, D - 1, D, D + 1, 2 * D - 1, 2 * D, 2 * D + 1, 3 * D, 63, 64, 65, 127, 128, 129]
STATES = [1, 2, 71, 72]
NLS = ['none', 'relu', 'tanh']
CASES = [(S, '01', nl) for S in STATES for nl in NLS] + [(71, 'dyadic', nl) for nl in NLS]
HALF_NAME, F32_NAME, SCORE_NAME = 'chain_regs_kernel<f16 blocks>', 'chain_regs_kernel', 'label_map_score_kernel'
ORACLE_NL = {'none': fo.NL_NONE, 'relu': fo.NL_RELU, 'tanh': fo.NL_TANH}


def _model(S, kind):
    from re2nn_seq_amd import synth
    rng = np.random.RandomState(77 * S + 5)
    T, W, O, h0, hT = synth.random_ifst_tensors(V, S, C, rng, edges_per_word=max(1.0, 0.5 * S), n_final=min(2, S))
    if S <= 2:
        # (T + W stays 0 / 1 and upper triangular: no doubling loop -- 129 steps of one overflow f32)
        W = np.diag(np.diag(W)).astype(np.float32)
        T = np.triu(T * (W == 0.0)[None]).astype(np.float32)
    if kind == 'dyadic':
        # multiples of 1/8 below 1 in magnitude, most of them non-integers: every entry an f16 exactly, the sums soon are not
        kT = rng.randint(1, 8, size=T.shape) * rng.choice([-1, 1], size=T.shape)
        kW = rng.randint(1, 8, size=W.shape) * rng.choice([-1, 1], size=W.shape)
        T = (T * kT / 8.0).astype(np.float32)
        W = (W * kW / 8.0).astype(np.float32)
    return T, W, O, h0, hT


def _batches():
    rng = np.random.RandomState(4321)
    lengths = np.asarray(LENGTHS, np.int64)
    x = np.full((len(lengths), L), V - 1, dtype=np.int64)
    for b, n in enumerate(lengths):
        x[b, :n] = rng.randint(0, V - 1, size=int(n))
    return [(x, lengths), (x[-1:].copy(), np.asarray([L], np.int64))]


def _tag(h, x, lengths, mode, want_flat, want_scores):
    """one farnn_tag call on handle h: (tags, flat or None, scores or None, chain kernel, score kernel)"""
    import torch
    from re2nn_seq_amd import _lib
    B, Lx = x.shape
    K = h.num_columns()
    xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(lengths).cuda()
    tags = torch.full((B, Lx), -7, dtype=torch.int32, device='cuda')
    nflat = B * Lx if mode == _lib.MODE_FULL else int(lengths.sum())
    flat = torch.full((max(nflat, 1),), -7, dtype=torch.int64, device='cuda') if want_flat else None
    scores = torch.full((B, Lx, K), -7.0, dtype=torch.float32, device='cuda') if want_scores else None
    h.tag(xd.data_ptr(), ld.data_ptr(), B, Lx, mode, tags.data_ptr(), flat.data_ptr() if want_flat else None,
          scores.data_ptr() if want_scores else None)
    torch.cuda.synchronize()
    return (tags.cpu().numpy(), flat.cpu().numpy()[:int(lengths.sum())] if want_flat else None,
            scores.cpu().numpy() if want_scores else None, h.kernel_name(_lib.KERN_CHAIN), h.kernel_name(_lib.KERN_SCORE))


def _create(model, nl, nofuse):
    from re2nn_seq_amd import _lib
    if nofuse:
        os.environ['FARNN_NOFUSE'] = '1'                  # (read at create) recurrence-only launch, the score tiles read the stash
    try:
        return _lib.create_onehot_ifst(*model, nl=nl)
    finally:
        if nofuse:
            del os.environ['FARNN_NOFUSE']


def _results():
    """every case under the switches of THIS process: {key: array}"""
    from re2nn_seq_amd import _lib
    out = {}
    for S, kind, nl in CASES:
        model = _model(S, kind)
        for bi, (x, lengths) in enumerate(_batches()):
            for mname, mode in (('local', _lib.MODE_LOCAL), ('full', _lib.MODE_FULL)):
                key = 'S{}_{}_{}_b{}_{}'.format(S, kind, nl, bi, mname)
                h = _create(model, nl, False)
                tags, _, _, kc, ks = _tag(h, x, lengths, mode, False, False)
                h.close()
                h = _create(model, nl, False)
                tagsf, flat, _, kc2, ks2 = _tag(h, x, lengths, mode, True, False)
                h.close()
                h = _create(model, nl, True)
                tags2, _, scores, kc3, _ = _tag(h, x, lengths, mode, False, True)
                h.close()
                out[key + '_tags'], out[key + '_tagsf'], out[key + '_flat'] = tags, tagsf, flat
                out[key + '_tags2'], out[key + '_scores'] = tags2, scores
                out[key + '_names'] = np.asarray([kc, ks, kc2, ks2, kc3])
    return out


@pytest.fixture(scope='module')
def both(tmp_path_factory):
    """(this process's results, the FARNN_NOHALF=1 child's): each computed once"""
    mine = _results()
    path = str(tmp_path_factory.mktemp('steady') / 'nohalf.npz')
    env = dict(os.environ, FARNN_NOHALF='1')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return mine, dict(np.load(path))


_REFS = {}


def _oracle(S, kind, nl, bi):
    """(float32 oracle scores, float64 ones) of a case: computed once"""
    key = (S, kind, nl, bi)
    if key not in _REFS:
        model = _model(S, kind)
        x, lengths = _batches()[bi]
        with np.errstate(all='ignore'):
            ref = fo.onehot_ifst_scores(*model, x, lengths, nl=ORACLE_NL[nl])
            ref64 = in_float64(lambda p, *a: fo.onehot_ifst_scores(p['T'], p['W'], p['O'], p['h0'], p['hT'], *a, nl=ORACLE_NL[nl]),
                               dict(zip(('T', 'W', 'O', 'h0', 'hT'), model)), x, lengths)
        _REFS[key] = (ref, ref64)
    return _REFS[key]


@pytest.mark.parametrize('S,kind,nl', CASES, ids=['S{}-{}-{}'.format(*c) for c in CASES])
def test_every_seam_of_the_two_step_bodies(S, kind, nl, both):
    mine, child = both
    for bi, (x, lengths) in enumerate(_batches()):
        ref, ref64 = _oracle(S, kind, nl, bi)
        for mname in ('local', 'full'):
            key = 'S{}_{}_{}_b{}_{}'.format(S, kind, nl, bi, mname)
            what = '{} B={}'.format(key, x.shape[0])
            if NO_SWITCH:
                assert list(mine[key + '_names']) == [HALF_NAME, SCORE_NAME, HALF_NAME, SCORE_NAME, HALF_NAME], what
                assert list(child[key + '_names']) == [F32_NAME, SCORE_NAME, F32_NAME, SCORE_NAME, F32_NAME], what
            # the same library on the f32 blocks: every bit
            for part in ('_tags', '_tagsf', '_flat', '_tags2'):
                assert np.array_equal(mine[key + part], child[key + part]), what + part
            assert np.array_equal(mine[key + '_scores'].view(np.uint32), child[key + '_scores'].view(np.uint32)), what
            # the oracle: exact where its float32 and float64 evaluations agree; else the project's margin rule for the tags
            valid = np.arange(L)[None, :] < lengths[:, None]
            mask = np.ones_like(valid) if mname == 'full' else valid
            fin = np.isfinite(ref64).all(-1) & np.isfinite(ref).all(-1)
            exact = bool(fin.all()) and np.array_equal(ref.astype(np.float64), ref64)
            want = fo.decode_argmax(ref, 0.5, 0)
            got = mine[key + '_scores']
            print('{}: oracle exact {}, finite {}/{}, max |got - ref32| {:.3e}'.format(
                what, exact, int(fin.sum()), fin.size, float(np.abs(got[mask & fin] - ref[mask & fin]).max()) if (mask & fin).any() else 0.0))
            assert exact or nl == 'tanh' or kind != '01', what      # (the 0/1 automata with an exact nl stay inside fp32's exact range)
            if exact:
                assert np.array_equal(got[mask], ref[mask]), what
                safe = mask
            else:
                refc = np.where(np.isfinite(ref64), ref64, 0.0); refc[..., -1] = np.minimum(refc[..., -1], 0.5)
                top2 = np.sort(refc, axis=-1)[..., -2:]
                with np.errstate(all='ignore'):
                    margin = 2e-4 * (1.0 + np.abs(refc).max(-1)) + 2 * np.abs(np.where(fin[..., None], ref - ref64, 0.0)).max(-1)
                safe = mask & fin & ((top2[..., 1] - top2[..., 0]) > margin)
            for t in (mine[key + '_tags'], mine[key + '_tagsf'], mine[key + '_tags2']):
                assert np.array_equal(t[safe], want[safe]), what
                assert (t[~mask] == -1).all(), what
            if mname == 'local' and exact:
                assert np.array_equal(mine[key + '_flat'], fo.forward_local_tags(ref, lengths, 0.5, 0)), what


def test_one_handle_twice_with_different_shapes():
    """nothing of a call survives into the next: (B, L) = (15, 129), then (3, 2 D + 1), then the first again"""
    from re2nn_seq_amd import _lib
    model = _model(71, '01')
    x, lengths = _batches()[0]
    L2 = 2 * D + 1
    x2, lengths2 = x[[5, 7, 1], :L2].copy(), np.asarray([2 * D - 1, L2, 1], np.int64)
    h = _create(model, 'none', False)
    a, _, _, name, sname = _tag(h, x, lengths, _lib.MODE_LOCAL, False, False)
    b, _, _, _, _ = _tag(h, x2, lengths2, _lib.MODE_LOCAL, False, False)
    c, _, _, _, _ = _tag(h, x, lengths, _lib.MODE_LOCAL, False, False)
    h.close()
    if NO_SWITCH:
        assert (name, sname) == (HALF_NAME, SCORE_NAME)
    ref = fo.onehot_ifst_scores(*model, x, lengths)
    ref2 = fo.onehot_ifst_scores(*model, x2, lengths2)
    m1, m2 = np.arange(L)[None, :] < lengths[:, None], np.arange(L2)[None, :] < lengths2[:, None]
    assert np.array_equal(a[m1], fo.decode_argmax(ref, 0.5, 0)[m1]) and (a[~m1] == -1).all()
    assert np.array_equal(b[m2], fo.decode_argmax(ref2, 0.5, 0)[m2]) and (b[~m2] == -1).all()
    assert np.array_equal(a, c)


def test_one_ineligible_entry_keeps_the_f32_kernel():
    from re2nn_seq_amd import _lib
    T, W, O, h0, hT = _model(71, '01')
    T[3, 0, 8] = 1.0 / 3.0
    x, lengths = _batches()[0]
    h = _create((T, W, O, h0, hT), 'none', False)
    tags, _, _, name, sname = _tag(h, x, lengths, _lib.MODE_LOCAL, False, False)
    h.close()
    if NO_SWITCH:
        assert (name, sname) == (F32_NAME, SCORE_NAME)
    assert 'f16' not in name
    with np.errstate(all='ignore'):
        ref = fo.onehot_ifst_scores(T, W, O, h0, hT, x, lengths)
        ref64 = in_float64(lambda p, *a: fo.onehot_ifst_scores(p['T'], p['W'], p['O'], p['h0'], p['hT'], *a),
                           dict(T=T, W=W, O=O, h0=h0, hT=hT), x, lengths)
    mask = np.arange(L)[None, :] < lengths[:, None]
    refc = ref64.copy(); refc[..., -1] = np.minimum(refc[..., -1], 0.5)
    top2 = np.sort(refc, axis=-1)[..., -2:]
    safe = mask & ((top2[..., 1] - top2[..., 0]) > 2e-4 * (1.0 + np.abs(ref64).max(-1)) + 2 * np.abs(ref - ref64).max(-1))
    assert np.array_equal(tags[safe], fo.decode_argmax(ref, 0.5, 0)[safe])
    assert (tags[~mask] == -1).all()


if __name__ == '__main__':                                # the child: the same cases under the parent's environment + FARNN_NOHALF=1
    np.savez(sys.argv[1], **_results())
