"""Helpers shared by the tests."""
import argparse
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
# FARNN_* switches the suite was STARTED under (scripts/gpu_r05_switches.sh runs it once per supported switch): a test's assertions
# about WHICH kernel ran hold for the default dispatch only; everything about results holds under every switch.
EXTERNAL_SWITCHES = sorted(k for k in os.environ if k.startswith('FARNN_') and k not in ('FARNN_LIB', 'FARNN_RCCL_LIB', 'FARNN_AB_CHILD') and
                           not k.startswith(('FARNN_SOAK', 'FARNN_SHAPE', 'FARNN_D1_SOAK', 'FARNN_BENCH')))
NO_SWITCH = not EXTERNAL_SWITCHES
AB_ONLY_SWITCHES = ('FARNN_CV_ONE', 'FARNN_CV_STASH', 'FARNN_NODEST')      # forms compiled into the A/B build only (csrc/build.py --probes)


def ab_build():
    """the loaded library carries the A/B-only forms (farnn_ab_build)"""
    from re2nn_seq_amd import _lib
    return _lib.ab_build()


def run_module_in_ab_build(path, extra_env=None, k=None, timeout=1500):
    """Runs a test module again in a child pytest with FARNN_LIB = the A/B build, where its A/B-only cases are not skipped.
    Returns None when there is nothing to do (already the A/B build, or it was not built)."""
    import subprocess
    import sys
    from re2nn_seq_amd import _lib
    if _lib.ab_build() or os.environ.get('FARNN_AB_CHILD') or not os.path.exists(_lib.AB_LIB_PATH):
        return None
    env = dict(os.environ, FARNN_LIB=_lib.AB_LIB_PATH, FARNN_AB_CHILD='1')
    env.update(extra_env or {})
    cmd = [sys.executable, '-m', 'pytest', path, '-q', '-x', '-m', 'gpu', '-p', 'no:cacheprovider'] + (['-k', k] if k else [])
    return subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)


def ns(**kw):
    """The fields the model classes read from the reference's `args` Namespace (main.py:14-100)."""
    d = dict(rand_constant=0.0, train_wildcard=0, train_wildcard_wildcard=0, margin=0.3,
             threshold=0.5, train_mode='sum', local_loss_func='CE1', use_priority=0,
             independent=2, update_nonlinear='none', additional_states=0, train_word_embed=0,
             use_crf=0, random=0, train_h0=0, train_hT=0, train_V_embed=0, train_c_output=1,
             farnn=0, xavier=0, bias_init=5.0, sigmoid_exponent=5, beta=1.0, train_beta=0,
             additional_nonlinear='none', random_pad_func='uniform', marryup_type='none',
             c1_kdpr=1.0, c2_kdpr=1.0, c3_pr=1.0)
    d.update(kw)
    return argparse.Namespace(**d)


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'))


def assert_scores(sc, ref, exact):
    if exact:
        assert np.array_equal(sc, ref), 'max abs diff {}'.format(np.abs(sc - ref).max())
    else:
        np.testing.assert_allclose(sc, ref, rtol=1e-4, atol=1e-4)


def in_float64(fn, params, *args, **kw):
    """`fn(params, ...)` of the oracle evaluated in float64 (fo.precision): every float array of `params` widened first."""
    from oracle import farnn_oracle as fo
    wide = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype.kind == 'f' else v) for k, v in params.items()}
    kw = {k: (v.astype(np.float64) if isinstance(v, np.ndarray) and v.dtype.kind == 'f' else v) for k, v in kw.items()}
    with fo.precision(np.float64):
        return fn(wide, *args, **kw)


def assert_float_path(got, ref32, ref64, tol=1e-4, err_msg=''):
    """ONE rule for a floating-point kernel (north_star: "within 1e-4"): within `tol` (absolute + relative) of the EXACT value
    -- the oracle evaluated in float64 -- and never farther from the float32 oracle than `tol` plus that oracle's own distance
    from the exact value at the same entry (two float32 evaluations of a sensitive recurrence scatter around the exact value;
    neither is the other's yardstick beyond its own noise).  No per-shape bars."""
    got, ref32, ref64 = np.asarray(got, np.float64), np.asarray(ref32, np.float64), np.asarray(ref64, np.float64)
    e64 = np.abs(got - ref64)
    bad = e64 > tol * (1.0 + np.abs(ref64))
    assert not bad.any(), '{} {} of {} entries beyond {} of the float64 value; worst {:.3e}'.format(
        err_msg, int(bad.sum()), bad.size, tol, float((e64 / (1.0 + np.abs(ref64))).max()))
    e32 = np.abs(got - ref32)
    bad = e32 > tol * (1.0 + np.abs(ref32)) + np.abs(ref32 - ref64)
    assert not bad.any(), '{} {} of {} entries beyond {} + the float32 oracle\'s own error; worst {:.3e}'.format(
        err_msg, int(bad.sum()), bad.size, tol, float(e32.max()))


def _grad_figures(got, ref32, ref64, tol, slices, present):
    """(figures, per-word scale or None): s = max |ref64|; 'kernel' = max |got - ref64| / s; 'oracle' = max |ref32 - ref64| / s;
    with slices, 'slice' = the worst present word's max |got - ref64| over its scale (its own max |ref64[w]|, or s where the
    word fell back), 'fallback' / 'present' = the word counts."""
    assert got.shape == ref32.shape == ref64.shape, (got.shape, ref32.shape, ref64.shape)
    s = float(np.abs(ref64).max()) if ref64.size else 0.0
    div = s if s > 0 else 1.0
    r = {'s': s, 'kernel': float(np.abs(got - ref64).max()) / div if got.size else 0.0,
         'oracle': float(np.abs(ref32 - ref64).max()) / div if got.size else 0.0}
    if slices is None:
        return r, None
    assert slices == 0, 'word slices run along axis 0'
    assert present.shape == (got.shape[0],), (present.shape, got.shape)
    g, a, b = (t.reshape(t.shape[0], -1)[present] for t in (got, ref32, ref64))
    sw = np.abs(b).max(1)
    fell = np.abs(a - b).max(1) > tol / 10 * sw
    scale = np.where(fell, s, sw)
    ratio = np.abs(g - b).max(1) / np.where(scale > 0, scale, 1.0)
    r.update(slice=float(ratio.max()) if len(ratio) else 0.0, fallback=int(fell.sum()), present=int(present.sum()))
    return r, scale


def assert_grad_path(got, ref32, ref64, tol=1e-4, slices=None, present=None, err_msg='', record=None):
    """The rule for a GRADIENT: assert_float_path's two clauses with its constant 1 replaced by the size of what is measured
    (a mean over the valid tokens leaves most gradient entries far below 1e-4, where `tol * (1 + |ref|)` accepts anything).

    Tensor clause: with s = max |ref64|, every entry within tol * s of the float64 oracle and never farther from the float32
    oracle than tol * s plus that oracle's own distance from float64 at the entry.
    Slice clause (slices = 0: axis 0 is the word id -- dVgen's rows, dT's [S, S] blocks; present = bool [V], the words that
    occur at a valid position): the same two clauses with s_w = max |ref64[w]| for every present word; a word that occurs at
    no valid position must be EXACTLY zero (the caller pre-fills the output buffer with something else).
    Conditions on the inputs, from the references alone, asserted here: the float32 oracle sits within tol / 10 * s of
    float64; a slice on which the float32 oracle alone exceeds tol / 10 * s_w is ill-conditioned (cancellation) and is judged
    at the tensor's scale, and at most 1 % of the present words may be: a case beyond that is badly drawn.
    record = (case, tensor): with TRAIN_GRAD_REPORT set, the figures are appended to that file BEFORE anything is asserted
    (profiles/train_grad_error.txt is one pytest -m gpu run into a fresh file; a record, never a source for the bar).
    Returns the figures."""
    got, ref32, ref64 = (np.asarray(a, np.float64) for a in (got, ref32, ref64))
    present = None if slices is None else np.asarray(present, bool)
    r, scale = _grad_figures(got, ref32, ref64, tol, slices, present)
    if record is not None and os.environ.get('TRAIN_GRAD_REPORT'):
        with open(os.environ['TRAIN_GRAD_REPORT'], 'a') as f:
            f.write('{:<44} {:<7} s {:.3e}  kernel {:.2e}  oracle32 {:.2e}'.format(record[0], record[1], r['s'], r['kernel'], r['oracle']))
            if slices is not None:
                f.write('  worst-slice {:.2e}  fallback {}/{}'.format(r['slice'], r['fallback'], r['present']))
            f.write('\n')
    s = r['s']
    assert np.isfinite(got).all(), '{} not finite'.format(err_msg)
    assert float(np.abs(ref32 - ref64).max()) <= tol / 10 * s, '{} badly drawn: the float32 oracle is {:.3e} of the tensor\'s scale from float64 (bar {:.1e})'.format(
        err_msg, r['oracle'], tol / 10)

    def clauses(g, a, b, scale, what):
        e64 = np.abs(g - b)
        bad = e64 > tol * scale
        assert not bad.any(), '{} {}: {} of {} entries beyond {} x scale of the float64 value; worst {:.3e} x scale'.format(
            err_msg, what, int(bad.sum()), bad.size, tol, float((e64 / np.where(scale > 0, scale, 1.0)).max()))
        e32 = np.abs(g - a)
        bad = e32 > tol * scale + np.abs(a - b)
        assert not bad.any(), '{} {}: {} of {} entries beyond {} x scale + the float32 oracle\'s own error; worst {:.3e}'.format(
            err_msg, what, int(bad.sum()), bad.size, tol, float(e32.max()))

    clauses(got, ref32, ref64, s, 'tensor')
    if slices is not None:
        assert r['fallback'] <= 0.01 * r['present'], '{} badly drawn: {} of {} present words ill-conditioned in the float32 oracle (cap 1 %)'.format(
            err_msg, r['fallback'], r['present'])
        g, a, b = (t.reshape(t.shape[0], -1) for t in (got, ref32, ref64))
        assert not ref64[~present].any() and not ref32[~present].any(), err_msg + ' the oracle has a gradient for an absent word'
        stale = g[~present] != 0
        assert not stale.any(), '{} {} entries of {} absent words are not exactly zero'.format(
            err_msg, int(stale.sum()), int(stale.any(1).sum()))
        clauses(g[present], a[present], b[present], scale[:, None], 'word slices')
    return r


def check_grad(case, tensor, got, ref32, ref64, tol=1e-4, slices=None, present=None):
    """assert_grad_path, named and recorded as (case, tensor)"""
    return assert_grad_path(got, ref32, ref64, tol, slices, present, err_msg='{} {}'.format(case, tensor), record=(case, tensor))


def present_words(x, lengths, V):
    """bool [V]: the words that occur at a valid position of the batch"""
    x, lengths = np.asarray(x), np.asarray(lengths)
    mask = np.arange(x.shape[1])[None, :] < lengths[:, None]
    p = np.zeros(V, bool)
    p[x[mask]] = True
    return p
