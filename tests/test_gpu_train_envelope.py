"""The three HIP training steps at every kernel form and size limit their C-ABI accepts, against high-precision references.

The host code (csrc/farnn_train.hip, with the shared pieces of csrc/train_host.hip.h) picks a template instantiation per step from S, R, K, L, B and the device's CU count.
Each case below is shaped to reach one form, named in its comment:
  decomposed sum step  train_forward_kernel / train_backward_kernel <LDSW, GATED, S slots, R slots, NSEQ> (weights in LDS
                       when vec + mat <= 160 KiB, else through L2 with nss of the S x S matrices in LDS; four sequences per
                       workgroup on the L2 path when 4 max(S, R) <= 1024 and B >= 2 n_cu; two S slots when NSEQ S > 512, two
                       R slots when NSEQ S or NSEQ R > 512) and train_loss_kernel<CLDS, PH> (C in LDS when
                       8 (SPd0 + 2K) 4 + K (S+1) 4 <= 150 KiB), CRF from K = 4 to K = 190 at L = 8;
  max-semiring step    tmax_* at S = 192 (the limit) and at rank 512;
  onehot step          onehot_train_chain_kernel<8 | 18 | 24 | 32>, onehot_dT_kernel<2 | 4 | 6 | 8> on both sides of each
                       boundary, train_loss_kernel<false, 0> and the score-column limit.
Every loss and gradient is held to tests/util.py:assert_float_path (1e-4) against the oracle evaluated in float64 and in
float32; the refusals return their FarnnError code and leave a live context usable."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import farnn_train_oracle as to  # noqa: E402
from test_gpu_onehot_train import _check_against_restatement, _random_case, _run_step, run_step_c_abi  # noqa: E402
import onehot_train_ref as otr  # noqa: E402
from test_gpu_train_max import check_against, gapped_case, run_library  # noqa: E402
from util import assert_float_path, check_grad, present_words  # noqa: E402

pytestmark = pytest.mark.gpu

ERANGE = -34
GATES = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')
# library output name -> the oracle's parameter name
GRADS = (('Vgen', 'V_embed'), ('S1', 'S1'), ('S2', 'S2'), ('W', 'wildcard_mat'), ('C', 'C_output_mat'), ('h0', 'h0'),
         ('hT', 'hT'))
FULL = -1          # B = 2 n_cu: the batch at which the through-L2 kernels take four sequences per workgroup


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- decomposed sum step ---------------------------------------------------------------------------------------------
def sum_case(S, R, K, V, B, L, farnn, crf, seed):
    """float32 weights named like the oracle's parameters, with the word table passed in directly (V_embed = Vgen,
    beta = 1, so the generated part is multiplied by an exact 0); contractive draws; an empty and a full-length sequence."""
    rng = np.random.RandomState(seed)
    f = lambda *shape, sc=0.3: torch.from_numpy((rng.randn(*shape) * sc).astype(np.float32))   # noqa: E731
    fs = 0.7 / np.sqrt(max(S, R))
    Cm = np.zeros((K, S), np.float32)
    Cm[rng.randint(0, K - (2 if crf else 0), size=S), np.arange(S)] = (rng.rand(S) < 0.8)
    p = {'S1': f(S, R, sc=fs), 'S2': f(S, R, sc=fs), 'V_embed': f(V, R, sc=0.8),
         'embed_r_generalized': torch.zeros(4, R), 'embedding.weight': torch.zeros(V, 4), 'beta_vec': torch.ones(R),
         'C_output_mat': torch.from_numpy(Cm + (rng.rand(K, S) * 0.2 / K).astype(np.float32)),   # C.sum(0) stays near 1
         'wildcard_mat': torch.from_numpy(((rng.rand(S, S) < 1.0 / S) * 0.5).astype(np.float32)),
         'h0': f(S, sc=0.5), 'hT': f(S, sc=0.5), 'priority_mat': torch.eye(K)}
    for n in GATES[:3 * farnn]:
        p[n] = f(1, S, sc=0.5) if n.startswith('bs') else (f(S, S, sc=0.5 / np.sqrt(S)) if n.startswith('Wss') else f(R, S, sc=0.5 / np.sqrt(R)))
    if crf:
        tr = (rng.randn(K, K) * 0.3).astype(np.float32)
        tr[:, K - 2] = -10000.0
        tr[K - 1, :] = -10000.0
        p['crf.transitions'] = torch.from_numpy(tr)
    lengths = rng.randint(1, L + 1, size=B).astype(np.int64)
    lengths[0] = L
    if B > 1:
        lengths[1] = 0
    x = rng.randint(0, V, size=(B, L)).astype(np.int64)
    labels = rng.randint(0, K - (2 if crf else 0), size=(B, L)).astype(np.int64)
    return p, x, lengths, labels


def sum_oracle(p, x, lengths, labels, nl, farnn, sig_k, dtype):
    q = {k: v.to(dtype) for k, v in p.items()}
    return to.train_step_batched(q, torch.from_numpy(x), torch.from_numpy(lengths), torch.from_numpy(labels), nl=nl,
                                 farnn=farnn, sig_k=sig_k)


class SumRun:
    """The library's inputs and outputs for one case, on the device (kept alive: the step takes raw pointers)."""

    def __init__(self, p, x, lengths, labels, farnn, crf):
        dev = torch.device('cuda')
        self.B, self.L = x.shape
        self.valid = int(lengths.sum())
        self.w = {n: p[k].to(dev).contiguous() for n, k in GRADS}
        self.w.update({n: p[n].to(dev).contiguous() for n in GATES[:3 * farnn]})
        self.trans = p['crf.transitions'].to(dev) if crf else None
        self.out = {'d' + n: torch.full_like(t, 7.0) for n, t in self.w.items()}      # the library must zero them itself
        self.dtrans = torch.full_like(self.trans, 7.0) if crf else None
        self.loss = torch.full((1,), 3.0, device=dev)
        self.tags = torch.empty((self.B, self.L), dtype=torch.int32, device=dev)
        self.x, self.lengths, self.labels = (torch.from_numpy(a).to(dev) for a in (x, lengths, labels))

    def step(self, tc):
        tc.step(dict({n: t.data_ptr() for n, t in self.w.items()}, P=None,
                     crf_trans=None if self.trans is None else self.trans.data_ptr()),
                self.x.data_ptr(), self.lengths.data_ptr(), self.labels.data_ptr(), self.B, self.L, self.valid,
                dict({n: t.data_ptr() for n, t in self.out.items()}, loss=self.loss.data_ptr(), tags=self.tags.data_ptr(),
                     dtrans=None if self.dtrans is None else self.dtrans.data_ptr()))
        torch.cuda.synchronize()
        res = {n: t.cpu().numpy() for n, t in self.out.items()}
        if self.dtrans is not None:
            res['dtrans'] = self.dtrans.cpu().numpy()
        res['loss'] = float(self.loss)
        res['tags'] = self.tags.cpu().numpy()
        return res


def viterbi_tags_and_margin(sc, lengths, trans):
    """Per position: the tag of the best path through it (max-product forward + backward in float64) and the gap to the
    best path through another tag there (a Viterbi tag is decided by more than float noise where that gap is wide)."""
    B, L, K = sc.shape
    START, STOP = K - 2, K - 1
    tags = np.full((B, L), -1, np.int64)
    gap = np.zeros((B, L))
    for b in range(B):
        n = int(lengths[b])
        if n == 0:
            continue
        e = sc[b, :n]
        al = np.empty((n, K))
        be = np.empty((n, K))
        al[0] = e[0] + trans[START]
        for t in range(1, n):
            al[t] = (al[t - 1][:, None] + trans).max(0) + e[t]
        be[n - 1] = trans[:, STOP]
        for t in range(n - 2, -1, -1):
            be[t] = (trans + (e[t + 1] + be[t + 1])[None, :]).max(1)
        through = al + be
        top2 = np.sort(through, 1)[:, -2:]
        tags[b, :n] = through.argmax(1)
        gap[b, :n] = (top2[:, 1] - top2[:, 0]) / (1.0 + np.abs(top2[:, 1]))
    return tags, gap


def check_sum_step(res, ref32, ref64, lengths, farnn, trans=None, o_idx=1, threshold=0.5, x=None, case='sum'):
    """loss and every gradient against the float64 and float32 oracle, by the ONE rule and by the gradient rule (each tensor
    at its own scale; with the batch `x`, dVgen also row by row at each present word's scale and exactly zero at the absent
    ones); tags against the float64 decode"""
    (l32, g32, _), (l64, g64, sc64) = ref32, ref64
    crf = trans is not None
    assert_float_path([res['loss']], [float(l32)], [float(l64)], err_msg='loss')
    names = GRADS + tuple((n, n) for n in GATES[:3 * farnn])
    for n, key in names:
        got = res['d' + n]
        assert_float_path(got, g32[key].numpy().reshape(got.shape), g64[key].numpy().reshape(got.shape), err_msg='d' + n)
        sliced = n == 'Vgen' and x is not None
        check_grad(case, 'd' + n, got, g32[key].numpy().reshape(got.shape), g64[key].numpy().reshape(got.shape),
                   slices=0 if sliced else None, present=present_words(x, lengths, got.shape[0]) if sliced else None)
    if crf:
        assert_float_path(res['dtrans'], g32['crf.transitions'].numpy(), g64['crf.transitions'].numpy(), err_msg='dtrans')
        check_grad(case, 'dtrans', res['dtrans'], g32['crf.transitions'].numpy(), g64['crf.transitions'].numpy())
    # tags where the decision is wider than float noise
    sc = sc64.numpy()
    B, L, K = sc.shape
    mask = np.arange(L)[None, :] < lengths[:, None]
    t = res['tags']
    assert (t[~mask] == -1).all()
    c = sc.copy()
    if crf:         # the Viterbi runs on the emissions with the O column (K-3) clamped (oracle/farnn_oracle.py:decode_crf)
        c[..., K - 3] = np.minimum(c[..., K - 3], threshold)
        want, gap = viterbi_tags_and_margin(c, lengths, np.asarray(trans, np.float64))
    else:
        c[..., K - 1] = np.minimum(c[..., K - 1], threshold)
        top2 = np.sort(c, -1)[..., -2:]
        gap = (top2[..., 1] - top2[..., 0]) / (1.0 + np.abs(top2[..., 1]))
        want = c.argmax(-1)
    want = np.where(want == (K - 3 if crf else K - 1), o_idx, want)
    safe = mask & (gap > 1e-4)
    assert safe.sum() >= 0.5 * mask.sum(), 'too few positions decided by more than float noise'
    bad = np.argwhere(safe & (t != want))
    assert not len(bad), '{} of {} decided tags differ; (b, i, len, got, want, gap): {}'.format(
        len(bad), int(safe.sum()), [(int(b), int(i), int(lengths[b]), int(t[b, i]), int(want[b, i]), float(gap[b, i]))
                                    for b, i in bad[:8]])


SUM_CASES = [   # S, R, K, V, B, L, farnn, crf, nl
    pytest.param(257, 40, 12, 50, 5, 10, 0, False, 'tanh', id='S257'),            # L2, 2 seq, 2 S-slots + 2 R-slots
    pytest.param(300, 40, 9, 50, 5, 10, 1, True, 'none', id='S300-g1-crf'),       # L2 gated, 2 seq, (2, 2)
    pytest.param(512, 512, 20, 40, 4, 8, 0, False, 'tanh', id='S512R512'),        # the ABI's 512 / 512 limit: L2, 2 seq, (2, 2)
    pytest.param(512, 512, 75, 40, 3, 8, 2, True, 'tanh', id='S512R512-g2-crf'),  # L2 gated, 2 seq, (2, 2); loss CLDS=false
    pytest.param(40, 257, 12, 50, 5, 10, 0, True, 'none', id='R257'),             # forward LDS (1, 2); backward L2 (1, 2), nss 1
    pytest.param(64, 400, 12, 50, 5, 10, 2, False, 'tanh', id='R400-g2'),         # L2 gated, 2 seq, (1, 2), nss 3
    pytest.param(64, 200, 12, 50, 5, 10, 1, True, 'tanh', id='R200-g1-crf'),      # forward LDS gated (1, 1); backward L2, nss 2
    pytest.param(104, 250, 75, 120, FULL, 16, 2, True, 'tanh', id='R250-g2-crf-full'),   # L2 gated, 4 seq, (1, 2)
    pytest.param(129, 100, 12, 100, FULL, 10, 0, False, 'none', id='S129-full'),  # L2, 4 seq, (2, 2)
    pytest.param(200, 60, 30, 100, FULL, 12, 1, False, 'tanh', id='S200-g1-full'),       # L2 gated, 4 seq, (2, 2)
    pytest.param(256, 256, 12, 100, FULL, 10, 0, True, 'tanh', id='S256R256-crf-full'),  # L2, 4 seq at 4 max(S, R) = 1024
    pytest.param(256, 256, 12, 100, FULL, 10, 2, False, 'tanh', id='S256R256-g2-full'),  # L2 gated, 4 seq at 4 max(S, R) = 1024
    pytest.param(256, 64, 256, 50, 6, 12, 0, False, 'tanh', id='K256'),           # train_loss_kernel<false, 0>
    pytest.param(190, 30, 190, 50, 3, 8, 0, True, 'tanh', id='K190-crf'),         # largest CRF (K = 190 at L = 8): crf<true>, loss<false, 1|2>
    pytest.param(300, 40, 300, 50, 4, 6, 1, False, 'tanh', id='K300-g1'),         # train_loss_kernel<false, 0>, gated (2, 2)
    pytest.param(12, 8, 4, 30, 5, 10, 0, True, 'none', id='K4-crf'),              # smallest CRF (K = 4); all LDS (1, 1)
]


@pytest.mark.parametrize('S,R,K,V,B,L,farnn,crf,nl', SUM_CASES)
def test_sum_step_forms_vs_float64_oracle(S, R, K, V, B, L, farnn, crf, nl):
    from re2nn_seq_amd import _lib
    if B == FULL:
        B = 2 * n_cu()
    p, x, lengths, labels = sum_case(S, R, K, V, B, L, farnn, crf, seed=S + 3 * R + K + farnn)
    ref64 = sum_oracle(p, x, lengths, labels, nl, farnn, 3.0, torch.float64)
    ref32 = sum_oracle(p, x, lengths, labels, nl, farnn, 3.0, torch.float32)
    tc = _lib.TrainContext(V, S, R, K, nl=nl, threshold=0.5, o_idx=1, use_crf=crf, farnn=farnn, sigmoid_exponent=3.0)
    res = SumRun(p, x, lengths, labels, farnn, crf).step(tc)
    check_sum_step(res, ref32, ref64, lengths, farnn, p['crf.transitions'] if crf else None, x=x,
                   case='envelope-sum S{} R{} K{} farnn{} crf{}'.format(S, R, K, farnn, int(crf)))
    tc.close()


def _expect_erange(call, match):
    from re2nn_seq_amd import _lib
    with pytest.raises(_lib.FarnnError, match=match) as e:
        call()
    assert 'code {}'.format(ERANGE) in str(e.value), str(e.value)


def test_sum_step_refusals_leave_the_context_usable():
    """On one live context (S = R = 512, farnn 2): a batch with B (L+1) max(S, R) >= 2^30 is refused before anything is
    enqueued; so is a sequence length whose forward chain kernel needs more than 160 KiB of LDS (the step's plan refuses
    it).  Both leave the pre-filled output buffers as they were.  A valid step on the same context then matches the oracle."""
    from re2nn_seq_amd import _lib
    S = R = 512
    K, V, farnn, nl = 12, 40, 2, 'tanh'
    p, x, lengths, labels = sum_case(S, R, K, V, 3, 8, farnn, False, seed=91)
    run = SumRun(p, x, lengths, labels, farnn, False)
    tc = _lib.TrainContext(V, S, R, K, nl=nl, threshold=0.5, o_idx=1, farnn=farnn, sigmoid_exponent=3.0)
    dev = torch.device('cuda')

    def refused_step(B, L):
        # inputs of the full size, so that nothing could be read past an end even if the refusal were missing
        big = SumRun(p, np.zeros((B, L), np.int64), np.full(B, L, np.int64), np.zeros((B, L), np.int64), farnn, False)

        def call():
            try:
                big.step(tc)
            finally:        # a refused step has enqueued nothing: the outputs still hold what SumRun filled them with
                torch.cuda.synchronize(dev)
                assert float(big.loss) == 3.0
                for n, t in big.out.items():
                    assert bool((t == 7.0).all()), n
        return call

    B, L = 2048, 1024
    assert B * (L + 1) * max(S, R) >= 1 << 30
    _expect_erange(refused_step(B, L), 'below 2\\^30')
    _expect_erange(refused_step(1, 2600), 'more than 160 KiB of LDS')
    torch.cuda.synchronize(dev)
    res = run.step(tc)
    check_sum_step(res, sum_oracle(p, x, lengths, labels, nl, farnn, 3.0, torch.float32),
                   sum_oracle(p, x, lengths, labels, nl, farnn, 3.0, torch.float64), lengths, farnn, x=x, case='envelope-sum after refusals')
    tc.close()


@pytest.mark.parametrize('S,R', [(513, 8), (8, 513)])
def test_sum_step_refuses_more_than_512_states_or_rank(S, R):
    """accepted at create (the max semiring and the tagging path have their own limits), refused at the step"""
    from re2nn_seq_amd import _lib
    K, V = 5, 10
    p, x, lengths, labels = sum_case(S, R, K, V, 2, 3, 0, False, seed=4)
    tc = _lib.TrainContext(V, S, R, K, nl='tanh')
    run = SumRun(p, x, lengths, labels, 0, False)
    _expect_erange(lambda: run.step(tc), 'more than 512 states or rank above 512')
    tc.close()


# ---- max-semiring step -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,R,K,V,B,L,nl,farnn,crf,prio', [
    (192, 300, 40, 60, 4, 6, 'tanh', 2, True, False),      # TM_MAX_S = 192: dM_w [S][S] is 144 KiB of LDS; gates + CRF
    (160, 512, 20, 60, 4, 6, 'tanh', 0, False, False),     # rank 512: tmax_wgrad_kernel's grid of ceil(R / 64) = 8
])
def test_max_step_at_its_limits_vs_float64_restatement(S, R, K, V, B, L, nl, farnn, crf, prio):
    w, x, lengths, labels, ref32, ref64 = gapped_case(S, R, K, V, B, L, nl, farnn, crf, prio, seed0=S + R)
    res, _ = run_library(w, x, lengths, labels, nl, farnn, crf)
    check_against(res, ref32, ref64, farnn, crf, x=x, lengths=lengths, case='envelope-max S{} R{}'.format(S, R))
    mask = np.arange(L)[None, :] < lengths[:, None]
    assert (res['tags'][~mask] == -1).all()


# ---- onehot step -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [
    32,    # chain <8>, dT <2> (its last S)
    33,    # chain <8>, dT <4>
    64,    # chain <8> (its last S), dT <4>
    65,    # chain <18>, dT <6>
    72,    # chain <18> (its last S), dT <6>
    73,    # chain <24>, dT <6>
    80,    # chain <24>, dT <6>
    96,    # chain <24> (its last S), dT <6>
    97,    # chain <32>, dT <8>
    128,   # chain <32> at OT_MAX_S, dT <8>
])
def test_onehot_step_each_chain_and_dT_form(S):
    _check_against_restatement(_random_case(300, S, 20, 9, 15, seed=S), nl='tanh', case='envelope-onehot S{}'.format(S))


@pytest.mark.parametrize('S,C,B,L', [
    (128, 300, 6, 12),     # train_loss_kernel<false, 0>: output_mat read through L2
    (80, 20, 1, 1),        # one sequence of one token
    (97, 20, 40, 256),     # a long ragged batch
])
def test_onehot_step_loss_forms_and_geometries(S, C, B, L):
    c = _random_case(300, S, C, B, L, seed=S + C + B)
    if B > 1:
        assert c['lengths'].max() == L and c['lengths'].min() < L
    _check_against_restatement(c, nl='none', case='envelope-onehot S{} C{} B{} L{}'.format(S, C, B, L))


def test_onehot_create_refusals_and_the_score_column_limit():
    """S = 129 and more score columns than the loss kernel's per-wavefront vectors can hold in LDS are refused at create;
    the largest accepted count (8 (SPd0 + 2C) 4 bytes = 150 KiB at S = 128: C = 2332) trains and matches the references."""
    from re2nn_seq_amd import _lib
    _expect_erange(lambda: _lib.OnehotTrainContext(30, 129, 20), 'more than 128 states')
    _expect_erange(lambda: _lib.OnehotTrainContext(30, 128, 2333), 'too many score columns')
    c = _random_case(40, 128, 2332, 3, 5, seed=2332)
    loss, dT, tags, tc = _run_step(**c)
    l32, g32, _ = otr.step(dtype=torch.float32, **c)
    l64, g64, _ = otr.step(dtype=torch.float64, **c)
    assert_float_path(loss, l32, l64, err_msg='loss')
    assert_float_path(dT, g32, g64, err_msg='dT')
    check_grad('envelope-onehot C2332', 'dT', run_step_c_abi(c)[1], g32, g64, slices=0, present=present_words(c['x'], c['lengths'], 40))
    mask = np.arange(c['x'].shape[1])[None, :] < c['lengths'][:, None]
    assert (tags[~mask] == -1).all()
    tc.close()
