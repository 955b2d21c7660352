"""The life cycle the five training contexts share (csrc/train_host.hip.h: TrainCtxBase, run_train_step), held to one behaviour
on each of them: profiling off and on, the totals' reset, a step the plan refuses while profiling is on, the step after it, and
a second close().  The smallest shapes the kernels take: V 6, S 5, C 4, R = R_O = 3, B 3, L 4, lengths 4 / 2 / 1."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V, S, C, R, B, L = 6, 5, 4, 3, 3, 4
LENGTHS = np.array([4, 2, 1], np.int64)
CONTEXTS = ('TrainContext', 'OnehotTrainContext', 'Fst4TrainContext', 'Ind1TrainContext', 'Decomp1TrainContext')


def _case(kind):
    """(context, weights by their C-ABI names, the batch, the gradients' names): drawn by the per-step tests' helpers"""
    from re2nn_seq_amd import _lib
    if kind == 'TrainContext':
        from test_gpu_train_max import OUT_NAMES, draw
        w, x, _, labels = draw(S, R, C, V, B, L, 'relu', 0, False, False, seed=3)
        return _lib.TrainContext(V, S, R, C, nl='relu', o_idx=1), w, (x, labels), OUT_NAMES
    if kind == 'OnehotTrainContext':
        from test_gpu_onehot_train import _random_case
        c = _random_case(V, S, C, B, L, seed=3)
        return _lib.OnehotTrainContext(V, S, C), {n: c[n] for n in ('T', 'W', 'O', 'h0', 'hT')}, (c['x'], c['labels']), ('T',)
    if kind == 'Fst4TrainContext':
        from test_gpu_fst4_train import make_case
        c = make_case(V, S, C, B, L, seed=3, lengths=LENGTHS)
        return _lib.Fst4TrainContext(V, S, C), {n: c[n] for n in ('T4', 'W4', 'h0', 'hT')}, (c['x'], c['labels']), ('T4', 'W4')
    if kind == 'Ind1TrainContext':
        from test_gpu_ind1_train import make_case
        c = make_case(V, S, C, B, L, seed=3, lengths=LENGTHS)
        return _lib.Ind1TrainContext(V, S, C), {n: c[n] for n in ('T', 'W', 'O', 'h0', 'hT')}, (c['x'], c['labels']), ('T',)
    from test_gpu_decomp1_train import ABI, NAMES, make_case
    c = make_case(V, S, R, R, C, B, L, seed=3, lengths=LENGTHS)
    return (_lib.Decomp1TrainContext(V, S, R, R, C, nl=c['nl']), {ABI[n]: c['p'][n] for n in NAMES}, (c['x'], c['labels']),
            tuple(ABI[n] for n in NAMES))


class _Stepper:
    """one context and its batch on the device; step() runs the library step on outputs pre-filled with 7.0 / 3.0 / -7"""

    def __init__(self, kind):
        dev = torch.device('cuda', 0)
        self.tc, w, (x, labels), self.grads = _case(kind)
        self.w = {n: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for n, a in w.items()}
        self.x, self.lengths, self.labels = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (x, LENGTHS, labels))

    def step(self, B=B, L=L):
        dev = self.x.device
        out = {'d' + n: torch.full_like(self.w[n], 7.0) for n in self.grads}
        out['loss'] = torch.full((1,), 3.0, device=dev)
        out['tags'] = torch.full(self.x.shape, -7, dtype=torch.int32, device=dev)
        try:
            self.tc.step({n: t.data_ptr() for n, t in self.w.items()}, self.x.data_ptr(), self.lengths.data_ptr(),
                         self.labels.data_ptr(), B, L, int(LENGTHS.sum()), {n: t.data_ptr() for n, t in out.items()})
        finally:
            torch.cuda.synchronize()
        return {n: t.cpu().numpy() for n, t in out.items()}


@pytest.mark.parametrize('kind', CONTEXTS)
def test_the_shared_life_cycle(kind):
    from re2nn_seq_amd import _lib
    st = _Stepper(kind)
    tc = st.tc
    try:
        # 1. profiling off: a step leaves nothing to report
        first = st.step()
        assert np.isfinite(first['loss']).all()
        assert tc.time() == (0.0, 0)
        # 2. profiling on: two steps, two event pairs; reading the totals resets them
        tc.set_profiling(1)
        st.step()
        st.step()
        ms, n = tc.time()
        assert n == 2 and ms > 0
        assert tc.time() == (0.0, 0)
        # 3. a step the plan refuses before any launch (B (L+1) >= 2^30, the small batch's real pointers) leaves no event pair
        with pytest.raises(_lib.FarnnError) as e:
            st.step(B=1 << 15, L=1 << 15)
        assert 'must stay below 2^30' in str(e.value)
        assert tc.time() == (0.0, 0)
        # 4. the next good step on the same context is the first one again
        again = st.step()
        assert np.array_equal(again['tags'], first['tags'])
        for name, ref in first.items():
            if kind == 'TrainContext':                      # float atomics in its kernels: the tests' rule for that step
                assert (np.abs(again[name] - ref) <= 1e-4 * (1 + np.abs(ref))).all(), name
            else:
                assert np.array_equal(again[name], ref), name
    finally:
        # 5. a second close() is harmless
        tc.close()
        tc.close()
