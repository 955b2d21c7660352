"""The training step of the vector-input tagger (FARNN_S_SF) restated through the existing training oracle,
for the CPU and GPU tests of farnn_decomp_sf_train_step.

FARNN_S_SF.forward(train=True) is FARNN_S_D_W_I_S.forward_local(train=True) with the looked-up row Vgen[x[b, t]] replaced by the
given vector v[b, t]: oracle/farnn_train_oracle.train_step, called with the leaf V_embed := v.reshape(B L, R), beta_vec = 1 (so
that Vgen IS that leaf) and the ids x = arange(B L).reshape(B, L), is that model, and the gradient of the leaf is d loss / d v.
Nothing under oracle/ is edited.

The cases are drawn here, once, for both test files: the shapes are the smallest at which the new kernels can go wrong (S and R
no multiple of 4 / 16 / 64, on both sides of one wavefront's 64 columns and of one 16-wide MFMA tile; an odd batch against two
and four sequences per workgroup; lengths 0, 1 and L in one batch; a batch without any pad row).  Magnitudes are automaton-like
(every state feeds one label, about one wildcard edge per state) so that check_grad's own conditions on the references hold:
tests/test_sf_train_cpu.py asserts that for every case, from the references alone.
"""
import functools

import numpy as np
import torch

import sf_tag_ref
from oracle import farnn_train_oracle as to

TOL = 1e-4
SHAPES = ((9, 7), (40, 33), (70, 70), (33, 130))                 # (S, R)
BATCHES = ((1, 1, (1,)), (3, 2, (0, 1, 2)), (5, 9, (0, 1, 9, 4, 9)), (3, 9, (9, 9, 9)), (5, 2, (2, 0, 1, 2, 1)), (1, 9, (9,)))
# (farnn, update_nonlinear, CRF, priority layer): every farnn x loss pair twice, every nonlinearity with and without P
VARIANTS = ((0, 'none', False, False), (1, 'tanh', False, True), (2, 'relutanh', False, False),
            (0, 'tanh', True, True), (1, 'relutanh', True, False), (2, 'none', True, True),
            (0, 'relutanh', False, True), (1, 'none', False, False), (2, 'tanh', False, False),
            (0, 'none', True, False), (1, 'tanh', True, True), (2, 'relutanh', True, False))
GATE_NAMES = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')
# the library's name of a weight -> the oracle's
ORACLE_KEY = {'S1': 'S1', 'S2': 'S2', 'W': 'wildcard_mat', 'C': 'C_output_mat', 'h0': 'h0', 'hT': 'hT', 'crf_trans': 'crf.transitions',
              **{k: k for k in GATE_NAMES}}
SIG_K = 5.0
LABELS = 4                                                        # real labels; K = LABELS + 1 ("O" column), + 2 more under the CRF


def cases():
    out = []
    for i, (S, R) in enumerate(SHAPES):
        for j, (B, L, lens) in enumerate(BATCHES):
            farnn, nl, crf, prio = VARIANTS[(i * 7 + j) % len(VARIANTS)]
            out.append(dict(name='S{}R{}-B{}L{}{}-f{}-{}{}{}'.format(S, R, B, L, 'full' if min(lens) == L else '', farnn, nl,
                                                                   '-crf' if crf else '', '-P' if prio else ''),
                            S=S, R=R, B=B, L=L, lengths=lens, farnn=farnn, nl=nl, crf=crf, prio=prio, seed=100 * i + j))
    return out


CASES = cases()
CASE_IDS = [c['name'] for c in CASES]


def by_name(name):
    return CASES[CASE_IDS.index(name)]


def draw(case):
    """(p, v, lengths, labels): p the oracle's parameter dict (float32 torch tensors, without the leaf for v), v float32
    [B, L, R] numpy, int64 lengths [B] and labels [B, L]."""
    S, R, B, L, farnn = case['S'], case['R'], case['B'], case['L'], case['farnn']
    K = LABELS + 1 + (2 if case['crf'] else 0)
    rng = np.random.RandomState(case['seed'])
    f = lambda *shape, sc=0.3: torch.from_numpy((rng.randn(*shape) * sc).astype(np.float32))   # noqa: E731
    Cm = np.zeros((K, S), np.float32)
    Cm[rng.randint(0, K, size=S), np.arange(S)] = (rng.rand(S) < 0.8)
    p = {'S1': f(S, R, sc=1.0 / np.sqrt(S)), 'S2': f(S, R, sc=1.0 / np.sqrt(S)),
         'C_output_mat': torch.from_numpy(Cm + (rng.rand(K, S) * 0.02).astype(np.float32)),
         'wildcard_mat': torch.from_numpy(((rng.rand(S, S) < 1.0 / S) * 0.5).astype(np.float32)),
         'h0': f(S, sc=0.5), 'hT': f(S, sc=0.5),
         'priority_mat': torch.from_numpy((np.eye(K) + (rng.rand(K, K) < 0.05) * 0.5).astype(np.float32))}
    for g in range(farnn):
        p['Wss%d' % (g + 1)] = f(S, S, sc=0.3 / np.sqrt(S))
        p['Wrs%d' % (g + 1)] = f(R, S, sc=0.3 / np.sqrt(R))
        p['bs%d' % (g + 1)] = f(1, S, sc=0.2)
    if case['crf']:
        tr = (rng.randn(K, K) * 0.1).astype(np.float32)
        tr[:, K - 2] = -10000.0
        tr[K - 1, :] = -10000.0
        p['crf.transitions'] = torch.from_numpy(tr)
    v = (rng.randn(B, L, R) * 0.8).astype(np.float32)
    lengths = np.asarray(case['lengths'], np.int64)
    labels = rng.randint(0, LABELS + 1, size=(B, L)).astype(np.int64)
    return p, v, lengths, labels


def valid_mask(lengths, L):
    return np.arange(L)[None, :] < np.asarray(lengths)[:, None]


def oracle_step(p, v, lengths, labels, case, dtype=torch.float32):
    """(loss, {oracle key: gradient as numpy, 'v': [B, L, R]}, flat scores [sum len, K]) of the oracle in `dtype`."""
    B, L, R = v.shape
    q = {k: t.to(dtype) for k, t in p.items()}
    q.update({'V_embed': torch.from_numpy(np.ascontiguousarray(v).reshape(B * L, R)).to(dtype), 'beta_vec': torch.ones(R, dtype=dtype),
              'embedding.weight': torch.zeros(B * L, 1, dtype=dtype), 'embed_r_generalized': torch.zeros(1, R, dtype=dtype)})
    x = torch.arange(B * L, dtype=torch.int64).reshape(B, L)
    loss, g, s = to.train_step(q, x, torch.from_numpy(np.asarray(lengths)), torch.from_numpy(labels), nl=case['nl'],
                               use_priority=case['prio'], farnn=case['farnn'], sig_k=SIG_K)
    grads = {k: t.numpy() for k, t in g.items() if k not in ('V_embed', 'beta_vec', 'embedding.weight', 'embed_r_generalized')}
    grads['v'] = g['V_embed'].numpy().reshape(B, L, R)
    return float(loss), grads, s.numpy()


@functools.lru_cache(maxsize=None)
def refs(name):
    """The drawn inputs and both references of a case, computed once: (p, v, lengths, labels, ref32, ref64), a reference being
    (loss, grads, flat scores).  Callers leave them unchanged."""
    case = by_name(name)
    p, v, lengths, labels = draw(case)
    return p, v, lengths, labels, oracle_step(p, v, lengths, labels, case), oracle_step(p, v, lengths, labels, case, torch.float64)


def decided_tags(s64_flat, lengths, L, threshold, crf_tr=None):
    """bool [B, L]: the valid positions whose tag the float64 scores (flat, [sum len, K]) decide beyond the float path's error --
    tests/sf_tag_ref.decided, called on the sequences that have a token (its CRF branch walks none of length 0)."""
    lengths = np.asarray(lengths)
    B, K = len(lengths), s64_flat.shape[1]
    s64 = np.zeros((B, L, K))
    s64[valid_mask(lengths, L)] = s64_flat
    out = np.zeros((B, L), bool)
    some = lengths > 0
    out[some] = sf_tag_ref.decided(s64[some], lengths[some], threshold, crf_tr)
    return out


def grad_names(case):
    """the library's names of the weights whose gradient the step returns"""
    return ('S1', 'S2', 'W', 'C', 'h0', 'hT') + GATE_NAMES[:3 * case['farnn']] + (('crf_trans',) if case['crf'] else ())


def check_all(case, got_loss, got, ref32, ref64, lengths, check_grad, tol=TOL):
    """The loss, every weight gradient and dv under tests/util.check_grad (dv: row by row at each valid position's own scale,
    exact zeros at the pads).  got: {library name: array, 'v': dv [B, L, R]}."""
    l32, g32, _ = ref32
    l64, g64, _ = ref64
    assert abs(got_loss - l64) <= tol * (1 + abs(l64)) and abs(got_loss - l32) <= tol * (1 + abs(l32)) + abs(l32 - l64), \
        '{} loss {} against {} (float64 {})'.format(case['name'], got_loss, l32, l64)
    for n in grad_names(case):
        k = ORACLE_KEY[n]
        check_grad(case['name'], 'd' + n, np.asarray(got[n]).reshape(g64[k].shape), g32[k], g64[k], tol=tol)
    B, L, R = got['v'].shape
    present = valid_mask(lengths, L).reshape(-1)
    check_grad(case['name'], 'dv', got['v'].reshape(B * L, R), g32['v'].reshape(B * L, R), g64['v'].reshape(B * L, R), tol=tol,
               slices=0, present=present)


# ---- d loss / d v split into the three terms sf_dv_kernel adds (the planted-fault check) --------------------------------------
def split_dv(p, v, lengths, labels, case):
    """(loss, DVf, DVb, GT) in float64, each [B, L, R] indexed by (sequence, STEP of its chain): DVf[b, i] the forward chain's
    share of d v at its step i (token i), DVb[b, j] the backward chain's at its step j (token len - 1 - j), GT[b, i] both gates'
    share for token i.  The same recurrence as the oracle's chain_scores, with one leaf per use of a vector: the caller holds
    their sum to the oracle's gradient before using them."""
    dt = torch.float64
    q = {k: t.to(dt) for k, t in p.items()}
    B, L, R = v.shape
    farnn, nl = case['farnn'], case['nl']
    vv = torch.from_numpy(v).to(dt)
    vf, vb, vg = (vv.clone().requires_grad_(True) for _ in range(3))
    osum = q['C_output_mat'].sum(0)

    def step(h, vc, vgate, h_init, fwd):
        if farnn >= 1:
            z = torch.sigmoid(SIG_K * (h @ q['Wss1'] + vgate @ q['Wrs1'] + q['bs1'].reshape(-1)))
        hbar = h
        if farnn == 2:
            r = torch.sigmoid(SIG_K * (h @ q['Wss2'] + vgate @ q['Wrs2'] + q['bs2'].reshape(-1)))
            hbar = (1 - r) * h_init + r * h
        if fwd:
            nxt = to._nl((((hbar @ q['S1']) * vc) @ q['S2'].T + hbar @ q['wildcard_mat']) * osum, nl)
        else:
            bb = hbar * osum
            nxt = to._nl(((bb @ q['S2']) * vc) @ q['S1'].T + bb @ q['wildcard_mat'].T, nl)
        return nxt if farnn == 0 else (1 - z) * h + z * nxt

    flat = []
    for b in range(B):
        n = int(lengths[b])
        if n == 0:
            continue
        fs, bs = [q['h0']], [q['hT']]
        for i in range(n):
            fs.append(step(fs[-1], vf[b, i], vg[b, i], q['h0'], True))
        for j in range(n):
            bs.append(step(bs[-1], vb[b, n - 1 - j], vg[b, n - 1 - j], q['hT'], False))
        for i in range(n):
            flat.append((fs[i + 1] * bs[n - 1 - i]) @ q['C_output_mat'].T)
    s = torch.stack(flat)
    if case['prio']:
        s = s @ q['priority_mat']
    if case['crf']:
        loss = to.crf_nll(s, lengths, torch.from_numpy(labels), q['crf.transitions'])
    else:
        loss = torch.nn.functional.cross_entropy(s, torch.cat([torch.from_numpy(labels[b, :int(lengths[b])]) for b in range(B)]))
    loss.backward()
    DVb = np.zeros_like(v, dtype=np.float64)                                  # by the backward chain's step, as the kernel stores it
    for b in range(B):
        n = int(lengths[b])
        DVb[b, :n] = vb.grad.numpy()[b, :n][::-1]
    return float(loss.detach()), vf.grad.numpy(), DVb, vg.grad.numpy()


def assemble_dv(DVf, DVb, GT, lengths, backward_row='len-t', gate=True):
    """dv[b, t] = DVf[b, t] + DVb[b, len - 1 - t] + GT[b, t] at the valid positions, zeros at the pads -- sf_dv_kernel's sum
    (its stash rows are one further: step i is row i + 1).  backward_row='t' and gate=False are the planted faults."""
    B, L, R = DVf.shape
    dv = np.zeros((B, L, R))
    for b in range(B):
        n = int(lengths[b])
        for t in range(n):
            dv[b, t] = DVf[b, t] + DVb[b, n - 1 - t if backward_row == 'len-t' else t]
            if gate:
                dv[b, t] = dv[b, t] + GT[b, t]
    return dv
