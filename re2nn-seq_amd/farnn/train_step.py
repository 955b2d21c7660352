"""The training steps on the HIP path: one torch.autograd.Function (_TrainStep) around farnn_decomp_ifst_train_step,
farnn_onehot_ifst_train_step, farnn_fst4_train_step, farnn_ind1_train_step, farnn_decomp_ind1_train_step and
farnn_decomp_sf_train_step (include/farnn.h).
Each public function below describes its weights to it (the C struct's field, the tensor, when its gradient is asked of the
library) and, where the call is not the context's plain step(), makes the library call itself (teacher_step, step_crf).

What the reference does in FARNN_S_D_W_I_S.forward_local(train=True) + loss.backward()
(model_decompose_single.py:207-304, train_decompose.py:186-190) is split like this: the word table
Vgen = V_embed*beta + act(E G)*(1-beta) (model_decompose.py:222-241) is built for the whole vocabulary
by ordinary torch ops (one [V,D]x[D,R] product: its gradient flows to the embedding, the bridge matrix,
V_embed and beta through torch's autograd); everything that depends on the batch -- both chains, the
scores, the cross-entropy and the back-propagation through time -- is one library call.  The library
computes loss and all gradients in its forward call (the stash lives in its workspace); backward()
only hands them out, scaled by the incoming gradient.

Scope: farnn = 0/1/2, sum or max semiring (TrainContext(semiring=...)), CE1 loss or (use_crf) the CRF
negative log-likelihood; in either semiring also with the KD / PR teacher term (teacher=...; on a max context through
farnn_decomp_ifst_teacher_max_train_step, TrainContext(teacher_max=True)).

The onehot i-FST (FARNN_S_O_I_S, model_onehot.py:351-428 + train_onehot.py:156-206) trains only
language_tensor: one library call computes the loss, the tags and d loss / d language_tensor.

The onehot FST (FARNN_S_O, model_onehot.py:66-146) trains language_tensor [V,C,S,S] and, with
--train_wildcard, wildcard_tensor [C,S,S]: again one library call.

The onehot independent=1 model (FARNN_S_O_I, model_onehot.py:184-306) trains language_tensor [V,S,S]
only: one library call.

The decomposed independent=1 model (FARNN_S_D_W_I, model_decompose_independent.py:148-300): the word table as
for f3 through torch's autograd, and one library call (farnn_decomp_ind1_train_step) for the loss, the tags and the gradients of
Vgen, S1, S2, wildcard_mat, C_output, S1_output, S2_output, h0 and hT.  Under --use_crf 1 (crf_trans given) the call is
farnn_decomp_ind1_crf_train_step: the CRF's negative log-likelihood, the Viterbi tags and the transitions' gradient as well.
With the gates of --farnn 1 | 2 (gates=...) the call is farnn_decomp_ind1_gated_train_step, with or without crf_trans: the
gates' gradients as well; on a max context (--train_mode max) it is farnn_decomp_ind1_gated_max_train_step.
"""
import torch

from .. import _lib


GATE_NAMES = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')


def _f32(t):
    return None if t is None else t.detach().contiguous().float()


def _step_inputs(ref, ntok, x, lengths, labels):
    """What both steps do before the library call: the device check on `ref` (a weight), the token count, x / lengths /
    labels on the device, the loss and tags outputs.  Returns (dev, ntok, x, lengths, labels, loss, tags)."""
    dev = ref.device
    if dev.type != 'cuda':
        raise _lib.FarnnError('the training step runs on the HIP device only (no CPU fallback)')
    B, L = x.shape
    if ntok is None:            # counted on the host when the lengths live there (no device round trip in the step)
        ntok = int(lengths.clamp(0, L).sum())
    x, lengths, labels = (t.to(dev).contiguous() for t in (x, lengths, labels))
    if ntok <= 0:
        raise ValueError('empty batch')
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    tags = torch.empty((B, L), dtype=torch.int32, device=dev)
    return dev, ntok, x, lengths, labels, loss, tags


ALWAYS, IF_REQUIRED, NEVER = 'always', 'if it requires one', 'never'      # when a weight's gradient is asked of the library
_GRAD_FIELD = {'crf_trans': 'dtrans'}                                      # the outputs struct's field, where it is not 'd' + name


class _TrainStep(torch.autograd.Function):
    """One library step.  names / wants / tensors describe the weights: the field of the C weights struct, when the gradient
    is wanted, and the tensor (None: a null pointer and no gradient).  call(weights, ptrs, dims, outputs, stream) makes the
    library call, with ptrs = the device pointers of x, lengths and labels and dims = (B, L, valid_tokens); None is tc.step."""
    @staticmethod
    def forward(ctx, tc, ntok, x, lengths, labels, call, names, wants, *tensors):
        dev, ntok, x, lengths, labels, loss, tags = _step_inputs(tensors[0], ntok, x, lengths, labels)
        ws = [_f32(t) for t in tensors]
        grads = [torch.empty_like(w) if w is not None and (want == ALWAYS or (want == IF_REQUIRED and t.requires_grad)) else None
                 for t, w, want in zip(tensors, ws, wants)]
        weights = {n: None if w is None else w.data_ptr() for n, w in zip(names, ws)}
        outputs = {_GRAD_FIELD.get(n, 'd' + n): None if g is None else g.data_ptr() for n, g in zip(names, grads)}
        outputs['loss'] = loss.data_ptr()
        outputs['tags'] = tags.data_ptr()
        (call or _plain(tc))(weights, (x.data_ptr(), lengths.data_ptr(), labels.data_ptr()), tuple(x.shape) + (ntok,), outputs,
                             torch.cuda.current_stream(dev).cuda_stream)
        ctx.have = tuple(g is not None for g in grads)
        ctx.save_for_backward(*[g for g in grads if g is not None])
        ctx.mark_non_differentiable(tags)
        return loss.reshape(()), tags

    @staticmethod
    def backward(ctx, gloss, _gtags):
        saved = iter(ctx.saved_tensors)
        return (None,) * 8 + tuple(next(saved) * gloss if h else None for h in ctx.have)


def _plain(tc):
    return lambda weights, ptrs, dims, outputs, stream: tc.step(weights, *ptrs, *dims, outputs, stream)


def _step(tc, ntok, x, lengths, labels, spec, call=None):
    """spec: (name, tensor, ALWAYS | IF_REQUIRED | NEVER) per weight; the first one is a tensor and names the device."""
    names, tensors, wants = zip(*spec)
    return _TrainStep.apply(tc, ntok, x, lengths, labels, call, names, wants, *tensors)


def decomp_ifst_train_step(tc, Vgen, S1, S2, W, Cmat, h0, hT, P, x, lengths, labels, crf_trans=None, gates=(),
                           valid_tokens=None, teacher=None):
    """Returns (loss scalar tensor with grad, tags int32 [B,L] with -1 at pads).  gates: the tensors Wss1, Wrs1, bs1
    (farnn = 1) followed by Wss2, Wrs2, bs2 (farnn = 2), in that order.  valid_tokens: sum of the clamped lengths if
    the caller already has it (device-resident lengths would otherwise cost a synchronising read per step).
    teacher: None, or (re_scores [B,L,K] with the zero columns appended, 'kd' | 'pr', c1, pi) for
    loss = pi * original + (1 - pi) * KL (farnn_decomp_ifst_teacher_train_step / _teacher_max_train_step, include/farnn.h); the teacher scores get no
    gradient."""
    call = None
    if teacher is not None:
        def call(weights, ptrs, dims, outputs, stream):
            re, mode, c1, pi = teacher
            re = re.detach().to(Vgen.device).float().contiguous()
            if tuple(re.shape) != dims[:2] + (Cmat.shape[0],):
                raise ValueError('teacher scores must be [B, L, K] = {}, not {}'.format(dims[:2] + (Cmat.shape[0],), tuple(re.shape)))
            tc.teacher_step(weights, *ptrs, re.data_ptr(), mode, c1, pi, *dims, outputs, stream)
    spec = [(n, t, ALWAYS) for n, t in zip(('Vgen', 'S1', 'S2', 'W', 'C', 'h0', 'hT'), (Vgen, S1, S2, W, Cmat, h0, hT))]
    spec += [('P', P, NEVER), ('crf_trans', crf_trans, ALWAYS)] + [(n, g, ALWAYS) for n, g in zip(GATE_NAMES, gates)]
    return _step(tc, valid_tokens, x, lengths, labels, spec, call)


def decomp_sf_train_step(tc, v, S1, S2, W, Cmat, h0, hT, P, lengths, labels, crf_trans=None, gates=(), valid_tokens=None):
    """The vector-input i-FST (FARNN_S_SF, model_decompose_single.py:483-580), sum semiring, no teacher: returns
    (loss scalar tensor with grad, tags int32 [B,L] with -1 at pads).  v [B, >= L, R] is a differentiable input, L =
    labels.shape[1]: v[:, :L] is made contiguous float32 on the weights' device, and its gradient (exact zeros at the pad
    positions, bit-identical from call to call) comes back scaled by the incoming gradient, like the weights'.  One library call
    (farnn_decomp_sf_train_step on an _lib.SfTrainContext).  gates, crf_trans, valid_tokens: as decomp_ifst_train_step's."""
    if len(gates) not in (0, 3, 6):
        raise ValueError('gates: none, Wss1 Wrs1 bs1 (farnn 1) or those and Wss2 Wrs2 bs2 (farnn 2), not {} tensors'.format(len(gates)))
    B, L = labels.shape
    if v.dim() != 3 or v.shape[0] != B or v.shape[1] < L or v.shape[2] != S1.shape[1]:
        raise ValueError('v must be [B, >= L, R] = [{}, >= {}, {}], not {}'.format(B, L, S1.shape[1], tuple(v.shape)))
    v = v[:, :L].to(device=S1.device)

    def call(weights, ptrs, dims, outputs, stream):
        tc.step_vectors(weights, weights['v'], ptrs[1], ptrs[2], *dims, outputs, outputs['dv'], stream)
    spec = [(n, t, ALWAYS) for n, t in zip(('S1', 'S2', 'W', 'C', 'h0', 'hT'), (S1, S2, W, Cmat, h0, hT))]
    spec += [('v', v, ALWAYS), ('P', P, NEVER), ('crf_trans', crf_trans, ALWAYS)] + [(n, g, ALWAYS) for n, g in zip(GATE_NAMES, gates)]
    return _step(tc, valid_tokens, labels, lengths, labels, spec, call)      # (x only gives the step its [B, L])


_D0_NAMES = ('Vgen', 'Ce', 'S1', 'S2', 'Cw', 'S1w', 'S2w', 'WW', 'h0', 'hT')


def decomp_fst_train_step(tc, Vgen, Ce, S1, S2, Cw, S1w, S2w, WW, h0, hT, P, x, lengths, labels, crf_trans=None, gates=(),
                          valid_tokens=None):
    """The decomposed FST (FARNN_S_D_W, model_decompose.py:243-456), sum semiring: returns (loss scalar tensor
    with grad, tags int32 [B,L] with -1 at pads).  One library call (farnn_decomp_fst_train_step) computes the loss (CE1, or the
    CRF's negative log-likelihood when crf_trans is given), the tags and the gradients of Vgen [V,R] (which flows on through
    torch's autograd as for f3), C_embed, S1, S2, C_wildcard, S1_wildcard, S2_wildcard, wildcard_wildcard, h0, hT, the gates
    (as decomp_ifst_train_step's) and crf_trans.  P is read only."""
    if len(gates) not in (0, 3, 6):
        raise ValueError('gates: none, Wss1 Wrs1 bs1 (farnn 1) or those and Wss2 Wrs2 bs2 (farnn 2), not {} tensors'.format(len(gates)))
    spec = [(n, t, ALWAYS) for n, t in zip(_D0_NAMES, (Vgen, Ce, S1, S2, Cw, S1w, S2w, WW, h0, hT))]
    spec += [('P', P, NEVER), ('crf_trans', crf_trans, ALWAYS)] + [(n, g, ALWAYS) for n, g in zip(GATE_NAMES, gates)]
    return _step(tc, valid_tokens, x, lengths, labels, spec)


def _onehot_t_step(tc, T, W, O, h0, hT, P, x, lengths, labels, valid_tokens):
    """The onehot i-FST and the onehot independent=1 step: the same weights T, W, O, h0, hT and the one gradient dT; which
    library step runs is the context's (OnehotTrainContext or Ind1TrainContext)."""
    return _step(tc, valid_tokens, x, lengths, labels,
                 [('T', T, ALWAYS)] + [(n, t, NEVER) for n, t in (('W', W), ('O', O), ('h0', h0), ('hT', hT), ('P', P))])


def onehot_ifst_train_step(tc, T, W, O, h0, hT, P, x, lengths, labels, valid_tokens=None):
    """Returns (loss scalar tensor with grad towards T, tags int32 [B,L] with -1 at pads).  W, O, h0, hT and P are read
    but receive no gradient (the reference's requires_grad=False, model_onehot.py:326-337).  valid_tokens: the sum of
    the clamped lengths if the caller already has it."""
    return _onehot_t_step(tc, T, W, O, h0, hT, P, x, lengths, labels, valid_tokens)


def onehot_fst4_train_step(tc, T4, W4, h0, hT, P, x, lengths, labels, valid_tokens=None):
    """Returns (loss scalar tensor with grad towards T4 and, if it requires grad, W4; tags int32 [B,L] with -1 at pads).
    h0, hT and P are read but receive no gradient (model_onehot.py:32-33)."""
    return _step(tc, valid_tokens, x, lengths, labels,
                 [('T4', T4, ALWAYS), ('W4', W4, IF_REQUIRED), ('h0', h0, NEVER), ('hT', hT, NEVER), ('P', P, NEVER)])


def onehot_ind1_train_step(tc, T, W, O, h0, hT, P, x, lengths, labels, valid_tokens=None):
    """Returns (loss scalar tensor with grad towards T, tags int32 [B,L] with -1 at pads).  W [S,S], O [C,S,S], h0, hT and
    P are read but receive no gradient (the reference's requires_grad=False, model_onehot.py:209-223).  Whether the chains
    run on (T + W) * O.sum(0) (args.independent == 2) is the context's mask_by_output."""
    return _onehot_t_step(tc, T, W, O, h0, hT, P, x, lengths, labels, valid_tokens)


_D1_NAMES = ('Vgen', 'S1', 'S2', 'W', 'C', 'S1o', 'S2o', 'h0', 'hT')
_D1_OPTIONAL = ('W', 'C', 'S1o', 'S2o', 'h0', 'hT')       # gradients the library writes only when asked (include/farnn.h)


def decomp_ind1_train_step(tc, Vgen, S1, S2, W, Cout, S1o, S2o, h0, hT, P, x, lengths, labels, valid_tokens=None,
                           crf_trans=None, gates=(), sigmoid_exponent=5.0):
    """The decomposed independent=1 model (FARNN_S_D_W_I, model_decompose_independent.py:219-300): returns
    (loss scalar tensor with grad, tags int32 [B,L] with -1 at pads).  Vgen [V,R] (its gradient flows on through torch's
    autograd to V_embed, embed_r_generalized, embedding.weight and beta_vec), S1 and S2 always get a gradient; wildcard_mat W,
    C_output, S1_output, S2_output, h0 and hT get one when they require it and None otherwise.  P is read only.
    crf_trans [C,C] (C counts START and STOP): the loss is the CRF's negative log-likelihood, a sum over the sequences, the
    tags are the Viterbi path, and crf_trans gets a gradient (farnn_decomp_ind1_crf_train_step).
    gates: as decomp_ifst_train_step's -- Wss1, Wrs1, bs1 (farnn = 1) followed by Wss2, Wrs2, bs2 (farnn = 2); with them the
    call is farnn_decomp_ind1_gated_train_step (with or without crf_trans; farnn_decomp_ind1_gated_max_train_step when the
    context's semiring is 'max'), every gate gets a gradient, and sigmoid_exponent is the gates' k."""
    call = None
    if len(gates) not in (0, 3, 6):
        raise ValueError('gates: none, Wss1 Wrs1 bs1 (farnn 1) or those and Wss2 Wrs2 bs2 (farnn 2), not {} tensors'.format(len(gates)))
    if crf_trans is not None or gates:
        def call(weights, ptrs, dims, outputs, stream):
            if crf_trans is not None and tuple(crf_trans.shape) != (Cout.shape[0],) * 2:
                raise ValueError('CRF transitions must be [C, C] = {}, not {}'.format((Cout.shape[0],) * 2, tuple(crf_trans.shape)))
            if gates:
                step = tc.gated_max_step if tc.semiring == 'max' else tc.gated_step
                step(weights, len(gates) // 3, sigmoid_exponent, *ptrs, *dims, outputs, stream,
                     trans_ptr=weights.get('crf_trans'), dtrans_ptr=outputs.get('dtrans'))
            else:
                tc.step_crf(weights, weights['crf_trans'], *ptrs, *dims, outputs, outputs['dtrans'], stream)
    spec = [(n, t, IF_REQUIRED if n in _D1_OPTIONAL else ALWAYS) for n, t in zip(_D1_NAMES, (Vgen, S1, S2, W, Cout, S1o, S2o, h0, hT))]
    spec += [('P', P, NEVER), ('crf_trans', crf_trans, ALWAYS)] + [(n, g, ALWAYS) for n, g in zip(GATE_NAMES, gates)]
    return _step(tc, valid_tokens, x, lengths, labels, spec, call)
