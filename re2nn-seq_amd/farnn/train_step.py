"""The training steps on the HIP path, as torch.autograd.Functions around farnn_decomp_ifst_train_step,
farnn_onehot_ifst_train_step, farnn_fst4_train_step, farnn_ind1_train_step and farnn_decomp_ind1_train_step (include/farnn.h).

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


class _DecompIfstTrainStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tc, ntok, x, lengths, labels, teacher, P, Vgen, S1, S2, W, Cmat, h0, hT, trans, *gates):
        dev, ntok, x, lengths, labels, loss, tags = _step_inputs(Vgen, ntok, x, lengths, labels)
        B, L = x.shape
        ws = [_f32(t) for t in (Vgen, S1, S2, W, Cmat, h0, hT)]
        Pc, tr = _f32(P), _f32(trans)
        gs = [_f32(g) for g in gates]
        grads = [torch.empty_like(t) for t in ws]
        gtr = None if tr is None else torch.empty_like(tr)
        ggs = [torch.empty_like(g) for g in gs]
        names = ('Vgen', 'S1', 'S2', 'W', 'C', 'h0', 'hT')
        weights = {n: t.data_ptr() for n, t in zip(names, ws)}
        weights['P'] = None if Pc is None else Pc.data_ptr()
        weights['crf_trans'] = None if tr is None else tr.data_ptr()
        outputs = {'d' + n: g.data_ptr() for n, g in zip(names, grads)}
        outputs['loss'] = loss.data_ptr()
        outputs['tags'] = tags.data_ptr()
        outputs['dtrans'] = None if gtr is None else gtr.data_ptr()
        for n, g, gg in zip(GATE_NAMES, gs, ggs):
            weights[n] = g.data_ptr()
            outputs['d' + n] = gg.data_ptr()
        stream = torch.cuda.current_stream(dev).cuda_stream
        if teacher is None:
            tc.step(weights, x.data_ptr(), lengths.data_ptr(), labels.data_ptr(), B, L, ntok, outputs, stream)
        else:
            re, mode, c1, pi = teacher
            re = re.detach().to(dev).float().contiguous()
            if tuple(re.shape) != (B, L, Cmat.shape[0]):
                raise ValueError('teacher scores must be [B, L, K] = {}, not {}'.format((B, L, Cmat.shape[0]), tuple(re.shape)))
            tc.teacher_step(weights, x.data_ptr(), lengths.data_ptr(), labels.data_ptr(), re.data_ptr(), mode, c1, pi, B, L,
                            ntok, outputs, stream)
        ctx.has_tr = gtr is not None
        ctx.n_gates = len(gs)
        ctx.save_for_backward(*(grads + ([gtr] if gtr is not None else []) + ggs))
        ctx.mark_non_differentiable(tags)
        return loss.reshape(()), tags

    @staticmethod
    def backward(ctx, gloss, _gtags):
        saved = ctx.saved_tensors
        grads = [g * gloss for g in saved[:7]]
        k = 7
        gtr = None
        if ctx.has_tr:
            gtr = saved[k] * gloss
            k += 1
        ggs = [g * gloss for g in saved[k:k + ctx.n_gates]]
        return (None, None, None, None, None, None, None) + tuple(grads) + (gtr,) + tuple(ggs)


def decomp_ifst_train_step(tc, Vgen, S1, S2, W, Cmat, h0, hT, P, x, lengths, labels, crf_trans=None, gates=(),
                           valid_tokens=None, teacher=None):
    """Returns (loss scalar tensor with grad, tags int32 [B,L] with -1 at pads).  gates: the tensors Wss1, Wrs1, bs1
    (farnn = 1) followed by Wss2, Wrs2, bs2 (farnn = 2), in that order.  valid_tokens: sum of the clamped lengths if
    the caller already has it (device-resident lengths would otherwise cost a synchronising read per step).
    teacher: None, or (re_scores [B,L,K] with the zero columns appended, 'kd' | 'pr', c1, pi) for
    loss = pi * original + (1 - pi) * KL (farnn_decomp_ifst_teacher_train_step / _teacher_max_train_step, include/farnn.h); the teacher scores get no
    gradient."""
    return _DecompIfstTrainStep.apply(tc, valid_tokens, x, lengths, labels, teacher, P, Vgen, S1, S2, W, Cmat, h0, hT, crf_trans,
                                      *gates)


class _OnehotTTrainStep(torch.autograd.Function):
    """The onehot i-FST and the onehot independent=1 step: the same weights T, W, O, h0, hT and the one gradient dT; which
    library step runs is the context's (OnehotTrainContext or Ind1TrainContext)."""
    @staticmethod
    def forward(ctx, tc, ntok, x, lengths, labels, P, W, O, h0, hT, T):
        dev, ntok, x, lengths, labels, loss, tags = _step_inputs(T, ntok, x, lengths, labels)
        B, L = x.shape
        ws = {n: _f32(t) for n, t in (('T', T), ('W', W), ('O', O), ('h0', h0), ('hT', hT))}
        Pc = _f32(P)
        dT = torch.empty_like(ws['T'])
        weights = {n: t.data_ptr() for n, t in ws.items()}
        weights['P'] = None if Pc is None else Pc.data_ptr()
        outputs = {'loss': loss.data_ptr(), 'dT': dT.data_ptr(), 'tags': tags.data_ptr()}
        tc.step(weights, x.data_ptr(), lengths.data_ptr(), labels.data_ptr(), B, L, ntok, outputs,
                torch.cuda.current_stream(dev).cuda_stream)
        ctx.save_for_backward(dT)
        ctx.mark_non_differentiable(tags)
        return loss.reshape(()), tags

    @staticmethod
    def backward(ctx, gloss, _gtags):
        dT, = ctx.saved_tensors
        return (None,) * 10 + (dT * gloss,)


def onehot_ifst_train_step(tc, T, W, O, h0, hT, P, x, lengths, labels, valid_tokens=None):
    """Returns (loss scalar tensor with grad towards T, tags int32 [B,L] with -1 at pads).  W, O, h0, hT and P are read
    but receive no gradient (the reference's requires_grad=False, model_onehot.py:326-337).  valid_tokens: the sum of
    the clamped lengths if the caller already has it."""
    return _OnehotTTrainStep.apply(tc, valid_tokens, x, lengths, labels, P, W, O, h0, hT, T)


class _OnehotFst4TrainStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tc, ntok, x, lengths, labels, P, h0, hT, T4, W4):
        dev, ntok, x, lengths, labels, loss, tags = _step_inputs(T4, ntok, x, lengths, labels)
        B, L = x.shape
        ws = {n: _f32(t) for n, t in (('T4', T4), ('W4', W4), ('h0', h0), ('hT', hT))}
        Pc = _f32(P)
        dT4 = torch.empty_like(ws['T4'])
        dW4 = torch.empty_like(ws['W4']) if W4.requires_grad else None
        weights = {n: t.data_ptr() for n, t in ws.items()}
        weights['P'] = None if Pc is None else Pc.data_ptr()
        outputs = {'loss': loss.data_ptr(), 'dT4': dT4.data_ptr(), 'dW4': None if dW4 is None else dW4.data_ptr(),
                   'tags': tags.data_ptr()}
        tc.step(weights, x.data_ptr(), lengths.data_ptr(), labels.data_ptr(), B, L, ntok, outputs,
                torch.cuda.current_stream(dev).cuda_stream)
        ctx.has_w = dW4 is not None
        ctx.save_for_backward(*([dT4] + ([dW4] if dW4 is not None else [])))
        ctx.mark_non_differentiable(tags)
        return loss.reshape(()), tags

    @staticmethod
    def backward(ctx, gloss, _gtags):
        saved = ctx.saved_tensors
        return (None,) * 8 + (saved[0] * gloss, saved[1] * gloss if ctx.has_w else None)


def onehot_fst4_train_step(tc, T4, W4, h0, hT, P, x, lengths, labels, valid_tokens=None):
    """Returns (loss scalar tensor with grad towards T4 and, if it requires grad, W4; tags int32 [B,L] with -1 at pads).
    h0, hT and P are read but receive no gradient (model_onehot.py:32-33)."""
    return _OnehotFst4TrainStep.apply(tc, valid_tokens, x, lengths, labels, P, h0, hT, T4, W4)


def onehot_ind1_train_step(tc, T, W, O, h0, hT, P, x, lengths, labels, valid_tokens=None):
    """Returns (loss scalar tensor with grad towards T, tags int32 [B,L] with -1 at pads).  W [S,S], O [C,S,S], h0, hT and
    P are read but receive no gradient (the reference's requires_grad=False, model_onehot.py:209-223).  Whether the chains
    run on (T + W) * O.sum(0) (args.independent == 2) is the context's mask_by_output."""
    return _OnehotTTrainStep.apply(tc, valid_tokens, x, lengths, labels, P, W, O, h0, hT, T)


_D1_NAMES = ('Vgen', 'S1', 'S2', 'W', 'C', 'S1o', 'S2o', 'h0', 'hT')
_D1_OPTIONAL = ('W', 'C', 'S1o', 'S2o', 'h0', 'hT')       # gradients the library writes only when asked (include/farnn.h)


class _DecompInd1TrainStep(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tc, ntok, x, lengths, labels, P, Vgen, S1, S2, W, Cout, S1o, S2o, h0, hT, trans):
        dev, ntok, x, lengths, labels, loss, tags = _step_inputs(S1, ntok, x, lengths, labels)
        B, L = x.shape
        ts = dict(zip(_D1_NAMES, (Vgen, S1, S2, W, Cout, S1o, S2o, h0, hT)))
        ws = {n: _f32(t) for n, t in ts.items()}
        Pc, tr = _f32(P), _f32(trans)
        grads = {n: torch.empty_like(ws[n]) for n in _D1_NAMES if n not in _D1_OPTIONAL or ts[n].requires_grad}
        weights = {n: t.data_ptr() for n, t in ws.items()}
        weights['P'] = None if Pc is None else Pc.data_ptr()
        outputs = {'d' + n: (grads[n].data_ptr() if n in grads else None) for n in _D1_NAMES}
        outputs['loss'] = loss.data_ptr()
        outputs['tags'] = tags.data_ptr()
        stream = torch.cuda.current_stream(dev).cuda_stream
        if tr is None:
            tc.step(weights, x.data_ptr(), lengths.data_ptr(), labels.data_ptr(), B, L, ntok, outputs, stream)
        else:
            if tuple(tr.shape) != (Cout.shape[0],) * 2:
                raise ValueError('CRF transitions must be [C, C] = {}, not {}'.format((Cout.shape[0],) * 2, tuple(tr.shape)))
            grads['trans'] = torch.empty_like(tr)
            tc.step_crf(weights, tr.data_ptr(), x.data_ptr(), lengths.data_ptr(), labels.data_ptr(), B, L, ntok, outputs,
                        grads['trans'].data_ptr(), stream)
        ctx.have = tuple(n in grads for n in _D1_NAMES + ('trans',))
        ctx.save_for_backward(*[grads[n] for n in _D1_NAMES + ('trans',) if n in grads])
        ctx.mark_non_differentiable(tags)
        return loss.reshape(()), tags

    @staticmethod
    def backward(ctx, gloss, _gtags):
        saved = iter(ctx.saved_tensors)
        return (None,) * 6 + tuple(next(saved) * gloss if h else None for h in ctx.have)


def decomp_ind1_train_step(tc, Vgen, S1, S2, W, Cout, S1o, S2o, h0, hT, P, x, lengths, labels, valid_tokens=None,
                           crf_trans=None):
    """The decomposed independent=1 model (FARNN_S_D_W_I, model_decompose_independent.py:219-300): returns
    (loss scalar tensor with grad, tags int32 [B,L] with -1 at pads).  Vgen [V,R] (its gradient flows on through torch's
    autograd to V_embed, embed_r_generalized, embedding.weight and beta_vec), S1 and S2 always get a gradient; wildcard_mat W,
    C_output, S1_output, S2_output, h0 and hT get one when they require it and None otherwise.  P is read only.
    crf_trans [C,C] (C counts START and STOP): the loss is the CRF's negative log-likelihood, a sum over the sequences, the
    tags are the Viterbi path, and crf_trans gets a gradient (farnn_decomp_ind1_crf_train_step)."""
    return _DecompInd1TrainStep.apply(tc, valid_tokens, x, lengths, labels, P, Vgen, S1, S2, W, Cout, S1o, S2o, h0, hT, crf_trans)
