"""Host mirror of the reference's decomposed i-FST tagger ``FARNN_S_D_W_I_S``
(src_seq/farnn/model_decompose_single.py:12-304; shared pieces from model_decompose.py).

The constructor keeps the reference's argument list and builds the same parameter set
(state padding with ``additional_states``, the pseudo-inverse word-embedding bridge, optional
GRU-style gates, optional CRF) with torch CPU ops; inference runs in the HIP library.  Because the
weights are frozen on the tagging path, the per-token ``get_generalized_v_embed_vec``
(model_decompose.py:222-241) is folded once into a table ``Vgen[V,R]`` when the device handle is
built -- the reference recomputes it twice per time step.
"""
import numpy as np
import torch

from .. import _lib
from . import train_step
from ._native import NativeTagger, opted_in
from ._trainable import Trainable
from .priority import expand_priority

_GATE_KEYS = ('Wss1', 'Wrs1', 'bs1', 'Wss2', 'Wrs2', 'bs2')
_PARAM_KEYS = ('S1', 'S2', 'V_embed', 'embed_r_generalized', 'C_output_mat', 'wildcard_mat',
               'wildcard_output_vector', 'h0', 'hT', 'beta_vec') + _GATE_KEYS


def crf_default_transitions(tagset_size):
    """CRF.__init__ of the reference (baselines/crf.py:31-46)."""
    K = tagset_size + 2
    tr = torch.zeros(K, K)
    tr[:, K - 2] = -10000.0
    tr[K - 1, :] = -10000.0
    return tr


class FARNN_S_D_W_I_S(Trainable, NativeTagger):
    _param_keys = _PARAM_KEYS
    local_uses_max_len = True        # forward_local iterates lengths.max() positions (ref :221)
    _check_needs_re_tags = True      # so enable_training() and train_onehot.check_trainable() leave the check to forward_local

    def __init__(self, V=None, S1=None, S2=None, C_output_mat=None, wildcard_mat=None,
                 wildcard_output_vector=None, final_vector=None, start_vector=None,
                 pretrained_word_embed=None, priority_mat=None, args=None, o_idx=0, is_cuda=True):
        super().__init__(args, o_idx)
        self.additional_states = int(args.additional_states)
        self.embedding = torch.from_numpy(np.asarray(pretrained_word_embed)).float()       # V x D
        self.C = C_output_mat.shape[0]
        self.S, self.R = S1.shape
        self.use_crf = bool(args.use_crf)
        self.crf_transitions = None
        if self.use_crf:
            self.crf_transitions = crf_default_transitions(self.C)
            self.C += 2
        self.priority_full = expand_priority(self.C, priority_mat)
        self.random = bool(args.random)
        self.h0 = self.pad_additional_states(torch.from_numpy(np.asarray(start_vector)).float())
        self.hT = self.pad_additional_states(torch.from_numpy(np.asarray(final_vector)).float())
        self._init_forward_parameters(S1, S2, V, C_output_mat, wildcard_mat, wildcard_output_vector)
        self.beta = args.beta
        self.beta_vec = torch.tensor([self.beta] * self.R).float()

    # ---- parameter construction (ref model_decompose_single.py:68-136) ------------------------
    def get_random(self, sizes):
        """ref model_decompose.py:189-199"""
        f = self.args.random_pad_func
        if f == 'uniform':
            return torch.rand(sizes)
        if f == 'normal':
            return torch.randn(sizes)
        a = torch.randn(sizes)
        torch.nn.init.xavier_normal_(a)
        return a

    def pad_additional_states(self, obj):
        """ref model_decompose.py:201-220: EVERY dimension equal to S grows by additional_states;
        new entries are rand * rand_constant (zeros for vectors)."""
        shape = tuple(obj.shape)
        padded = tuple(d if d != self.S else d + self.additional_states for d in shape)
        if len(shape) == 1:
            out = torch.zeros(padded)
        else:
            out = self.get_random(padded) * self.args.rand_constant
        out[tuple(slice(0, d) for d in shape)] = obj
        return out

    def _init_forward_parameters(self, S1, S2, V, C_o, W, W_o):
        a = self.args
        t = lambda x: torch.from_numpy(np.asarray(x)).float()      # noqa: E731
        self.S1 = self.pad_additional_states(t(S1))
        self.S2 = self.pad_additional_states(t(S2))
        self.V_embed = t(V)
        self.embed_r_generalized = torch.matmul(self.embedding.pinverse(), self.V_embed)   # D x R (:73-76)
        C_o = np.asarray(C_o)
        if a.use_crf == 1:       # two extra rows for START/STOP (:78-79)
            C_o = np.concatenate((C_o, self.get_random((2, self.S)).numpy() * a.rand_constant), axis=0)
        self.C_output_mat = self.pad_additional_states(t(C_o))
        self.wildcard_mat = self.pad_additional_states(t(W))
        self.wildcard_output_vector = self.pad_additional_states(t(W_o))
        Sp = self.S + self.additional_states
        if a.farnn in (1, 2):    # gate parameters (:93-123)
            self.Wss1 = torch.randn((Sp, Sp)).float()
            self.Wrs1 = torch.randn((self.R, Sp)).float()
            self.bs1 = torch.ones((1, Sp)).float() * a.bias_init
            if a.farnn == 2:
                self.Wss2 = torch.randn((Sp, Sp)).float()
                self.Wrs2 = torch.randn((self.R, Sp)).float()
                self.bs2 = torch.ones((1, Sp)).float() * a.bias_init
            if a.xavier:
                for name in _GATE_KEYS:
                    if hasattr(self, name) and not name.startswith('bs'):
                        torch.nn.init.xavier_normal_(getattr(self, name))
                if a.farnn == 1:
                    torch.nn.init.xavier_normal_(self.bs1)
        if self.random:          # (:125-136)
            for name in ('S1', 'S2', 'V_embed', 'C_output_mat', 'embed_r_generalized', 'wildcard_mat'):
                torch.nn.init.xavier_normal_(getattr(self, name))
            torch.nn.init.normal_(self.h0)
            torch.nn.init.normal_(self.hT)

    # ---- state dict compatible with the reference's key names ---------------------------------
    def state_dict(self):
        sd = {k: getattr(self, k) for k in self._param_keys if hasattr(self, k)}
        sd['embedding.weight'] = self.embedding
        sd['priority_layer.priority_mat'] = torch.from_numpy(self.priority_full)
        if self.use_crf:
            sd['crf.transitions'] = self.crf_transitions
        return sd

    def load_state_dict(self, sd, strict=False):
        for k, v in sd.items():
            v = torch.as_tensor(np.asarray(v)).float() if not torch.is_tensor(v) else v.detach().float().cpu()
            if k in self._param_keys:
                setattr(self, k, v)
            elif k == 'embedding.weight':
                self.embedding = v
            elif k == 'priority_layer.priority_mat':
                self.priority_full = v.numpy()
            elif k == 'crf.transitions':
                self.crf_transitions = v
        self.invalidate()
        return self

    # ---- device handle ------------------------------------------------------------------------
    def generalized_vocab_table(self):
        """get_generalized_v_embed_vec for every word id at once (ref model_decompose.py:222-241)."""
        gen = torch.matmul(self.embedding, self.embed_r_generalized)
        nl = self.args.additional_nonlinear
        if nl == 'relu':
            gen = torch.relu(gen)
        elif nl == 'tanh':
            gen = torch.tanh(gen)
        elif nl == 'sigmoid':
            gen = torch.sigmoid(gen)
        elif nl == 'relutanh':
            gen = torch.tanh(torch.relu(gen))
        return self.V_embed * self.beta_vec + gen * (1 - self.beta_vec)

    def _build_handle(self):
        a = self.args
        if a.local_loss_func != 'CE1':
            raise NotImplementedError('only CE1 is reachable from main.py (:127)')
        gates = {k: getattr(self, k).reshape(-1) if k.startswith('bs') else getattr(self, k)
                 for k in _GATE_KEYS if hasattr(self, k)}
        gates = {k: v.numpy() for k, v in gates.items()}
        # the word table Vgen = V_embed * beta + nl_add(E @ G) * (1 - beta) is folded by the library on the device
        # (farnn_decomp_ifst_create_folded); generalized_vocab_table() remains as the host statement of it
        return _lib.create_decomp_ifst_folded(
            self.V_embed.numpy(), self.embedding.numpy(), self.embed_r_generalized.numpy(), self.beta_vec.numpy(),
            self.S1.numpy(), self.S2.numpy(),
            self.wildcard_mat.numpy(), self.C_output_mat.numpy(), self.h0.numpy(), self.hT.numpy(),
            add_nl=a.additional_nonlinear,
            P=self.priority_full if a.use_priority else None, farnn=a.farnn, gates=gates,
            sigmoid_exponent=a.sigmoid_exponent, nl=a.update_nonlinear,
            semiring=self._semiring(), threshold=a.threshold, o_idx=self.o_idx, use_crf=self.use_crf,
            crf_trans=None if self.crf_transitions is None else self.crf_transitions.numpy(),
            device=self.device_index)

    def forward_RE(self, input, label, lengths, train=False):
        raise NotImplementedError('forward_RE exists only on the onehot models (ref model_onehot.py:148)')

    # ---- training step (reference :207-304 with train=True + train_decompose.py:186-190) ----
    # which tensors get a gradient: the reference's requires_grad flags (model_decompose.py:53-63,105-132)
    _TRAIN_FLAGS = {'S1': None, 'S2': None, 'embed_r_generalized': None, 'V_embed': 'train_V_embed',
                    'C_output_mat': 'train_c_output', 'wildcard_mat': 'train_wildcard', 'h0': 'train_h0',
                    'hT': 'train_hT', 'beta_vec': 'train_beta', 'embedding.weight': 'train_word_embed'}

    def _check_trainable(self, re_tags):
        """Raises before any device work.  The KD / PR teacher terms (--marryup_type kd | pr) are opt-in
        for their first release: RE2NN_DECOMP_TEACHER_TRAIN=1, and under --train_mode max RE2NN_DECOMP_TEACHER_MAX_TRAIN=1 beside it."""
        a = self.args
        marryup = getattr(a, 'marryup_type', 'none')
        teacher = marryup in ('kd', 'pr')
        plain = re_tags is None and marryup in ('none', None)
        with_teacher = opted_in('DECOMP_TEACHER_TRAIN') and marryup in ('none', None, 'kd', 'pr')
        if a.farnn not in (0, 1, 2) or a.train_mode not in ('sum', 'max') or a.local_loss_func != 'CE1' \
                or not (plain or with_teacher):
            raise NotImplementedError('the HIP training step covers the sum and max semirings and the CE1 loss (with or '
                                      'without the CRF), no KD/PR teachers (DESIGN.md, row f3)')
        if teacher and re_tags is None:
            raise ValueError('--marryup_type {} needs the RE teacher\'s scores: forward_local(..., re_tags=...)'.format(marryup))
        if re_tags is not None and not teacher:
            raise ValueError('re_tags were given but --marryup_type is {!r}: the teacher term would be dropped silently'.format(marryup))
        if teacher and a.train_mode == 'max' and not opted_in('DECOMP_TEACHER_MAX_TRAIN'):
            raise NotImplementedError('the KD / PR teacher terms are built for the sum semiring only; --train_mode max walks the '
                                      'valid positions only (DESIGN.md, row f3)')
        return teacher

    # PR's pi = max(c2_kdpr, c3_pr ** t) (ref :299).  The reference sets t = 1 in the constructor (model_decompose.py:42) and
    # the decomposed models never advance it, so the exponent stays 1 here as well.
    t = 1

    def _teacher(self, re_tags, Lmax):
        """(scores [B, Lmax, K], mode, c1, pi) of the teacher step: the zero columns of ref :213-218 (one without the CRF,
        three with it), the cut to Lmax of :292-298, and the weight of the original loss."""
        a = self.args
        B, L, _ = re_tags.shape
        re = torch.cat([re_tags.float(), torch.zeros(B, L, 3 if self.use_crf else 1, dtype=torch.float32, device=re_tags.device)],
                       dim=2)[:, :Lmax]
        pi = float(a.c2_kdpr) if a.marryup_type == 'kd' else max(float(a.c2_kdpr), float(a.c3_pr) ** self.t)
        return re, a.marryup_type, float(a.c1_kdpr), pi

    def _train_decl(self):
        """_TRAIN_FLAGS, then the gates of --farnn 1 / 2 and the CRF's transitions: nn.Parameters of the reference, always trainable
        (baselines/crf.py:46)."""
        extra = _GATE_KEYS[:3 * int(self.args.farnn)] + (('crf.transitions',) if self.use_crf else ())
        return super()._train_decl() + [(k, True) for k in extra]

    def _train_context(self):
        tp, a = self._tp, self.args
        S, R = tp['S1'].shape
        return _lib.TrainContext(tp['V_embed'].shape[0], S, R, tp['C_output_mat'].shape[0], nl=a.update_nonlinear,
                                 threshold=a.threshold, o_idx=self.o_idx, device=self.device_index, use_crf=self.use_crf,
                                 farnn=int(a.farnn), sigmoid_exponent=float(a.sigmoid_exponent), semiring=self._semiring(),
                                 teacher_max=opted_in('DECOMP_TEACHER_MAX_TRAIN'))

    def _copy_back(self, tp):
        for k, t in tp.items():
            setattr(self, {'embedding.weight': 'embedding', 'crf.transitions': 'crf_transitions'}.get(k, k), t.detach().cpu())

    def _train_vgen(self):
        tp = self._tp
        gen = torch.matmul(tp['embedding.weight'], tp['embed_r_generalized'])
        nl = self.args.additional_nonlinear
        if nl == 'relu':
            gen = torch.relu(gen)
        elif nl == 'tanh':
            gen = torch.tanh(gen)
        elif nl == 'sigmoid':
            gen = torch.sigmoid(gen)
        elif nl == 'relutanh':
            gen = torch.tanh(torch.relu(gen))
        return tp['V_embed'] * tp['beta_vec'] + gen * (1 - tp['beta_vec'])

    def _check_step(self, re_tags):
        self._check_trainable(re_tags)

    def _train_call(self, x, lengths, lab, ntok, re_tags):
        tp = self._tp                  # past _check_trainable, re_tags are given exactly under --marryup_type kd | pr
        return train_step.decomp_ifst_train_step(self._tc, self._train_vgen(), tp['S1'], tp['S2'], tp['wildcard_mat'],
                                                 tp['C_output_mat'], tp['h0'], tp['hT'], self._tpP, x, lengths, lab,
                                                 crf_trans=tp.get('crf.transitions'),
                                                 gates=tuple(tp[k] for k in _GATE_KEYS[:3 * int(self.args.farnn)]), valid_tokens=ntok,
                                                 teacher=None if re_tags is None else self._teacher(re_tags, x.shape[1]))


_SF_PARAM_KEYS = ('S1', 'S2', 'C_output_mat', 'wildcard_mat', 'wildcard_output_vector', 'h0', 'hT') + _GATE_KEYS


class FARNN_S_SF(Trainable, NativeTagger):
    """Host mirror of the reference's vector-input i-FST tagger ``FARNN_S_SF`` (model_decompose_single.py:307-579): the
    recurrence of FARNN_S_D_W_I_S on a dense input [B, L, R], one rule-space vector per token, in place of word ids and a word
    table.  Inference runs in the HIP library (farnn_decomp_sf_create / farnn_tag_vectors).  Training is
    one library call as well (farnn_decomp_sf_train_step): forward(..., train=True) returns a loss that autograd connects to
    the trainable weights AND to ``input``, so that whatever produced the vectors (an encoder, EmbedAggregator's bridge matrix)
    is fine-tuned through the automaton.  Scope: the sum semiring, farnn 0 / 1 / 2, CE1 or the CRF, the priority layer; no KD /
    PR teacher.  Opt-in for its first release: RE2NN_SF_TRAIN=1.  --train_mode max (ref :435-442) tags only
    (farnn_decomp_sf_max_create), under RE2NN_SF_MAX=1; its training is not built."""
    _param_keys = _SF_PARAM_KEYS
    # which tensors get a gradient: the reference's requires_grad flags (ref :343-346, :357-401)
    _TRAIN_FLAGS = {'S1': None, 'S2': None, 'C_output_mat': 'train_c_output', 'wildcard_mat': 'train_wildcard',
                    'h0': 'train_h0', 'hT': 'train_hT'}

    def _train_decl(self):
        """_TRAIN_FLAGS, then the gates of --farnn 1 / 2 and the CRF's transitions, always trainable (as FARNN_S_D_W_I_S's)."""
        extra = _GATE_KEYS[:3 * int(self.args.farnn)] + (('crf.transitions',) if self.use_crf else ())
        return Trainable._train_decl(self) + [(k, True) for k in extra]

    def _check_trainable(self):
        a = self.args
        if a.farnn not in (0, 1, 2) or a.train_mode != 'sum' or a.local_loss_func != 'CE1':
            raise NotImplementedError('FARNN_S_SF: the HIP training step covers the sum semiring and the CE1 loss (with or without '
                                      'the CRF) (DESIGN.md, row f14)')

    def _check_step(self, re_tags):
        if re_tags is not None or getattr(self.args, 'marryup_type', 'none') in ('kd', 'pr'):
            raise NotImplementedError('FARNN_S_SF: the KD / PR teacher terms (re_tags, --marryup_type kd | pr) are not built: their KL '
                                      'term reads the scores at the pad positions, that is the pad vectors (DESIGN.md, row f14)')

    def _train_context(self):
        tp, a = self._tp, self.args
        S, R = tp['S1'].shape
        return _lib.SfTrainContext(S, R, tp['C_output_mat'].shape[0], nl=a.update_nonlinear, threshold=a.threshold,
                                   o_idx=self.o_idx, device=self.device_index, use_crf=self.use_crf, farnn=int(a.farnn),
                                   sigmoid_exponent=float(a.sigmoid_exponent))

    def _copy_back(self, tp):
        for k, t in tp.items():
            setattr(self, {'crf.transitions': 'crf_transitions'}.get(k, k), t.detach().cpu())

    def _train_call(self, v, lengths, lab, ntok, re_tags):
        tp = self._tp
        if v.shape[2] != self.R:
            raise ValueError('FARNN_S_SF: input vectors have {} entries, the automaton\'s rank is {}'.format(v.shape[2], self.R))
        return train_step.decomp_sf_train_step(self._tc, v, tp['S1'], tp['S2'], tp['wildcard_mat'], tp['C_output_mat'], tp['h0'],
                                               tp['hT'], self._tpP, lengths, lab, crf_trans=tp.get('crf.transitions'),
                                               gates=tuple(tp[k] for k in _GATE_KEYS[:3 * int(self.args.farnn)]), valid_tokens=ntok)
    pad_additional_states = FARNN_S_D_W_I_S.pad_additional_states
    get_random = FARNN_S_D_W_I_S.get_random

    def state_dict(self):
        sd = {k: getattr(self, k) for k in self._param_keys if hasattr(self, k)}
        sd['priority_layer.priority_mat'] = torch.from_numpy(self.priority_full)
        if self.use_crf:
            sd['crf.transitions'] = self.crf_transitions
        return sd

    def load_state_dict(self, sd, strict=False):
        for k, v in sd.items():
            v = torch.as_tensor(np.asarray(v)).float() if not torch.is_tensor(v) else v.detach().float().cpu()
            if k in self._param_keys:
                setattr(self, k, v)
            elif k == 'priority_layer.priority_mat':
                self.priority_full = v.numpy()
            elif k == 'crf.transitions':
                self.crf_transitions = v
        self.invalidate()
        return self

    def __init__(self, S1=None, S2=None, C_output_mat=None, wildcard_mat=None, wildcard_output_vector=None,
                 final_vector=None, start_vector=None, priority_mat=None, args=None, o_idx=0, is_cuda=True):
        super().__init__(args, o_idx)
        a = args
        if a.train_mode == 'max' and not opted_in('SF_MAX'):
            raise NotImplementedError('FARNN_S_SF: --train_mode max needs an S x S block per token; the vector-input tagger exists '
                                      'in the sum semiring only (DESIGN.md, row f14)')
        t = lambda x: torch.from_numpy(np.asarray(x)).float()      # noqa: E731
        self.additional_states = int(a.additional_states)
        self.C = C_output_mat.shape[0]
        self.S, self.R = S1.shape
        self.use_crf = bool(a.use_crf)
        self.crf_transitions = None
        if self.use_crf:
            self.crf_transitions = crf_default_transitions(self.C)
            self.C += 2
        self.priority_full = expand_priority(self.C, priority_mat)
        self.random = bool(a.random)
        self.h0 = self.pad_additional_states(t(start_vector))
        self.hT = self.pad_additional_states(t(final_vector))
        # init_forward_parameters (ref :355-415)
        self.S1 = self.pad_additional_states(t(S1))
        self.S2 = self.pad_additional_states(t(S2))
        C_o = np.asarray(C_output_mat)
        if a.use_crf == 1:
            C_o = np.concatenate((C_o, self.get_random((2, self.S)).numpy() * a.rand_constant), axis=0)
        self.C_output_mat = self.pad_additional_states(t(C_o))
        self.wildcard_mat = self.pad_additional_states(t(wildcard_mat))
        self.wildcard_output_vector = self.pad_additional_states(t(wildcard_output_vector))
        Sp = self.S + self.additional_states
        if a.farnn in (1, 2):
            self.Wss1 = torch.randn((Sp, Sp)).float()
            self.Wrs1 = torch.randn((self.R, Sp)).float()
            self.bs1 = torch.ones((1, Sp)).float() * a.bias_init
            if a.farnn == 2:
                self.Wss2 = torch.randn((Sp, Sp)).float()
                self.Wrs2 = torch.randn((self.R, Sp)).float()
                self.bs2 = torch.ones((1, Sp)).float() * a.bias_init
            if a.xavier:
                for name in _GATE_KEYS:
                    if hasattr(self, name) and not name.startswith('bs'):
                        torch.nn.init.xavier_normal_(getattr(self, name))
                if a.farnn == 1:
                    torch.nn.init.xavier_normal_(self.bs1)
        if self.random:
            for name in ('S1', 'S2', 'C_output_mat', 'wildcard_mat'):
                torch.nn.init.xavier_normal_(getattr(self, name))
            torch.nn.init.normal_(self.h0)
            torch.nn.init.normal_(self.hT)

    def _build_handle(self):
        a = self.args
        if a.local_loss_func != 'CE1':
            raise NotImplementedError('only CE1 is reachable from main.py (:127)')
        gates = {k: (getattr(self, k).reshape(-1) if k.startswith('bs') else getattr(self, k)).numpy()
                 for k in _GATE_KEYS if hasattr(self, k)}
        kw = dict(P=self.priority_full if a.use_priority else None, farnn=a.farnn, gates=gates,
                  sigmoid_exponent=a.sigmoid_exponent, nl=a.update_nonlinear, threshold=a.threshold,
                  o_idx=self.o_idx, use_crf=self.use_crf,
                  crf_trans=None if self.crf_transitions is None else self.crf_transitions.numpy(), device=self.device_index)
        w = (self.S1.numpy(), self.S2.numpy(), self.wildcard_mat.numpy(), self.C_output_mat.numpy(), self.h0.numpy(), self.hT.numpy())
        if a.train_mode == 'max':      # (constructed under RE2NN_SF_MAX=1 only)
            return _lib.create_decomp_sf_max(*w, **kw)
        return _lib.create_decomp_sf(*w, semiring='sum', **kw)

    def run_vectors(self, input, lengths, want_tags=False, want_flat=False, want_scores=False):
        """One farnn_tag_vectors() call on input[:, :lengths.max()] (ref :497: L = lengths.max()).  A view that is not
        contiguous, not float32 or not on the device is copied on the host side, like the id mirrors' inputs."""
        dev = self._dev()
        h = self.handle
        L = int(lengths.max().item())
        v = input[:, :L].to(device=dev, dtype=torch.float32).contiguous()
        ln = lengths.to(device=dev, dtype=torch.int64).contiguous()
        B, _, R = v.shape
        if R != self.R:
            raise ValueError('FARNN_S_SF: input vectors have {} entries, the automaton\'s rank is {}'.format(R, self.R))
        tags = torch.empty((B, L), dtype=torch.int32, device=dev) if want_tags else None
        flat = torch.empty((int(ln.clamp(0, L).sum().item()),), dtype=torch.int64, device=dev) if want_flat else None
        scores = torch.empty((B, L, h.num_columns()), dtype=torch.float32, device=dev) if want_scores else None
        with torch.cuda.device(dev):
            h.tag_vectors(v.data_ptr(), ln.data_ptr(), B, L, _lib.MODE_LOCAL,
                          None if tags is None else tags.data_ptr(), None if flat is None else flat.data_ptr(),
                          None if scores is None else scores.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        return {'tags': tags, 'flat': flat, 'scores': scores, '_keep': (v, ln)}

    def forward(self, input, label, lengths, train=False, re_tags=None):
        """(loss, flat_pred, flat_true) of ref :483-579; the loss is None with train=False.  train=True (under RE2NN_SF_TRAIN=1):
        the loss carries a gradient towards ``input`` and the trainable weights (parameters())."""
        if train:
            if self.args.train_mode == 'max':
                raise NotImplementedError('FARNN_S_SF: --train_mode max is built for tagging only; its training step needs dM per '
                                          'token and is not built (DESIGN.md, row f14); call forward(..., train=False)')
            if not opted_in('SF_TRAIN'):
                raise NotImplementedError('FARNN_S_SF: training needs d loss / d input for the encoder in front of it and is not '
                                          'built (DESIGN.md, row f14); call forward(..., train=False)')
            self._check_step(re_tags)
            return Trainable.forward_local(self, input, label, lengths, train=True, re_tags=re_tags)
        self.sync_from_training()
        r = self.run_vectors(input, lengths, want_flat=True)
        return None, r['flat'].to(label.device), self._flatten(label, lengths)

    __call__ = forward
    forward_local = forward

    def forward_score(self, *a, **k):
        raise NotImplementedError('forward_score exists only on the onehot models (ref model_onehot.py:351)')

    def forward_RE(self, *a, **k):
        raise NotImplementedError('forward_RE exists only on the onehot models (ref model_onehot.py:148)')

    def submit_local(self, *a, **k):
        raise NotImplementedError('FARNN_S_SF takes vectors: the host-buffer path (word ids) does not apply')


class FARNN_S_bert:
    """``FARNN_S_bert`` of the reference (model_decompose_single_with_bert.py): EmbedAggregator in front of FARNN_S_SF.  The
    reference builds a BertModel inside; here ``encoder`` is ANY callable (bert_input, bert_attend_mask, bert_valid_mask,
    lengths) -> [B, L, D] contextual token vectors, D = static_embed.shape[1]."""

    def __init__(self, V=None, S1=None, S2=None, C_output_mat=None, wildcard_mat=None, wildcard_output_vector=None,
                 final_vector=None, start_vector=None, static_embed=None, priority_mat=None, args=None, o_idx=0,
                 is_cuda=True, encoder=None):
        from .embed_aggregator import EmbedAggregator
        self.embed = EmbedAggregator(args, V, static_embed, encoder=encoder)
        self.slot_filler = FARNN_S_SF(S1=S1, S2=S2, C_output_mat=C_output_mat, wildcard_mat=wildcard_mat,
                                      wildcard_output_vector=wildcard_output_vector, final_vector=final_vector,
                                      start_vector=start_vector, priority_mat=priority_mat, args=args, o_idx=o_idx,
                                      is_cuda=is_cuda)

    def parameters(self):
        """The aggregator's leaves (EmbedAggregator.requires_grad_()), a torch.nn.Module encoder's parameters, and the
        automaton's (after its first training step, or slot_filler.enable_training())."""
        return iter(list(self.embed.parameters()) + list(self.slot_filler.parameters()))

    def forward(self, input, bert_input, bert_attend_mask, bert_valid_mask, lengths, label, train=False, re_tags=None):
        """train=True (RE2NN_SF_TRAIN=1): the loss's backward() reaches the aggregator's leaves and the
        encoder through d loss / d vecs."""
        vecs = self.embed.forward_bert(input, bert_input, bert_attend_mask, bert_valid_mask, lengths)
        return self.slot_filler(vecs, label, lengths, train=train, re_tags=re_tags)

    __call__ = forward
