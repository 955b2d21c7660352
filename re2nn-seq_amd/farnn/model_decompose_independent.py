"""Host mirror of the reference's decomposed independent=1 tagger ``FARNN_S_D_W_I``
(src_seq/farnn/model_decompose_independent.py:11-300): a rank-R language tensor plus a separate
rank-R_O output tensor (C_output, S1_output, S2_output).  Same constructor arguments and state-dict
keys as the reference; inference runs in the HIP library (farnn_decomp_ind1_create).
Training (opt-in, RE2NN_DECOMP_IND1_TRAIN=1): farnn_decomp_ind1_train_step; with --use_crf 1
(RE2NN_DECOMP_IND1_CRF_TRAIN=1 beside it): farnn_decomp_ind1_crf_train_step; with --farnn 1 | 2
(RE2NN_DECOMP_IND1_GATED_TRAIN=1 beside it, sum semiring): farnn_decomp_ind1_gated_train_step, with or without the CRF; with
--farnn 1 | 2 --train_mode max (RE2NN_DECOMP_IND1_GATED_MAX_TRAIN=1 beside that and RE2NN_BUCKETED_MAX_TRAIN=1):
farnn_decomp_ind1_gated_max_train_step.
"""
import numpy as np
import torch

from .. import _lib
from .model_decompose_single import FARNN_S_D_W_I_S, crf_default_transitions, _GATE_KEYS
from . import train_step
from ._native import NativeTagger, bucketed_max_train_enabled, opted_in
from .priority import expand_priority

_PARAM_KEYS = ('S1', 'S2', 'V_embed', 'embed_r_generalized', 'C_output', 'S1_output', 'S2_output',
               'wildcard_mat', 'wildcard_output', 'h0', 'hT', 'beta_vec') + _GATE_KEYS


class FARNN_S_D_W_I(FARNN_S_D_W_I_S):
    _param_keys = _PARAM_KEYS

    def __init__(self, V=None, S1=None, S2=None, C_output=None, S1_output=None, S2_output=None,
                 wildcard_mat=None, wildcard_output=None, final_vector=None, start_vector=None,
                 pretrained_word_embed=None, priority_mat=None, args=None, o_idx=0, is_cuda=True):
        NativeTagger.__init__(self, args, o_idx)
        self.additional_states = int(args.additional_states)
        self.embedding = torch.from_numpy(np.asarray(pretrained_word_embed)).float()       # V x D
        self.C, self.R_O = C_output.shape                                                  # (:39)
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
        self._init_forward_parameters_ind1(S1, S2, V, S1_output, S2_output, C_output, wildcard_mat,
                                           wildcard_output)
        self.beta = args.beta
        self.beta_vec = torch.tensor([self.beta] * self.R).float()

    # ---- parameter construction (ref model_decompose_independent.py:68-146) ---------------------
    def _init_forward_parameters_ind1(self, S1, S2, V, S1_o, S2_o, C_o, W, W_o):
        a = self.args
        t = lambda x: torch.from_numpy(np.asarray(x)).float()      # noqa: E731
        self.S1 = self.pad_additional_states(t(S1))
        self.S2 = self.pad_additional_states(t(S2))
        self.V_embed = t(V)
        self.embed_r_generalized = torch.matmul(self.embedding.pinverse(), self.V_embed)   # D x R (:72-75)
        C_o = np.asarray(C_o)
        if a.use_crf:            # two extra rows for START/STOP (:77-79)
            C_o = np.concatenate((C_o, self.get_random((2, self.R_O)).numpy() * a.rand_constant), axis=0)
        self.C_output = self.pad_additional_states(t(C_o))
        self.S1_output = self.pad_additional_states(t(S1_o))
        self.S2_output = self.pad_additional_states(t(S2_o))
        self.wildcard_mat = self.pad_additional_states(t(W))
        if W_o is not None:
            self.wildcard_output = self.pad_additional_states(t(W_o))
        Sp = self.S + self.additional_states
        if a.farnn in (1, 2):    # gate parameters (:99-130)
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
        if self.random:          # (:132-146)
            for name in ('S1', 'S2', 'V_embed', 'S1_output', 'S2_output', 'C_output',
                         'embed_r_generalized', 'wildcard_mat'):
                torch.nn.init.xavier_normal_(getattr(self, name))
            torch.nn.init.normal_(self.h0)
            torch.nn.init.normal_(self.hT)

    # ---- device handle ------------------------------------------------------------------------
    def _build_handle(self):
        a = self.args
        gates = {k: getattr(self, k).reshape(-1) if k.startswith('bs') else getattr(self, k)
                 for k in _GATE_KEYS if hasattr(self, k)}
        gates = {k: v.numpy() for k, v in gates.items()}
        Wo = None                      # CE1 drops wildcard_output from the output sum (:213-216)
        if a.local_loss_func != 'CE1' and getattr(self, 'wildcard_output', None) is not None:
            Wo = self.wildcard_output.numpy()
        return _lib.create_decomp_ind1(
            self.generalized_vocab_table().numpy(), self.S1.numpy(), self.S2.numpy(),
            self.wildcard_mat.numpy(), self.C_output.numpy(), self.S1_output.numpy(),
            self.S2_output.numpy(), self.h0.numpy(), self.hT.numpy(), Wo=Wo,
            P=self.priority_full if a.use_priority else None, farnn=a.farnn, gates=gates,
            sigmoid_exponent=a.sigmoid_exponent, nl=a.update_nonlinear,
            semiring=self._semiring(), threshold=a.threshold, o_idx=self.o_idx, use_crf=self.use_crf,
            crf_trans=None if self.crf_transitions is None else self.crf_transitions.numpy(),
            device=self.device_index)

    # ---- training step (reference :148-300 with train=True + train_decompose.py:161-221) ----
    # which tensors get a gradient: the reference's requires_grad flags (:52-55, :70-97).  wildcard_output is not read under
    # CE1 (:213-216): it has no gradient, is not a parameter here and stays as it is in the state dict.
    _TRAIN_FLAGS = {'S1': None, 'S2': None, 'embed_r_generalized': None, 'V_embed': 'train_V_embed',
                    'C_output': 'train_wildcard', 'S1_output': 'train_wildcard', 'S2_output': 'train_wildcard',
                    'wildcard_mat': 'train_wildcard_wildcard', 'h0': 'train_h0', 'hT': 'train_hT',
                    'beta_vec': 'train_beta', 'embedding.weight': 'train_word_embed'}

    _check_needs_re_tags = False     # every refusal but the teacher's is known without a batch

    def _check_trainable(self, re_tags=None):
        """The cases the HIP training step does not cover, refused before any device work."""
        if not opted_in('DECOMP_IND1_TRAIN'):          # before self.args is touched: the refusal needs the type only
            from ..train_onehot import no_training_step
            raise no_training_step(self)
        a = self.args
        why = None
        gated = a.farnn != 0
        if gated and not (a.farnn in (1, 2) and opted_in('DECOMP_IND1_GATED_TRAIN')):
            why = 'the gated recurrences (--farnn {})'.format(a.farnn)
        elif a.train_mode != 'sum' and not (a.train_mode == 'max' and bucketed_max_train_enabled() and
                                            (not gated or opted_in('DECOMP_IND1_GATED_MAX_TRAIN'))):
            why = 'the max semiring (--train_mode {})'.format(a.train_mode)      # (the gated chains: behind a switch of their own)
        elif a.use_crf and not opted_in('DECOMP_IND1_CRF_TRAIN'):
            why = 'the CRF (--use_crf 1)'
        elif a.local_loss_func != 'CE1':
            why = 'a loss other than CE1 (--local_loss_func {})'.format(a.local_loss_func)
        elif re_tags is not None or getattr(a, 'marryup_type', 'none') not in ('none', None):
            why = 'the KD / PR teacher terms (--marryup_type {})'.format(getattr(a, 'marryup_type', 'none'))
        else:
            from ..dist import world
            if world()[1] > 1:
                why = 'multi-GPU data-parallel training'
        if why is not None:
            raise NotImplementedError('training the decomposed independent=1 model covers farnn 0, the sum semiring and the CE1 '
                                      'loss on one GPU; {} is not built (DESIGN.md, row f9)'.format(why))

    def _train_context(self):
        tp = self._tp
        S, R = tp['S1'].shape
        C, RO = tp['C_output'].shape
        return _lib.Decomp1TrainContext(tp['V_embed'].shape[0], S, R, RO, C, nl=self.args.update_nonlinear,
                                        threshold=self.args.threshold, o_idx=self.o_idx, device=self.device_index,
                                        semiring=self._semiring())

    # (the gates of --farnn 1 | 2 -- Wss1, Wrs1, bs1, then Wss2, Wrs2, bs2 -- and crf.transitions follow _TRAIN_FLAGS in
    #  FARNN_S_D_W_I_S._train_decl: always trainable, present only for the model's farnn; _copy_back writes them back by name)
    def _train_call(self, x, lengths, lab, ntok, re_tags):
        tp = self._tp
        farnn = int(self.args.farnn)
        return train_step.decomp_ind1_train_step(self._tc, self._train_vgen(), tp['S1'], tp['S2'], tp['wildcard_mat'],
                                                 tp['C_output'], tp['S1_output'], tp['S2_output'], tp['h0'], tp['hT'], self._tpP,
                                                 x, lengths, lab, valid_tokens=ntok, crf_trans=tp.get('crf.transitions'),
                                                 gates=tuple(tp[k] for k in _GATE_KEYS[:3 * farnn]),
                                                 sigmoid_exponent=float(self.args.sigmoid_exponent))
