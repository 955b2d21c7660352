"""Host mirrors of the reference's onehot FA-RNN taggers (src_seq/farnn/model_onehot.py).

Same class names, constructor arguments and inference methods as the reference, so
``train_onehot.py``-style drivers construct and call them unchanged; all arithmetic runs in the
HIP library through the C-ABI (include/farnn.h).

  FARNN_S_O      FST, 4-D tensor          (--independent 0)   ref :8-181
  FARNN_S_O_I    two 3-D tensors          (--independent 1)   ref :184-306
  FARNN_S_O_I_S  i-FST, T[V,S,S] + O[C,S] (--independent 2)   ref :310-428
"""
import numpy as np
import torch

from .. import _lib
from . import train_step
from ._native import NativeTagger, bucketed_max_train_enabled, opted_in
from ._trainable import Trainable
from .priority import expand_priority


def _noisy(arr, amp):
    """reference utils.add_random_noise (:273-274) applied after the float32 cast."""
    t = torch.from_numpy(np.asarray(arr)).float()
    if amp:
        t = t + torch.rand_like(t) * amp
    return t.numpy()


class _OnehotBase(NativeTagger):
    def __init__(self, args, o_idx, n_labels, priority_mat, is_cuda=False):
        super().__init__(args, o_idx)
        if args.local_loss_func not in ('CE', 'CE1'):
            raise NotImplementedError()            # ref :63-64
        self.C = int(n_labels)
        self.amp = args.rand_constant
        self.priority_full = expand_priority(self.C, priority_mat)

    def _P(self):
        return self.priority_full if self.args.use_priority else None


class FARNN_S_O_I_S(Trainable, _OnehotBase):
    def __init__(self, language_tensor=None, output_mat=None, wildcard_mat=None,
                 output_wildcard_vector=None, final_vector=None, start_vector=None, priority_mat=None,
                 args=None, o_idx=0, is_cuda=False):
        C, S = output_mat.shape
        super().__init__(args, o_idx, C, priority_mat, is_cuda)
        self.S = S
        # same order of (possibly noisy) casts as the reference constructor (:322-336)
        self.h0 = _noisy(start_vector, self.amp)
        self.hT = _noisy(final_vector, self.amp)
        self.language_tensor = _noisy(language_tensor, self.amp)
        self.wildcard_mat = _noisy(wildcard_mat, self.amp)
        self.output_mat = _lib.f32(output_mat)
        self.output_wildcard_vector = _lib.f32(output_wildcard_vector)
        self.use_crf = False          # the reference's onehot models never read use_crf
        self.crf_transitions = None

    @classmethod
    def from_automaton(cls, automata, word2idx, slot2idx, priority_mat=None, args=None, o_idx=0,
                       dataset='MITR-BIO'):
        """The same tagger built WITHOUT the dense host tensors: the automaton's edges go
        to the device as int32 lists and are scattered in HBM (farnn_onehot_ifst_create_from_edges).
        Only for rand_constant == 0 (the noise of utils.add_random_noise is dense by nature)."""
        from ..wfa.fsa_to_tensor import dfa_to_edges_slot_single_wildcard
        if args.rand_constant:
            raise ValueError('from_automaton needs rand_constant == 0')
        word, frm, to, label, fin, sta, _ = dfa_to_edges_slot_single_wildcard(automata, word2idx, slot2idx, dataset)
        self = cls.__new__(cls)
        C, S = len(slot2idx) + 1, len(automata['states'])
        _OnehotBase.__init__(self, args, o_idx, C, priority_mat, False)
        self.S, self.V = S, len(word2idx)
        self.h0, self.hT = _noisy(sta, 0), _noisy(fin, 0)
        self.edges = (word, frm, to, label)
        self.use_crf = False
        self.crf_transitions = None
        return self

    def _dense(self):
        """language_tensor / wildcard_mat / output_mat of an edge-built model, on demand (state_dict)."""
        word, frm, to, label = self.edges
        C = self.C
        T = np.zeros((self.V, self.S, self.S), np.float32)
        W = np.zeros((self.S, self.S), np.float32)
        O = np.zeros((C, self.S), np.float32)
        lang = word >= 0
        T[word[lang], frm[lang], to[lang]] = 1
        wild = word == -1
        W[frm[wild], to[wild]] = 1
        O[label, to] = 1
        return T, W, O

    def enable_crf(self, transitions=None):
        """BASELINE config 4 (onehot + fused Viterbi): the composition SURVEY.md 8a-note defines --
        scores + two zero columns -> clamp column C'-3 -> CRF._viterbi_decode -> C'-3 -> o_idx."""
        self.use_crf = True
        self.crf_transitions = None if transitions is None else _lib.f32(transitions)
        self.invalidate()
        return self

    def _build_handle(self):
        a = self.args
        if a.local_loss_func != 'CE1':
            raise NotImplementedError('only CE1 is reachable from main.py (:127)')
        kw = dict(P=self._P(), nl=a.update_nonlinear, semiring=self._semiring(), threshold=a.threshold, o_idx=self.o_idx,
                  use_crf=self.use_crf, crf_trans=self.crf_transitions, device=self.device_index)
        if getattr(self, 'edges', None) is not None:
            word, frm, to, label = self.edges
            return _lib.create_onehot_ifst_from_edges(self.V, self.S, self.C, word, frm, to, label,
                                                      self.h0, self.hT, **kw)
        return _lib.create_onehot_ifst(self.language_tensor, self.wildcard_mat, self.output_mat, self.h0,
                                       self.hT, **kw)

    # ---- training step (reference :351-428 with train=True + train_onehot.py:156-206) ----
    def _check_trainable(self):
        """The cases the HIP training step does not cover, refused before any device work."""
        a = self.args
        if a.train_mode != 'sum' and not (a.train_mode == 'max' and opted_in('ONEHOT_MAX_TRAIN')):
            raise NotImplementedError('training the onehot i-FST covers the sum semiring only by default; --train_mode max '
                                      'is opt-in (set RE2NN_ONEHOT_MAX_TRAIN=1), --train_mode {} was asked for '
                                      '(DESIGN.md, row f5)'.format(a.train_mode))
        if a.local_loss_func != 'CE1':
            raise NotImplementedError('training the onehot i-FST covers the CE1 loss only (main.py:127)')
        if self.use_crf:
            raise NotImplementedError('training the onehot i-FST with the CRF extension (enable_crf) is not built; the '
                                      "reference's onehot models never read use_crf (DESIGN.md, row f5)")
        from ..dist import world
        if world()[1] > 1:
            raise NotImplementedError('multi-GPU data-parallel training of the onehot i-FST is not built; train on one '
                                      'GPU (DESIGN.md, row f5)')

    _TRAIN_FLAGS = {'language_tensor': None, 'wildcard_mat': False, 'output_mat': False, 'h0': False, 'hT': False}   # ref :326-337

    def _train_context(self):
        V, S, _ = self._tp['language_tensor'].shape
        return _lib.OnehotTrainContext(V, S, self.C, nl=self.args.update_nonlinear, threshold=self.args.threshold,
                                       o_idx=self.o_idx, device=self.device_index, semiring=self._semiring())

    def _train_call(self, x, lengths, lab, ntok, re_tags):
        tp = self._tp
        return train_step.onehot_ifst_train_step(self._tc, tp['language_tensor'], tp['wildcard_mat'], tp['output_mat'],
                                                 tp['h0'], tp['hT'], self._tpP, x, lengths, lab, valid_tokens=ntok)

    def _copy_back(self, tp):
        """An edge-built model becomes a dense one (its edges no longer describe the weights)."""
        if getattr(self, 'edges', None) is not None:
            self.language_tensor, self.wildcard_mat, self.output_mat = self._dense()
            self.output_wildcard_vector = np.zeros(self.S, np.float32)
            self.edges = None
        self.language_tensor = tp['language_tensor'].detach().cpu().numpy()

    def state_dict(self):
        self.sync_from_training()
        if getattr(self, 'edges', None) is not None:
            T, W, O = self._dense()
            return {'h0': self.h0, 'hT': self.hT, 'language_tensor': T, 'wildcard_mat': W, 'output_mat': O,
                    'output_wildcard_vector': np.zeros(self.S, np.float32)}
        return {'h0': self.h0, 'hT': self.hT, 'language_tensor': self.language_tensor,
                'wildcard_mat': self.wildcard_mat, 'output_mat': self.output_mat,
                'output_wildcard_vector': self.output_wildcard_vector}


class FARNN_S_O(Trainable, _OnehotBase):
    def __init__(self, language_tensor=None, wildcard_tensor=None, wildcard_wildcard_mat=None,
                 final_vector=None, start_vector=None, priority_mat=None, args=None, o_idx=0,
                 is_cuda=False):
        C, S, _ = wildcard_tensor.shape
        super().__init__(args, o_idx, C, priority_mat, is_cuda)
        self.S = S
        self.h0 = _noisy(start_vector, self.amp)
        self.hT = _noisy(final_vector, self.amp)
        self.language_tensor = _noisy(language_tensor, self.amp)
        self.wildcard_tensor = _noisy(wildcard_tensor, self.amp)
        self.wildcard_wildcard_mat = _lib.f32(wildcard_wildcard_mat)

    @classmethod
    def from_automaton(cls, automata, word2idx, slot2idx, priority_mat=None, args=None, o_idx=0,
                       dataset='MITR-BIO'):
        """Built without the dense [V,C,S,S] host tensor (2.5 GB at ATIS size): see FARNN_S_O_I_S.from_automaton."""
        from ..wfa.fsa_to_tensor import dfa_to_edges_slot_new_wildcard
        if args.rand_constant:
            raise ValueError('from_automaton needs rand_constant == 0')
        word, frm, to, label, fin, sta, _ = dfa_to_edges_slot_new_wildcard(automata, word2idx, slot2idx, dataset)
        self = cls.__new__(cls)
        _OnehotBase.__init__(self, args, o_idx, len(slot2idx) + 1, priority_mat, False)
        self.S, self.V = len(automata['states']), len(word2idx)
        self.h0, self.hT = _noisy(sta, 0), _noisy(fin, 0)
        self.edges = (word, frm, to, label)
        return self

    def _build_handle(self):
        a = self.args
        if a.local_loss_func != 'CE1':
            raise NotImplementedError('only CE1 is reachable from main.py (:127)')
        if getattr(self, 'edges', None) is not None:
            word, frm, to, label = self.edges
            return _lib.create_onehot_fst4_from_edges(
                self.V, self.S, self.C, word, frm, to, label, self.h0, self.hT, P=self._P(),
                semiring=self._semiring(), threshold=a.threshold, o_idx=self.o_idx, device=self.device_index)
        return _lib.create_onehot_fst4(
            self.language_tensor, self.wildcard_tensor, self.h0, self.hT, P=self._P(),
            semiring=self._semiring(), threshold=a.threshold, o_idx=self.o_idx, device=self.device_index)

    def _dense(self):
        """language_tensor / wildcard_tensor of an edge-built model, on demand (enable_training, state_dict)."""
        word, frm, to, label = self.edges
        T = np.zeros((self.V, self.C, self.S, self.S), np.float32)
        W = np.zeros((self.C, self.S, self.S), np.float32)
        lang = word >= 0
        T[word[lang], label[lang], frm[lang], to[lang]] = 1
        wild = word == -1
        W[label[wild], frm[wild], to[wild]] = 1
        return T, W

    # ---- training step (reference :66-146 with train=True + train_onehot.py:156-206) ----
    def _check_trainable(self):
        """The cases the HIP training step does not cover, refused before any device work."""
        if not opted_in('ONEHOT_FST_TRAIN'):           # before self.args is touched: the refusal needs the type only
            from ..train_onehot import no_training_step
            raise no_training_step(self)              # today's refusal, word for word
        a = self.args
        if a.train_mode != 'sum' and not (a.train_mode == 'max' and bucketed_max_train_enabled()):
            raise NotImplementedError('training the onehot FST covers the sum semiring only, --train_mode {} was asked for '
                                      '(DESIGN.md, row f7)'.format(a.train_mode))
        if a.local_loss_func != 'CE1':
            raise NotImplementedError('training the onehot FST covers the CE1 loss only (main.py:127)')
        if getattr(a, 'train_wildcard_wildcard', 0):
            raise NotImplementedError('training the onehot FST with --train_wildcard_wildcard 1 is not built: '
                                      'wildcard_wildcard_mat is not read under CE1 and has no gradient (DESIGN.md, row f7)')
        from ..dist import world
        if world()[1] > 1:
            raise NotImplementedError('multi-GPU data-parallel training of the onehot FST is not built; train on one GPU '
                                      '(DESIGN.md, row f7)')

    _TRAIN_FLAGS = {'language_tensor': None, 'wildcard_tensor': 'train_wildcard', 'h0': False, 'hT': False}          # ref :32-37

    def _train_context(self):
        return _lib.Fst4TrainContext(self._tp['language_tensor'].shape[0], self.S, self.C, threshold=self.args.threshold,
                                     o_idx=self.o_idx, device=self.device_index, semiring=self._semiring())

    def _train_call(self, x, lengths, lab, ntok, re_tags):
        tp = self._tp
        return train_step.onehot_fst4_train_step(self._tc, tp['language_tensor'], tp['wildcard_tensor'], tp['h0'], tp['hT'],
                                                 self._tpP, x, lengths, lab, valid_tokens=ntok)

    def _copy_back(self, tp):
        """An edge-built model becomes a dense one."""
        if getattr(self, 'edges', None) is not None:
            self.wildcard_wildcard_mat = np.zeros((self.S, self.S), np.float32)
            self.edges = None
        self.language_tensor = tp['language_tensor'].detach().cpu().numpy()
        self.wildcard_tensor = tp['wildcard_tensor'].detach().cpu().numpy()

    def state_dict(self):
        self.sync_from_training()
        if getattr(self, 'edges', None) is not None:
            T, W = self._dense()
            return {'h0': self.h0, 'hT': self.hT, 'language_tensor': T, 'wildcard_tensor': W,
                    'wildcard_wildcard_mat': np.zeros((self.S, self.S), np.float32)}
        return {'h0': self.h0, 'hT': self.hT, 'language_tensor': self.language_tensor,
                'wildcard_tensor': self.wildcard_tensor,
                'wildcard_wildcard_mat': self.wildcard_wildcard_mat}


class FARNN_S_O_I(Trainable, _OnehotBase):
    def __init__(self, language_tensor=None, output_tensor=None, wildcard_mat=None,
                 output_wildcard_mat=None, final_vector=None, start_vector=None, priority_mat=None,
                 args=None, o_idx=0, is_cuda=False):
        C, S, _ = output_tensor.shape
        super().__init__(args, o_idx, C, priority_mat, is_cuda)
        self.S = S
        self.h0 = _noisy(start_vector, self.amp)
        self.hT = _noisy(final_vector, self.amp)
        self.language_tensor = _noisy(language_tensor, self.amp)
        self.wildcard_mat = _noisy(wildcard_mat, self.amp)
        self.output_tensor = _lib.f32(output_tensor)
        self.output_wildcard_mat = None if output_wildcard_mat is None else _lib.f32(output_wildcard_mat)

    @classmethod
    def from_automaton(cls, automata, word2idx, slot2idx, priority_mat=None, args=None, o_idx=0,
                       dataset='MITR-BIO'):
        """Built without the dense host tensors: see FARNN_S_O_I_S.from_automaton."""
        from ..wfa.fsa_to_tensor import dfa_to_edges_slot_independent_wildcard
        if args.rand_constant:
            raise ValueError('from_automaton needs rand_constant == 0')
        word, frm, to, label, fin, sta, _ = dfa_to_edges_slot_independent_wildcard(automata, word2idx, slot2idx,
                                                                                   dataset)
        self = cls.__new__(cls)
        _OnehotBase.__init__(self, args, o_idx, len(slot2idx) + 1, priority_mat, False)
        self.S, self.V = len(automata['states']), len(word2idx)
        self.h0, self.hT = _noisy(sta, 0), _noisy(fin, 0)
        self.edges = (word, frm, to, label)
        return self

    def _build_handle(self):
        a = self.args
        if a.local_loss_func != 'CE1':
            raise NotImplementedError('only CE1 is reachable from main.py (:127)')
        if getattr(self, 'edges', None) is not None:
            word, frm, to, label = self.edges
            return _lib.create_onehot_ind1_from_edges(
                self.V, self.S, self.C, word, frm, to, label, self.h0, self.hT, P=self._P(),
                semiring=self._semiring(), mask_by_output=(a.independent == 2),
                threshold=a.threshold, o_idx=self.o_idx, device=self.device_index)
        return _lib.create_onehot_ind1(
            self.language_tensor, self.wildcard_mat, self.output_tensor, self.h0, self.hT, P=self._P(),
            semiring=self._semiring(), mask_by_output=(a.independent == 2), threshold=a.threshold, o_idx=self.o_idx,
            device=self.device_index)

    def _dense(self):
        """language_tensor / wildcard_mat / output_tensor of an edge-built model, on demand (enable_training, state_dict):
        what the edge-built handle scatters.  A class edge with no member in the vocabulary (word -2) keeps its label in
        output_tensor and writes nothing into language_tensor."""
        word, frm, to, label = self.edges
        T = np.zeros((self.V, self.S, self.S), np.float32)
        W = np.zeros((self.S, self.S), np.float32)
        O = np.zeros((self.C, self.S, self.S), np.float32)
        lang = word >= 0
        T[word[lang], frm[lang], to[lang]] = 1
        wild = word == -1
        W[frm[wild], to[wild]] = 1
        has = label >= 0
        O[label[has], frm[has], to[has]] = 1
        return T, W, O

    # ---- training step (reference :229-306 with train=True + train_onehot.py:156-206) ----
    def _check_trainable(self):
        """The cases the HIP training step does not cover, refused before any device work."""
        if not opted_in('ONEHOT_IND1_TRAIN'):          # before self.args is touched: the refusal needs the type only
            from ..train_onehot import no_training_step
            raise no_training_step(self)              # today's refusal, word for word
        a = self.args
        if a.train_mode != 'sum' and not (a.train_mode == 'max' and bucketed_max_train_enabled()):
            raise NotImplementedError('training the onehot independent=1 model covers the sum semiring only, --train_mode {} '
                                      'was asked for (DESIGN.md, row f8)'.format(a.train_mode))
        if a.local_loss_func != 'CE1':
            raise NotImplementedError('training the onehot independent=1 model covers the CE1 loss only (main.py:127)')
        from ..dist import world
        if world()[1] > 1:
            raise NotImplementedError('multi-GPU data-parallel training of the onehot independent=1 model is not built; '
                                      'train on one GPU (DESIGN.md, row f8)')

    _TRAIN_FLAGS = {'language_tensor': None, 'wildcard_mat': False, 'output_tensor': False, 'h0': False, 'hT': False}   # ref :209-223

    def _train_context(self):
        return _lib.Ind1TrainContext(self._tp['language_tensor'].shape[0], self.S, self.C,
                                     mask_by_output=(self.args.independent == 2), threshold=self.args.threshold,
                                     o_idx=self.o_idx, device=self.device_index, semiring=self._semiring())

    def _train_call(self, x, lengths, lab, ntok, re_tags):
        tp = self._tp
        return train_step.onehot_ind1_train_step(self._tc, tp['language_tensor'], tp['wildcard_mat'], tp['output_tensor'],
                                                 tp['h0'], tp['hT'], self._tpP, x, lengths, lab, valid_tokens=ntok)

    def _copy_back(self, tp):
        """An edge-built model becomes a dense one (its edges no longer describe the weights)."""
        if getattr(self, 'edges', None) is not None:
            self.language_tensor, self.wildcard_mat, self.output_tensor = self._dense()
            self.output_wildcard_mat = None
            self.edges = None
        self.language_tensor = tp['language_tensor'].detach().cpu().numpy()

    def state_dict(self):
        self.sync_from_training()
        if getattr(self, 'edges', None) is not None:
            T, W, O = self._dense()
            return {'h0': self.h0, 'hT': self.hT, 'language_tensor': T, 'wildcard_mat': W, 'output_tensor': O}
        return {'h0': self.h0, 'hT': self.hT, 'language_tensor': self.language_tensor,
                'wildcard_mat': self.wildcard_mat, 'output_tensor': self.output_tensor}
