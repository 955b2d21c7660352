"""Host mirrors of the reference's onehot FA-RNN taggers (src_seq/farnn/model_onehot.py).

Same class names, constructor arguments and inference methods as the reference, so
``train_onehot.py``-style drivers construct and call them unchanged; all arithmetic runs in the
HIP library through the C-ABI (include/farnn.h).

  FARNN_S_O      FST, 4-D tensor          (--independent 0)   ref :8-181
  FARNN_S_O_I    two 3-D tensors          (--independent 1)   ref :184-306
  FARNN_S_O_I_S  i-FST, T[V,S,S] + O[C,S] (--independent 2)   ref :310-428
"""
import os

import numpy as np
import torch

from .. import _lib
from ._native import NativeTagger, bucketed_max_train_enabled
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


class FARNN_S_O_I_S(_OnehotBase):
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
        kw = dict(P=self._P(), nl=a.update_nonlinear, semiring='max' if a.train_mode == 'max' else 'sum',
                  threshold=a.threshold, o_idx=self.o_idx, use_crf=self.use_crf,
                  crf_trans=self.crf_transitions, device=self.device_index)
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
        if a.train_mode != 'sum' and not (a.train_mode == 'max' and self._max_train_enabled()):
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

    @staticmethod
    def _max_train_enabled():
        """RE2NN_ONEHOT_MAX_TRAIN=1: the max-semiring training step (opt-in for its first release, as RE2NN_NATIVE_OPTIM)"""
        return os.environ.get('RE2NN_ONEHOT_MAX_TRAIN', '') == '1'

    def enable_training(self):
        """Device-resident tensors (language_tensor the only one with requires_grad, as in the reference :326-337) and
        the library context.  An edge-built model gets its dense tensors here (_dense())."""
        self._check_trainable()
        if getattr(self, '_tp', None) is not None:
            return self
        if not torch.cuda.is_available():
            raise _lib.FarnnError('no MI355X visible; the training step has no CPU fallback')
        dev = self._dev()
        sd = self.state_dict()
        self._tp = {}
        for k in ('language_tensor', 'wildcard_mat', 'output_mat', 'h0', 'hT'):
            t = torch.from_numpy(np.ascontiguousarray(sd[k], dtype=np.float32)).to(dev).clone()
            self._tp[k] = t.requires_grad_(k == 'language_tensor')
        self._tpP = torch.from_numpy(np.ascontiguousarray(self.priority_full, dtype=np.float32)).to(dev) \
            if self.args.use_priority else None
        V, S, _ = self._tp['language_tensor'].shape
        self._tc = _lib.OnehotTrainContext(V, S, self.C, nl=self.args.update_nonlinear, threshold=self.args.threshold,
                                           o_idx=self.o_idx, device=self.device_index,
                                           semiring='max' if self.args.train_mode == 'max' else 'sum')
        self._dirty = False
        return self

    def parameters(self):
        tp = getattr(self, '_tp', None)
        return iter(()) if tp is None else iter([t for t in tp.values() if t.requires_grad])

    def named_parameters(self):
        tp = getattr(self, '_tp', None)
        return iter(()) if tp is None else iter([(k, t) for k, t in tp.items() if t.requires_grad])

    def sync_from_training(self):
        """Copy the trained language_tensor back into the host attributes the tagging handle is built from.  An
        edge-built model becomes a dense one (its edges no longer describe the weights)."""
        tp = getattr(self, '_tp', None)
        if tp is None or not self._dirty:
            return
        if getattr(self, 'edges', None) is not None:
            self.language_tensor, self.wildcard_mat, self.output_mat = self._dense()
            self.output_wildcard_vector = np.zeros(self.S, np.float32)
            self.edges = None
        self.language_tensor = tp['language_tensor'].detach().cpu().numpy()
        self._dirty = False
        self.invalidate()

    def eval(self):
        self.sync_from_training()
        return super().eval()

    def forward_local(self, input, label, lengths, train=True, re_tags=None):
        if not train:
            self.sync_from_training()
            return super().forward_local(input, label, lengths, train=False, re_tags=re_tags)
        from .train_step import onehot_ifst_train_step
        self.enable_training()
        tp = self._tp
        on_host = lengths.device.type == 'cpu'
        Lmax = int(lengths.max()) if on_host else int(lengths.max().item())
        ntok = int(lengths.clamp(0, Lmax).sum()) if on_host else None
        x = input[:, :Lmax]
        lab = label[:, :Lmax]
        loss, tags = onehot_ifst_train_step(self._tc, tp['language_tensor'], tp['wildcard_mat'], tp['output_mat'],
                                            tp['h0'], tp['hT'], self._tpP, x, lengths, lab, valid_tokens=ntok)
        self._dirty = True
        pred = self._flatten(tags, lengths.to(tags.device)).to(torch.int64).to(input.device)
        true = self._flatten(label, lengths).to(input.device)
        return loss, pred, true

    def state_dict(self):
        self.sync_from_training()
        if getattr(self, 'edges', None) is not None:
            T, W, O = self._dense()
            return {'h0': self.h0, 'hT': self.hT, 'language_tensor': T, 'wildcard_mat': W, 'output_mat': O,
                    'output_wildcard_vector': np.zeros(self.S, np.float32)}
        return {'h0': self.h0, 'hT': self.hT, 'language_tensor': self.language_tensor,
                'wildcard_mat': self.wildcard_mat, 'output_mat': self.output_mat,
                'output_wildcard_vector': self.output_wildcard_vector}


class FARNN_S_O(_OnehotBase):
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
                semiring='max' if a.train_mode == 'max' else 'sum', threshold=a.threshold,
                o_idx=self.o_idx, device=self.device_index)
        return _lib.create_onehot_fst4(
            self.language_tensor, self.wildcard_tensor, self.h0, self.hT, P=self._P(),
            semiring='max' if a.train_mode == 'max' else 'sum', threshold=a.threshold,
            o_idx=self.o_idx, device=self.device_index)

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
    @staticmethod
    def _fst_train_enabled():
        """RE2NN_ONEHOT_FST_TRAIN=1: the FST's training step (opt-in for its first release, as RE2NN_ONEHOT_MAX_TRAIN)"""
        return os.environ.get('RE2NN_ONEHOT_FST_TRAIN', '') == '1'

    def _check_trainable(self):
        """The cases the HIP training step does not cover, refused before any device work."""
        a = self.args
        if not self._fst_train_enabled():
            from ..train_onehot import no_training_step
            raise no_training_step(self)              # today's refusal, word for word
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

    def enable_training(self):
        """Device-resident tensors (language_tensor with requires_grad, wildcard_tensor iff args.train_wildcard, as in
        the reference :32-37) and the library context.  An edge-built model gets its dense tensors here (_dense())."""
        self._check_trainable()
        if getattr(self, '_tp', None) is not None:
            return self
        if not torch.cuda.is_available():
            raise _lib.FarnnError('no MI355X visible; the training step has no CPU fallback')
        dev = self._dev()
        sd = self.state_dict()
        grad = {'language_tensor': True, 'wildcard_tensor': bool(getattr(self.args, 'train_wildcard', 0))}
        self._tp = {}
        for k in ('language_tensor', 'wildcard_tensor', 'h0', 'hT'):
            t = torch.from_numpy(np.ascontiguousarray(sd[k], dtype=np.float32)).to(dev).clone()
            self._tp[k] = t.requires_grad_(grad.get(k, False))
        self._tpP = torch.from_numpy(np.ascontiguousarray(self.priority_full, dtype=np.float32)).to(dev) \
            if self.args.use_priority else None
        V = self._tp['language_tensor'].shape[0]
        self._tc = _lib.Fst4TrainContext(V, self.S, self.C, threshold=self.args.threshold, o_idx=self.o_idx,
                                         device=self.device_index, semiring='max' if self.args.train_mode == 'max' else 'sum')
        self._dirty = False
        return self

    def parameters(self):
        tp = getattr(self, '_tp', None)
        return iter(()) if tp is None else iter([t for t in tp.values() if t.requires_grad])

    def named_parameters(self):
        tp = getattr(self, '_tp', None)
        return iter(()) if tp is None else iter([(k, t) for k, t in tp.items() if t.requires_grad])

    def sync_from_training(self):
        """Copy the trained tensors back into the host attributes the tagging handle is built from (the handle's own
        premixed copy is stale after an optimizer step).  An edge-built model becomes a dense one."""
        tp = getattr(self, '_tp', None)
        if tp is None or not self._dirty:
            return
        if getattr(self, 'edges', None) is not None:
            self.wildcard_wildcard_mat = np.zeros((self.S, self.S), np.float32)
            self.edges = None
        self.language_tensor = tp['language_tensor'].detach().cpu().numpy()
        self.wildcard_tensor = tp['wildcard_tensor'].detach().cpu().numpy()
        self._dirty = False
        self.invalidate()

    def eval(self):
        self.sync_from_training()
        return super().eval()

    def forward_local(self, input, label, lengths, train=True, re_tags=None):
        if not train:
            self.sync_from_training()
            return super().forward_local(input, label, lengths, train=False, re_tags=re_tags)
        from .train_step import onehot_fst4_train_step
        self.enable_training()
        tp = self._tp
        on_host = lengths.device.type == 'cpu'
        Lmax = int(lengths.max()) if on_host else int(lengths.max().item())
        ntok = int(lengths.clamp(0, Lmax).sum()) if on_host else None
        x = input[:, :Lmax]
        lab = label[:, :Lmax]
        loss, tags = onehot_fst4_train_step(self._tc, tp['language_tensor'], tp['wildcard_tensor'], tp['h0'], tp['hT'],
                                            self._tpP, x, lengths, lab, valid_tokens=ntok)
        self._dirty = True
        pred = self._flatten(tags, lengths.to(tags.device)).to(torch.int64).to(input.device)
        true = self._flatten(label, lengths).to(input.device)
        return loss, pred, true

    def state_dict(self):
        self.sync_from_training()
        if getattr(self, 'edges', None) is not None:
            T, W = self._dense()
            return {'h0': self.h0, 'hT': self.hT, 'language_tensor': T, 'wildcard_tensor': W,
                    'wildcard_wildcard_mat': np.zeros((self.S, self.S), np.float32)}
        return {'h0': self.h0, 'hT': self.hT, 'language_tensor': self.language_tensor,
                'wildcard_tensor': self.wildcard_tensor,
                'wildcard_wildcard_mat': self.wildcard_wildcard_mat}


class FARNN_S_O_I(_OnehotBase):
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
                semiring='max' if a.train_mode == 'max' else 'sum', mask_by_output=(a.independent == 2),
                threshold=a.threshold, o_idx=self.o_idx, device=self.device_index)
        return _lib.create_onehot_ind1(
            self.language_tensor, self.wildcard_mat, self.output_tensor, self.h0, self.hT, P=self._P(),
            semiring='max' if a.train_mode == 'max' else 'sum',
            mask_by_output=(a.independent == 2), threshold=a.threshold, o_idx=self.o_idx,
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
    @staticmethod
    def _ind1_train_enabled():
        """RE2NN_ONEHOT_IND1_TRAIN=1: this model's training step (opt-in for its first release, as RE2NN_ONEHOT_FST_TRAIN)"""
        return os.environ.get('RE2NN_ONEHOT_IND1_TRAIN', '') == '1'

    def _check_trainable(self):
        """The cases the HIP training step does not cover, refused before any device work."""
        if not self._ind1_train_enabled():            # before self.args is touched: the refusal needs the type only
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

    def enable_training(self):
        """Device-resident tensors (language_tensor the only one with requires_grad, as in the reference :209-223) and the
        library context.  An edge-built model gets its dense tensors here (_dense())."""
        self._check_trainable()
        if getattr(self, '_tp', None) is not None:
            return self
        if not torch.cuda.is_available():
            raise _lib.FarnnError('no MI355X visible; the training step has no CPU fallback')
        dev = self._dev()
        sd = self.state_dict()
        self._tp = {}
        for k in ('language_tensor', 'wildcard_mat', 'output_tensor', 'h0', 'hT'):
            t = torch.from_numpy(np.ascontiguousarray(sd[k], dtype=np.float32)).to(dev).clone()
            self._tp[k] = t.requires_grad_(k == 'language_tensor')
        self._tpP = torch.from_numpy(np.ascontiguousarray(self.priority_full, dtype=np.float32)).to(dev) \
            if self.args.use_priority else None
        V = self._tp['language_tensor'].shape[0]
        self._tc = _lib.Ind1TrainContext(V, self.S, self.C, mask_by_output=(self.args.independent == 2),
                                         threshold=self.args.threshold, o_idx=self.o_idx, device=self.device_index,
                                         semiring='max' if self.args.train_mode == 'max' else 'sum')
        self._dirty = False
        return self

    def parameters(self):
        tp = getattr(self, '_tp', None)
        return iter(()) if tp is None else iter([t for t in tp.values() if t.requires_grad])

    def named_parameters(self):
        tp = getattr(self, '_tp', None)
        return iter(()) if tp is None else iter([(k, t) for k, t in tp.items() if t.requires_grad])

    def sync_from_training(self):
        """Copy the trained language_tensor back into the host attributes the tagging handle is built from.  An
        edge-built model becomes a dense one (its edges no longer describe the weights)."""
        tp = getattr(self, '_tp', None)
        if tp is None or not self._dirty:
            return
        if getattr(self, 'edges', None) is not None:
            self.language_tensor, self.wildcard_mat, self.output_tensor = self._dense()
            self.output_wildcard_mat = None
            self.edges = None
        self.language_tensor = tp['language_tensor'].detach().cpu().numpy()
        self._dirty = False
        self.invalidate()

    def eval(self):
        self.sync_from_training()
        return super().eval()

    def forward_local(self, input, label, lengths, train=True, re_tags=None):
        if not train:
            self.sync_from_training()
            return super().forward_local(input, label, lengths, train=False, re_tags=re_tags)
        from .train_step import onehot_ind1_train_step
        self.enable_training()
        tp = self._tp
        on_host = lengths.device.type == 'cpu'
        Lmax = int(lengths.max()) if on_host else int(lengths.max().item())
        ntok = int(lengths.clamp(0, Lmax).sum()) if on_host else None
        x = input[:, :Lmax]
        lab = label[:, :Lmax]
        loss, tags = onehot_ind1_train_step(self._tc, tp['language_tensor'], tp['wildcard_mat'], tp['output_tensor'],
                                            tp['h0'], tp['hT'], self._tpP, x, lengths, lab, valid_tokens=ntok)
        self._dirty = True
        pred = self._flatten(tags, lengths.to(tags.device)).to(torch.int64).to(input.device)
        true = self._flatten(label, lengths).to(input.device)
        return loss, pred, true

    def state_dict(self):
        self.sync_from_training()
        if getattr(self, 'edges', None) is not None:
            T, W, O = self._dense()
            return {'h0': self.h0, 'hT': self.hT, 'language_tensor': T, 'wildcard_mat': W, 'output_tensor': O}
        return {'h0': self.h0, 'hT': self.hT, 'language_tensor': self.language_tensor,
                'wildcard_mat': self.wildcard_mat, 'output_tensor': self.output_tensor}
