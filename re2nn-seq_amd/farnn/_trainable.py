"""The training surface all six trainable mirrors share (FARNN_S_O_I_S, FARNN_S_O, FARNN_S_O_I, FARNN_S_D_W_I_S,
FARNN_S_D_W_I, FARNN_S_D_W): device-resident leaf tensors for the optimizer, the library context, the step inside forward_local(train=True)
and the copy back into the host attributes the tagging handle is built from.

A class lists ``Trainable`` before its NativeTagger base and keeps what is its own:

  _TRAIN_FLAGS            state_dict() name -> None (always a gradient), an ``args`` flag name, or False (never), in parameter order
  _train_context()        opens its ``_lib.*TrainContext`` (looked up at call time)
  _train_call(...)        its one ``train_step.*`` call
  _copy_back(tp)          writes the trained tensors into the host attributes
  _check_trainable(...)   the configurations its step does not cover, refused before any device work
"""
import numpy as np
import torch

from .. import _lib


def _leaf(v, dev):
    t = v.detach() if torch.is_tensor(v) else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return t.to(dev).float().clone()


class Trainable:
    _check_needs_re_tags = False      # FARNN_S_D_W_I_S: its _check_trainable(re_tags) runs in forward_local only

    def _train_decl(self):
        """[(state_dict() name, requires_grad)]: the insertion order of _tp, and so the order of parameters()."""
        return [(k, True if f is None else bool(f and getattr(self.args, f, 0))) for k, f in self._TRAIN_FLAGS.items()]

    def _check_step(self, re_tags):
        """What forward_local(train=True) checks beyond enable_training(); the onehot models take no re_tags."""

    def enable_training(self):
        """Device-resident leaf tensors for the optimizer (returned by parameters()) and the library context.  An edge-built
        onehot model gets its dense tensors here (state_dict() -> _dense())."""
        if not self._check_needs_re_tags:
            self._check_trainable()
        if getattr(self, '_tp', None) is not None:
            return self
        if not torch.cuda.is_available():
            raise _lib.FarnnError('no MI355X visible; the training step has no CPU fallback')
        dev = self._dev()
        sd = self.state_dict()
        self._tp = {}
        for k, grad in self._train_decl():
            self._tp[k] = _leaf(sd[k], dev).requires_grad_(grad)
        self._tpP = _leaf(self.priority_full, dev) if self.args.use_priority else None
        self._tc = self._train_context()
        self._dirty = False
        return self

    def parameters(self):
        return iter([t for _, t in self.named_parameters()])

    def named_parameters(self):
        tp = getattr(self, '_tp', None)
        return iter(()) if tp is None else iter([(k, t) for k, t in tp.items() if t.requires_grad])

    def sync_from_training(self):
        """Copy the trained tensors back into the host attributes the tagging handle is built from (the handle's own copy is
        stale after an optimizer step)."""
        tp = getattr(self, '_tp', None)
        if tp is None or not self._dirty:
            return
        self._copy_back(tp)
        self._dirty = False
        self.invalidate()

    def eval(self):
        self.sync_from_training()
        return super().eval()

    def forward_local(self, input, label, lengths, train=True, re_tags=None):
        if not train:
            self.sync_from_training()
            return super().forward_local(input, label, lengths, train=False, re_tags=re_tags)
        self._check_step(re_tags)
        self.enable_training()
        on_host = lengths.device.type == 'cpu'        # then the token count costs no device round trip in the step
        Lmax = int(lengths.max()) if on_host else int(lengths.max().item())
        ntok = int(lengths.clamp(0, Lmax).sum()) if on_host else None
        loss, tags = self._train_call(input[:, :Lmax], lengths, label[:, :Lmax], ntok, re_tags)
        self._dirty = True
        pred = self._flatten(tags, lengths.to(tags.device)).to(torch.int64).to(input.device)
        true = self._flatten(label, lengths).to(input.device)
        return loss, pred, true

    def forward_local_device(self, input, label, lengths, re_tags=None):
        """forward_local(train=True) for a caller that scores on the device (metrics/device.py): the same
        checks and the same step, but (loss, tags [B, Lmax] int32, labels [B, Lmax] int64, lengths [B] int64) as they lie on the
        device -- no flatten and no copy to the host."""
        self._check_step(re_tags)
        self.enable_training()
        on_host = lengths.device.type == 'cpu'
        Lmax = int(lengths.max()) if on_host else int(lengths.max().item())
        ntok = int(lengths.clamp(0, Lmax).sum()) if on_host else None
        dev = self._dev()
        lab = label[:, :Lmax].to(device=dev, dtype=torch.int64).contiguous()
        ln = lengths.to(device=dev, dtype=torch.int64).contiguous()
        loss, tags = self._train_call(input[:, :Lmax], ln, lab, ntok, re_tags)
        self._dirty = True
        return loss, tags, lab, ln
