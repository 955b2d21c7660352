"""A numpy restatement of the two update rules of the library's optimizer step (farnn_optim_*, include/farnn.h), written
from the formulas, for the tests of re2nn_seq_amd.farnn.optim.  Evaluates in `dtype` (float32 or float64).

  Adam (torch.optim.Adam's defaults: betas 0.9 / 0.999, eps 1e-8, no weight decay, no amsgrad), t = the tensor's own step:
      m += (g - m) (1 - beta1)
      v  = beta2 v + (1 - beta2) g^2
      p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps),     bc1 = 1 - beta1^t, bc2 = 1 - beta2^t  (in double)
  SGD:  p -= lr g
A gradient of None skips the tensor: nothing changes and its step count does not advance."""
import numpy as np


class AdamRef:
    """State of one tensor list.  step(grads) applies one update; grads[i] is None for a tensor without a gradient."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, dtype=np.float64):
        self.dtype = dtype
        self.p = [np.array(a, dtype=dtype) for a in params]
        self.m = [np.zeros_like(a) for a in self.p]
        self.v = [np.zeros_like(a) for a in self.p]
        self.t = [0] * len(self.p)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)

    def step(self, grads):
        dt = self.dtype
        b1, b2 = self.betas
        for i, g in enumerate(grads):
            if g is None:
                continue
            g = np.asarray(g, dtype=dt)
            self.t[i] += 1
            bc1 = 1.0 - b1 ** self.t[i]
            bc2 = 1.0 - b2 ** self.t[i]
            self.m[i] = self.m[i] + (g - self.m[i]) * dt(1.0 - b1)
            self.v[i] = self.v[i] * dt(b2) + dt(1.0 - b2) * g * g
            denom = np.sqrt(self.v[i]) / dt(np.sqrt(bc2)) + dt(self.eps)
            self.p[i] = self.p[i] - dt(self.lr / bc1) * (self.m[i] / denom)
        return self


class SgdRef:
    def __init__(self, params, lr=1e-3, dtype=np.float64):
        self.dtype = dtype
        self.p = [np.array(a, dtype=dtype) for a in params]
        self.t = [0] * len(self.p)
        self.lr = float(lr)

    def step(self, grads):
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.t[i] += 1
            self.p[i] = self.p[i] - self.dtype(self.lr) * np.asarray(g, dtype=self.dtype)
        return self
