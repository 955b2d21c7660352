"""torch.optim.Adam and torch.optim.SGD on the library's multi-tensor optimizer step (farnn_optim_*, include/farnn.h;
DESIGN.md, row f6): step() updates every tensor of a parameter group in one launch on the current stream.

The optimizer state is torch's own: `exp_avg` and `exp_avg_sq` are torch tensors and `step` is a float32 scalar tensor on
the host, all in `self.state`, and the parameter groups carry torch's keys -- state_dict() loads into torch.optim.Adam and
torch.optim.Adam's loads here.  Weight decay, amsgrad, maximize and momentum are not implemented and are refused.  There
is no CPU fallback: parameters that are not on the HIP device raise FarnnError before any device work, and so does a
parameter or gradient that is not contiguous float32 (ValueError).  step() is not to be captured into a HIP graph (the
bias corrections are computed on the host per call)."""
import torch

from .. import _lib


def _torch_defaults(cls, **kw):
    """the parameter-group keys of torch's own optimizer (they differ between torch versions), so that state dicts interchange"""
    return dict(cls([torch.zeros(1)], **kw).defaults)


class _NativeOptimizer(torch.optim.Optimizer):
    _kind = None
    _refused = ()               # group keys that must stay falsy

    def __init__(self, params, defaults):
        self._handles = {}      # group index -> (key, _lib.Optim)
        self._synced = {}       # group index -> the handle's step counts equal self.state's
        super().__init__(params, defaults)

    def add_param_group(self, group):
        super().add_param_group(group)
        self._check_devices(self.param_groups[-1])

    @staticmethod
    def _check_devices(group):
        for p in group['params']:
            if p.device.type != 'cuda':
                raise _lib.FarnnError('the optimizer step runs on the HIP device only (no CPU fallback): a parameter lives on {}'.format(p.device))

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._synced = {}

    def __setstate__(self, state):           # (unpickled: the library handles are built again by the first step)
        super().__setstate__(state)
        self._handles, self._synced = {}, {}

    def _check_group(self, group):
        self._check_devices(group)
        for k in self._refused:
            if group.get(k):
                raise ValueError('{} = {!r} is not implemented by the library optimizer (DESIGN.md, row f6)'.format(k, group[k]))
        dev = group['params'][0].device
        for p in group['params']:
            if p.device != dev:
                raise ValueError('the parameters of one group must share one device')
            for t, what in ((p, 'parameter'), (p.grad, 'gradient')):
                if t is None:
                    continue
                if t.is_sparse or t.dtype != torch.float32:
                    raise ValueError('the library optimizer takes dense float32 {}s, got {}'.format(what, t.dtype))
                if not t.is_contiguous():
                    raise ValueError('a {} is not contiguous'.format(what))
        return dev

    def _handle(self, gi, group, key):
        have = self._handles.get(gi)
        if have is None or have[0] != key:
            if have is not None:
                have[1].close()
            dev = group['params'][0].device
            have = (key, self._open(group, dev.index if dev.index is not None else torch.cuda.current_device()))
            self._handles[gi] = have
            self._synced.pop(gi, None)
        h = have[1]
        if h.lr != float(group['lr']):
            h.set_lr(group['lr'])
        return h

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:      # every refusal comes before any group's device work
            if group['params']:
                self._check_group(group)
        for gi, group in enumerate(self.param_groups):
            if group['params']:
                self._step_group(gi, group)
        return loss


class Adam(_NativeOptimizer):
    """torch.optim.Adam(params, lr, betas, eps) with weight_decay = 0 and amsgrad = False."""
    _kind = _lib.OPTIM_ADAM
    _refused = ('weight_decay', 'amsgrad', 'maximize', 'capturable', 'differentiable', 'decoupled_weight_decay')

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0):
        if weight_decay:
            raise ValueError('weight_decay is not implemented by the library optimizer (DESIGN.md, row f6)')
        super().__init__(params, _torch_defaults(torch.optim.Adam, lr=lr, betas=betas, eps=eps))

    def _open(self, group, device):
        b1, b2 = group['betas']
        return _lib.Optim(self._kind, [p.numel() for p in group['params']], group['lr'], b1, b2, group['eps'], device=device)

    def _step_group(self, gi, group):
        params = group['params']
        b1, b2 = group['betas']
        h = self._handle(gi, group, (tuple(p.numel() for p in params), float(b1), float(b2), float(group['eps']), params[0].device))
        P, G, M, V, stepped = [], [], [], [], []
        for p in params:
            g = p.grad
            if g is None:
                P.append(None); G.append(None); M.append(None); V.append(None)
                continue
            st = self.state[p]
            if len(st) == 0:                 # torch's lazy state, torch's layout (step: a float32 scalar on the host)
                st['step'] = torch.tensor(0.0, dtype=torch.float32)
                st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            m, v = st['exp_avg'], st['exp_avg_sq']
            if not (m.is_contiguous() and v.is_contiguous() and m.dtype == v.dtype == torch.float32 and m.device == v.device == p.device):
                raise ValueError('exp_avg / exp_avg_sq must be contiguous float32 tensors on the parameter\'s device')
            P.append(p.data_ptr()); G.append(g.data_ptr()); M.append(m.data_ptr()); V.append(v.data_ptr())
            stepped.append(st)
        if not stepped:
            return
        if not self._synced.get(gi):         # a fresh handle or a loaded state: the library's counts follow self.state
            for i, p in enumerate(params):
                st = self.state.get(p)
                h.set_steps(i, int(st['step']) if st else 0)
            self._synced[gi] = True
        h.step(P, G, M, V, torch.cuda.current_stream(params[0].device).cuda_stream)
        for st in stepped:
            st['step'] += 1


class SGD(_NativeOptimizer):
    """torch.optim.SGD(params, lr) with momentum = 0 and weight_decay = 0: param -= lr * grad.  It keeps no state."""
    _kind = _lib.OPTIM_SGD
    _refused = ('momentum', 'dampening', 'weight_decay', 'nesterov', 'maximize', 'differentiable')

    def __init__(self, params, lr=1e-3, weight_decay=0):
        if weight_decay:
            raise ValueError('weight_decay is not implemented by the library optimizer (DESIGN.md, row f6)')
        super().__init__(params, _torch_defaults(torch.optim.SGD, lr=lr))

    def _open(self, group, device):
        return _lib.Optim(self._kind, [p.numel() for p in group['params']], group['lr'], device=device)

    def _step_group(self, gi, group):
        params = group['params']
        h = self._handle(gi, group, (tuple(p.numel() for p in params), params[0].device))
        grads = [None if p.grad is None else p.grad.data_ptr() for p in params]
        if any(g is not None for g in grads):
            h.step([p.data_ptr() for p in params], grads, None, None, torch.cuda.current_stream(params[0].device).cuda_stream)
