"""FusedAdam -- torch.optim.Adam (amsgrad = maximize = False, L2 weight decay per group: what the reference's train.py:77-82 builds
with --adam) with the whole step as ONE HIP launch (csrc/optim.hip: adam_batch_kernel) instead of ATen's chain of about 60 foreach kernels over
the 294 parameter tensors of Darknet-53.  Same fp32 arithmetic in the same operator order; same `param_groups` keys and defaults and the
same `state[p]` layout ('step' a CPU fp32 scalar, 'exp_avg', 'exp_avg_sq'), so `state_dict()` is interchangeable with torch.optim.Adam's
in both directions.  Parameters that are not contiguous fp32 CUDA tensors, amsgrad, maximize, capturable, differentiable and decoupled
weight decay (AdamW) are not supported (construct torch.optim.Adam for those)."""
import torch

from .. import _lib
from .._lib import AdamJob as _Job

_REFUSED = ('amsgrad', 'maximize', 'capturable', 'differentiable', 'decoupled_weight_decay')


def _check_group(group):
    for k in _REFUSED:
        if group.get(k):
            raise ValueError("FusedAdam does not support %s=True (construct torch.optim.Adam)" % k)
    lr, (beta1, beta2) = group['lr'], group['betas']
    if isinstance(lr, torch.Tensor) or isinstance(beta1, torch.Tensor) or isinstance(beta2, torch.Tensor):
        raise ValueError("FusedAdam takes lr and betas as Python numbers (a tensor lr is torch.optim.Adam's capturable path)")
    if not 0.0 <= lr:
        raise ValueError("Invalid learning rate: %r" % (lr,))
    if not 0.0 <= group['eps']:
        raise ValueError("Invalid epsilon value: %r" % (group['eps'],))
    if not 0.0 <= beta1 < 1.0 or not 0.0 <= beta2 < 1.0:
        raise ValueError("Invalid beta parameters: %r" % (group['betas'],))
    if not 0.0 <= group['weight_decay']:
        raise ValueError("Invalid weight_decay value: %r" % (group['weight_decay'],))


class FusedAdam(torch.optim.Optimizer):
    # workgroups of a tensor of n elements: ceil(n / elems_per_block), at most max_blocks; it grid-strides the rest.
    # (tools/optim_step_bench.py measures this sizing against a grid capped near 2048 workgroups: DESIGN 3.5)
    elems_per_block = 2048
    max_blocks = 1024

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=foreach,
                        capturable=capturable, differentiable=differentiable, fused=fused, decoupled_weight_decay=decoupled_weight_decay)
        _check_group(defaults)
        super(FusedAdam, self).__init__(params, defaults)
        self._key = None
        self.grad_scale = 1.0        # data parallel: 1 / world (the all-reduce delivers the SUM; dist.py then skips its div_)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        f32, stepped, dev = torch.float32, [], None
        for gi, group in enumerate(self.param_groups):      # refuse before anything is touched
            _check_group(group)          # a loaded or edited group may carry what the constructor refuses
            for p in group['params']:
                g = p.grad
                if g is None:            # no job, no state, no step increment
                    continue
                dev = p.device if dev is None else dev
                st = self.state.get(p)   # (state is a defaultdict: indexing it would create the entry)
                ok = p.is_cuda and p.device == dev and g.device == dev and p.dtype == f32 and g.dtype == f32 and p.is_contiguous() \
                    and g.is_contiguous() and g.shape == p.shape
                if ok and st:
                    m, v = st['exp_avg'], st['exp_avg_sq']
                    ok = m.device == dev and v.device == dev and m.dtype == f32 and v.dtype == f32 and m.is_contiguous() \
                        and v.is_contiguous() and m.shape == p.shape and v.shape == p.shape
                if not ok:
                    raise RuntimeError("FusedAdam handles contiguous fp32 CUDA parameters and gradients on one device (and moments of their shape)")
                stepped.append((gi, p, g, st))
        if not stepped:
            return loss
        states = []
        for _, p, _, st in stepped:
            if not st:
                st = self.state[p]
                st['step'] = torch.tensor(0.0, dtype=f32)
                st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
            states.append(st)
        # the step counts: CPU scalars as torch keeps them (a checkpoint loaded with map_location may have put them on the GPU).  Counted
        # up the way torch.optim.Adam does it: one `+= 1` per tensor wraps the 1 again each time and costs several times the launch
        steps = [st['step'] for st in states]
        if all(s.is_cpu for s in steps):
            torch._foreach_add_(steps, torch.tensor(1.0), alpha=1.0)
        else:
            for s in steps:
                s.add_(1)
        ts = [s.item() for s in steps]
        rows, row_of, ptrs = [], {}, []
        gs = 0.0 if self.grad_scale == 1.0 else float(self.grad_scale)
        for (gi, p, g, _), st, t in zip(stepped, states, ts):
            row = row_of.get((gi, t))
            if row is None:              # torch counts steps per parameter: one row per (group, step count), in doubles as torch does
                group = self.param_groups[gi]
                beta1, beta2 = group['betas']
                row = row_of[gi, t] = len(rows)
                rows.append([-(group['lr'] / (1 - beta1 ** t)), (1 - beta2 ** t) ** 0.5, 1 - beta1, beta2, 1 - beta2, group['eps'],
                             group['weight_decay'], gs])
            m, v = st['exp_avg'], st['exp_avg_sq']
            ptrs.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), row))
        key = (self.elems_per_block, self.max_blocks, tuple(ptrs))
        if key != self._key:                       # a pointer or a row assignment changed (first step, new gradient tensors): rebuild + upload
            arr = (_Job * len(ptrs))()
            blk = 0
            for q, (pp, gp, mp, vp, n, row) in enumerate(ptrs):
                nb = max(1, min(self.max_blocks, (n + self.elems_per_block - 1) // self.elems_per_block))
                arr[q] = _Job(pp, gp, mp, vp, n, row, blk, blk + nb)
                blk += nb
            self._jobs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
            self._n, self._blocks, self._key = len(ptrs), blk, key
        hp = torch.tensor(rows, dtype=torch.float32).to(dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().ryolo_adam_step(self._jobs.data_ptr(), self._n, self._blocks, hp.data_ptr(), _lib.stream_ptr(dev)),
                       "ryolo_adam_step")
        # the kernel wrote the parameters through raw pointers: tell autograd (and everything that watches tensor versions --
        # Darknet's cached eval engines hold packed copies of the weights and compare versions before they are reused)
        torch.autograd.graph.increment_version([p for _, p, _, _ in stepped])
        return loss
