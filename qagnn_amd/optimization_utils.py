"""Optimisers behind the reference's OPTIMIZER_CLASSES interface (reference utils/optimization_utils.py:100-105).

`RAdam` keeps the reference's constructor, hyper-parameter groups, state layout (`step`, `exp_avg`, `exp_avg_sq` per
parameter, so optimizer.state_dict() round-trips with the reference's) and update rule (utils/optimization_utils.py:31-97),
but the update itself is ONE fused multi-tensor HIP launch sequence per (group, step count) instead of ~10 elementwise
kernels per parameter in a Python loop: the decoder has ~70 tensors / 2.85 M parameters, so a reference step is ~700 tiny
launches.  fp32 parameters on the GPU go through libqagnn_hip's qagnn_radam_step_f32; parameters that live on the CPU (unit
tests of the training driver) are updated with the same formulas in torch.

`clip_grad_norm_` is the line in front of the optimiser step in the reference's training loop (qagnn.py:267-278): the global L2 norm
and the clip coefficient are computed on the device (qagnn_grad_norm_f32) and applied either in place (qagnn_scale_multi_f32, any
optimiser) or, with `defer_to=` a `RAdam` of this module, inside that optimiser's next step as it reads the gradients.
"""
import math

import torch
from torch.optim import SGD, Adam
from torch.optim.optimizer import Optimizer


def radam_step_size(step, beta1, beta2, degenerated_to_sgd=True):
    """(N_sma, step_size) of the rectified update at `step` (utils/optimization_utils.py:63-80)."""
    beta2_t = beta2 ** step
    n_sma_max = 2 / (1 - beta2) - 1
    n_sma = n_sma_max - 2 * step * beta2_t / (1 - beta2_t)
    if n_sma >= 5:
        step_size = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_sma_max - 4) * (n_sma - 2) / n_sma * n_sma_max / (n_sma_max - 2)) / \
            (1 - beta1 ** step)
    elif degenerated_to_sgd:
        step_size = 1.0 / (1 - beta1 ** step)
    else:
        step_size = -1
    return n_sma, step_size


def radam_mode(n_sma, step_size):
    """the branch of the update: 2 rectified (N_sma >= 5), 1 SGD-like, 0 moments only (step_size < 0: degenerated_to_sgd=False below 5)"""
    return 2 if n_sma >= 5 else (1 if step_size > 0 else 0)


def radam_record(group, step, degenerated_to_sgd=True):
    """What the update of one tensor of `group` at step count `step` reads from its device record when the step is replayed from a captured
    graph (include/ext/qagnn_hip_step.h: qagnn_step_record), as Python doubles: exactly the doubles RAdam.step() hands to
    qagnn_radam_step_scaled_f32, combined as that entry point combines them.  The ONE rounding to fp32 happens where they are stored into
    the record (_step.pack_records), as it happens there in the `(float)` casts."""
    beta1, beta2 = group['betas']
    lr, wd = float(group['lr']), float(group['weight_decay'])
    n_sma, step_size = radam_step_size(step, beta1, beta2, degenerated_to_sgd)
    return dict(decay=-wd * lr, s=-float(step_size) * lr, mode=radam_mode(n_sma, step_size), beta1=float(beta1), beta2=float(beta2),
                ob1=1.0 - float(beta1), ob2=1.0 - float(beta2), eps=float(group['eps']))


class AdamW(Optimizer):
    """`transformers.AdamW` as the reference imports it (utils/optimization_utils.py:3; transformers == 3.4.0 is pinned in the
    reference's README, the class has since been removed from transformers): its defaults -- eps = 1e-6, weight_decay = 0.0,
    correct_bias = True -- AND its update rule, which is not torch.optim.AdamW's:

        m <- b1 m + (1 - b1) g;   v <- b2 v + (1 - b2) g^2
        p <- p - lr * sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps)        (eps is added to the UNcorrected sqrt(v): an effective
        p <- p - lr * weight_decay * p                                           eps of eps / sqrt(1 - b2^t), ~30x larger at t = 1;
                                                                                 the decay uses the parameter AFTER the Adam update)

    torch's class divides sqrt(v) by sqrt(1 - b2^t) before adding eps and applies the decay first.  The reference's driver sets
    weight_decay per parameter group and never passes eps (qagnn.py:196-206).  State layout as transformers': `step`, `exp_avg`,
    `exp_avg_sq` per parameter.  One multi-tensor (foreach) op sequence per group."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[1]))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            beta1, beta2 = group['betas']
            by_step = {}  # parameters that share a step count share their scalar factors
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError('Adam does not support sparse gradients, please consider SparseAdam instead')
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = 0
                    state['exp_avg'] = torch.zeros_like(p)
                    state['exp_avg_sq'] = torch.zeros_like(p)
                state['step'] += 1
                by_step.setdefault(state['step'], []).append(p)
            for t, ps in by_step.items():
                grads = [p.grad for p in ps]
                m = [self.state[p]['exp_avg'] for p in ps]
                v = [self.state[p]['exp_avg_sq'] for p in ps]
                torch._foreach_mul_(m, beta1)
                torch._foreach_add_(m, grads, alpha=1.0 - beta1)
                torch._foreach_mul_(v, beta2)
                torch._foreach_addcmul_(v, grads, grads, value=1.0 - beta2)
                denom = torch._foreach_sqrt(v)
                torch._foreach_add_(denom, group['eps'])
                step_size = group['lr']
                if group['correct_bias']:
                    step_size = step_size * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
                torch._foreach_addcdiv_(ps, m, denom, value=-step_size)
                if group['weight_decay'] > 0.0:
                    torch._foreach_mul_(ps, 1.0 - group['lr'] * group['weight_decay'])  # p <- p + (-lr wd) p, one rounding per element
        return loss


class RAdam(Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, degenerated_to_sgd=True):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(betas[1]))
        self.degenerated_to_sgd = degenerated_to_sgd
        self._grad_scale = None
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def defer_grad_scale(self, scale):
        """The NEXT step() reads every gradient as grad * scale (a one-element fp32 tensor, e.g. the clip coefficient left on the device
        by clip_grad_norm_(..., defer_to=self)) and leaves the gradients themselves untouched; consumed by that one step.  None: no scale."""
        if scale is not None and not (isinstance(scale, torch.Tensor) and scale.numel() == 1 and scale.dtype == torch.float32):
            raise TypeError('defer_grad_scale: need a one-element fp32 tensor or None')
        self._grad_scale = scale

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        scale, self._grad_scale = self._grad_scale, None
        for group in self.param_groups:
            beta1, beta2 = group['betas']
            buckets = {}  # (step, on_gpu) -> lists: parameters that share a step count share step_size and the branch taken
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError('RAdam does not support sparse gradients')
                state = self.state[p]
                if len(state) == 0:
                    state['step'] = 0
                    state['exp_avg'] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                    state['exp_avg_sq'] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                state['step'] += 1
                fused = p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()
                buckets.setdefault((state['step'], fused, p.device if fused else None), []).append(p)
            for (step, fused, dev), ps in buckets.items():
                n_sma, step_size = radam_step_size(step, beta1, beta2, self.degenerated_to_sgd)
                mode = 2 if n_sma >= 5 else (1 if step_size > 0 else 0)
                if fused:
                    from . import ops
                    grads = [p.grad if (p.grad.dtype == torch.float32 and p.grad.is_contiguous()) else p.grad.float().contiguous() for p in ps]
                    ops.kernels().radam_step(list(ps), grads, [self.state[p]['exp_avg'] for p in ps],
                                             [self.state[p]['exp_avg_sq'] for p in ps], beta1, beta2, group['eps'], group['lr'],
                                             group['weight_decay'], step_size, mode,
                                             grad_scale=None if scale is None else scale.to(dev).reshape(1))
                    continue
                for p in ps:  # CPU tensors / other dtypes: the same update, tensor by tensor (utils/optimization_utils.py:52-93)
                    state = self.state[p]
                    grad = p.grad.float()
                    if scale is not None:
                        grad = grad * scale.to(grad.device).reshape(())
                    p32 = p.float()
                    m, v = state['exp_avg'], state['exp_avg_sq']
                    v.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
                    m.mul_(beta1).add_(grad, alpha=1 - beta1)
                    if mode == 0:
                        continue
                    if group['weight_decay'] != 0:
                        p32.add_(p32, alpha=-group['weight_decay'] * group['lr'])
                    if mode == 2:
                        p32.addcdiv_(m, v.sqrt().add_(group['eps']), value=-step_size * group['lr'])
                    else:
                        p32.add_(m, alpha=-step_size * group['lr'])
                    p.copy_(p32)
        return loss


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None, *, defer_to=None):
    """torch.nn.utils.clip_grad_norm_ as the reference's training loop calls it (qagnn.py:267-278), without leaving the device: returns
    the total norm (0-dim tensor) and scales the gradients by min(1, max_norm / (norm + 1e-6)).

    Fused path -- every gradient fp32, contiguous, dense and on ONE GPU, norm_type == 2, error_if_nonfinite false: two-stage deterministic
    norm + coefficient on the device (qagnn_grad_norm_f32), then
      defer_to=None       one multi-tensor launch sequence g *= coef (qagnn_scale_multi_f32): works with any optimiser;
      defer_to=optimizer  (this module's RAdam only) the gradients are left as they are and the optimiser keeps the coefficient word: its
                          next step() multiplies each gradient by it as it reads (qagnn_radam_step_scaled_f32) and then drops it.
    Every other input (CPU tensors, other dtypes, gradients on two devices as in the reference's encoder-on-cuda:0 / decoder-on-cuda:1
    layout, other norms, error_if_nonfinite) goes as a whole to torch.nn.utils.clip_grad_norm_, which clips in place; defer_to is
    ignored there and the optimiser is given nothing to apply."""
    if defer_to is not None and not isinstance(defer_to, RAdam):
        raise TypeError(f'clip_grad_norm_(defer_to=...) takes a {RAdam.__module__}.RAdam, whose step applies the coefficient; '
                        f'got {type(defer_to).__name__} (clip in place for every other optimiser: defer_to=None)')
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    parameters = list(parameters)
    grads = [p.grad for p in parameters if p.grad is not None]
    fused = (len(grads) > 0 and float(norm_type) == 2.0 and not error_if_nonfinite
             and all(g.is_cuda and g.dtype == torch.float32 and not g.is_sparse and g.is_contiguous() and g.device == grads[0].device
                     for g in grads))
    if not fused:
        if defer_to is not None:
            defer_to.defer_grad_scale(None)
        return torch.nn.utils.clip_grad_norm_(parameters, max_norm, norm_type=norm_type, error_if_nonfinite=error_if_nonfinite,
                                              foreach=foreach)
    from . import ops
    k = ops.kernels()
    out = k.grad_norm(grads, max_norm)
    if defer_to is not None:
        defer_to.defer_grad_scale(out[1:2])
    else:
        k.scale_multi(grads, out[1:2])
    return out[0]


OPTIMIZER_CLASSES = {
    'sgd': SGD,
    'adam': Adam,
    'adamw': AdamW,   # transformers.AdamW's defaults (eps 1e-6, weight_decay 0) over torch.optim.AdamW's update
    'radam': RAdam,
}
