"""Torch emulation of the two kernels of include/ext/qagnn_hip_step.h.  TEST INFRASTRUCTURE ONLY.

The header's definitions written out in fp32 torch arithmetic on whatever device the tensors live on: the update of one tensor from its
record (a ctypes qagnn_step_record, i.e. fp32 scalars), and the window accumulation as a select.  Not bit-exact with the kernels (no fused
multiply-add on the CPU); held to the bars the eager kernel's emulation is held to.
"""
import torch


def _f(x):
    return torch.tensor(float(x), dtype=torch.float32)


def radam_step_records(params, grads, exp_avgs, exp_avg_sqs, rec_index, records, grad_scale=None):
    """qagnn_radam_step_records_f32: `records` a host array of qagnn_step_record (what _step.pack_records returns)"""
    with torch.no_grad():
        for p, g, m, v, ri in zip(params, grads, exp_avgs, exp_avg_sqs, rec_index):
            r = records[ri]
            assert r.mode in (0, 1, 2)
            g = g.float()
            if grad_scale is not None:
                g = g * grad_scale.reshape(()).to(g.device)
            v.mul_(_f(r.beta2)).add_(_f(r.ob2) * g * g)
            m.mul_(_f(r.beta1)).add_(_f(r.ob1) * g)
            if r.mode == 0:
                continue
            if r.decay != 0.0:
                p.add_(_f(r.decay) * p)
            p.add_(_f(r.s) * (m / (v.sqrt() + _f(r.eps))) if r.mode == 2 else _f(r.s) * m)


def window_accumulate(dst, src, first):
    """qagnn_window_accumulate_f32: a select on the word, dst is not read where it is set"""
    with torch.no_grad():
        for d, s in zip(dst, src):
            if int(first) != 0:
                d.copy_(s)
            else:
                d.add_(s)
