"""Torch emulation of the training losses (include/qagnn_hip_loss.h) on top of tests/emu_kernels.py.  TEST INFRASTRUCTURE ONLY.

The two provider methods qagnn_amd._lib.HipKernels adds -- choice_loss, choice_loss_bwd -- with the header's formulas written out (no
autograd, no torch loss module: those are the yardstick of tests/test_choice_loss.py), computed in float64 and rounded to fp32 once.
"""
import torch

from emu_infer import EmuInferKernels


class EmuLossKernels(EmuInferKernels):
    def __init__(self):
        super().__init__()
        self.bad_labels = 0  # rows with a label outside [0, nc) seen so far (the library's flag word)

    def zero_words(self, t):
        return t.zero_()

    def choice_loss(self, logits, labels, kind='cross_entropy', margin=0.1, weight=None, stats=None, g=None):
        Q, nc = logits.shape
        x = logits.detach().double()
        w = 1.0 if weight is None else float(weight.reshape(-1)[0])
        m = float(torch.tensor(margin, dtype=torch.float32))
        total, grad = 0.0, torch.zeros(Q, nc, dtype=torch.float64)
        for q in range(Q):
            l = int(labels[q])
            if not 0 <= l < nc:
                self.bad_labels += 1
                continue
            if kind == 'cross_entropy':
                e = torch.exp(x[q] - x[q].max())
                total += float(torch.log(e.sum()) - (x[q, l] - x[q].max()))
                grad[q] = e / e.sum() * (w / Q)
                grad[q, l] -= w / Q
            else:
                assert kind == 'margin_rank' and nc >= 2
                for c in range(nc):
                    h = float(m - x[q, l] + x[q, c])
                    if c != l and h >= 0:  # (a pair on the kink is active)
                        total += h
                        grad[q, c] += w / (Q * (nc - 1))
                        grad[q, l] -= w / (Q * (nc - 1))
        loss = torch.tensor([w * total / (Q * (nc - 1) if kind == 'margin_rank' else Q)], dtype=torch.float64).float()
        if stats is not None:
            stats[0] += loss[0].double()
            stats[1] += 1
        out = grad.float()
        if g is not None:
            g.copy_(out)
            out = g
        return loss, out

    def choice_loss_bwd(self, g, grad_out, out=None):
        r = g * grad_out.reshape(-1)[0]
        if out is not None:
            out.copy_(r)
            return out
        return r
