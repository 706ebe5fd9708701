"""Torch emulation of the forward-only path (include/qagnn_hip_infer.h) on top of tests/emu_kernels.py.  TEST INFRASTRUCTURE ONLY.

The three provider methods qagnn_amd._lib.HipKernels adds for the path -- bn_relu_absmax, choice_eval, stack_infer -- as the expected
value of the `-m gpu` tests and as the CPU provider of the host-logic tests (routing, evaluate_accuracy, the eval golden cases).
"""
import torch

from emu_kernels import EmuKernels
from qagnn_amd._lib import HOP_AMAX_WORDS


class EmuInferKernels(EmuKernels):
    def bn_relu_absmax(self, H, scale, shift, out=None):
        """the bit pattern of max relu(scale * H + shift) (NaNs skipped, nothing positive: 0) merged into out[0] by integer max"""
        v = torch.relu(H.double() * scale.double() + shift.double()).float()
        v = torch.where(torch.isnan(v), torch.zeros_like(v), v)
        word = int(v.max().view(torch.int32).item()) if v.numel() else 0
        if out is None:
            out = torch.zeros(4, dtype=torch.int32)
        out[0] = max(int(out[0]), word)
        return out

    def choice_eval(self, logits, labels, counts, pred=None):
        Q, nc = logits.shape
        p = torch.empty(Q, dtype=torch.long)
        for q in range(Q):  # written out: the first index among equals, a NaN is the greatest (and the first NaN wins)
            best, bi = logits[q, 0].item(), 0
            for c in range(1, nc):
                v = logits[q, c].item()
                if best == best and (v > best or v != v):
                    best, bi = v, c
            p[q] = bi
        if pred is not None:
            pred.copy_(p)
        if labels is not None:
            counts[0] += int((p == labels.cpu()).sum())
        counts[1] += Q
        return counts

    def stack_infer(self, graph, HP, qscale, X, S, ntype, prms, eps, cols=-1, x_amax=None, s_amax=None, keep=False):
        """k hops with running statistics, no dropout, through the composed per-kernel path; -> (y, amax words: none filled here)"""
        from qagnn_amd import ops
        x, saved = X, []
        for prm in prms:
            y, sv = ops.hop_fwd_composed(self, graph, HP, qscale, x, S, ntype, prm, False, eps, 0.0, 0, True, None, cols)
            saved.append(dict(zip(('KMQ', 'aa', 'aggr', 'h1', 'out', 'stats'), sv), y=y))
            x = y
        amax = torch.zeros((len(prms), HOP_AMAX_WORDS), dtype=torch.int32)
        return (x, amax, saved) if keep else (x, amax)
