"""Torch emulation of the forward-only stack with an attention buffer per hop, on top of tests/emu_infer.py.  TEST INFRASTRUCTURE ONLY.

What qagnn_amd._lib.HipKernels.stack_infer(attn=True) hands ops.attention_capture: the hops' pre-degree softmax in source order,
[k, Ep, 4].  The provider has NO attn_export / attn_trace: under it qagnn_amd.explain takes its stock-torch forms, which is what the
`-m "not gpu"` tests of the module run."""
import torch

from emu_infer import EmuInferKernels


class EmuExplainKernels(EmuInferKernels):
    infer_attn = True

    def __init__(self):
        self.calls = []

    def stack_infer(self, graph, HP, qscale, X, S, ntype, prms, eps, cols=-1, x_amax=None, s_amax=None, keep=False, attn=False):
        self.calls.append('stack_infer+attn' if attn else 'stack_infer')
        if not attn:
            return super().stack_infer(graph, HP, qscale, X, S, ntype, prms, eps, cols, x_amax, s_amax, keep)
        y, amax, saved = super().stack_infer(graph, HP, qscale, X, S, ntype, prms, eps, cols, x_amax, s_amax, True)
        return y, amax, torch.stack([sv['aa'][0] for sv in saved])
