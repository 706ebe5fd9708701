"""The training loss of the multiple-choice head, native and without a host wait per mini-batch.

The reference builds its loss inside train() (qagnn.py:208-224: nn.CrossEntropyLoss, or nn.MarginRankingLoss on pairs picked with
boolean-mask indexing, which synchronises the host) and logs it with one `loss.item()` per mini-batch (qagnn.py:266).  Here

  * `compute_loss` is the drop-in for that closure: one launch gives the loss and its gradient with respect to the logits
    (ops.choice_loss -> qagnn_choice_loss_f32, include/qagnn_hip_loss.h), both kinds, capturable into a hipGraph;
  * `LossMeter` keeps the running sum and count of the losses in two doubles ON THE DEVICE, added to by the loss kernel itself:
    `read()` is the one synchronisation of a logging window.
"""
import torch

from . import ops

LOSSES = ops.LOSS_KINDS


def check_loss_name(loss):
    if loss not in LOSSES:
        raise ValueError(f'unknown loss {loss!r}: one of {LOSSES}')
    return loss


class LossMeter:
    """meter = LossMeter(device);  compute_loss(..., meter=meter) adds every loss to it on the device;
    total, count = meter.read()  -- the sequential float64 sum of the fp32 losses since reset() and their number, one synchronisation."""

    def __init__(self, device):
        self.stats = torch.zeros(2, dtype=torch.float64, device=device)

    def reset(self):
        """zero the two doubles with the library's zeroing kernel where there is one (no memset node inside a captured region)"""
        K = ops._K if ops._K is not None else (ops.kernels() if self.stats.is_cuda else None)
        if self.stats.is_cuda and hasattr(K, 'zero_words'):
            K.zero_words(self.stats)
        else:
            self.stats.zero_()

    def read(self):
        total, count = self.stats.tolist()
        return total, int(count)


def compute_loss(logits, labels, loss='cross_entropy', margin=0.1, weight=None, meter=None):
    """logits [bs, nc] (any floating dtype: computed in fp32, as under the reference's autocast), labels int64 [bs] -> the scalar loss,
    times `weight` (a float or a one-element fp32 device tensor, e.g. the reference's (b - a) / bs) where one is given.
    loss: 'cross_entropy' | 'margin_rank' (the reference's --loss), margin: its MarginRankingLoss margin (0.1 there)."""
    check_loss_name(loss)
    if logits.dtype != torch.float32:
        logits = logits.float()
    return ops.choice_loss(logits, labels, loss, margin, weight, meter.stats if meter is not None else None)
