"""Torch emulation of the trainable entity table's gradient (include/qagnn_hip_rows.h) on top of tests/emu_loss.py.  TEST INFRASTRUCTURE ONLY.

The three provider methods qagnn_amd._lib.HipKernels adds -- row_groups, row_segment_sum, rows_scatter -- and their two workspace
queries, with the header's definitions written out: a stable sort for the grouping, the segment sums in float64 rounded to fp32 once.
"""
import torch

from emu_loss import EmuLossKernels


class EmuRowKernels(EmuLossKernels):
    def row_groups_workspace_elems(self, N):
        return 4

    def row_segment_sum_workspace_elems(self, N, cols):
        return 4

    def row_groups(self, ridx, table_rows, order, seg, uniq, count, workspace):
        N = ridx.numel()
        live = ((ridx >= 0) & (ridx < table_rows)).nonzero().flatten()
        by_id = torch.argsort(ridx[live], stable=True)
        pos, ids = live[by_id], ridx[live][by_id]
        M = pos.numel()
        head = torch.ones(M, dtype=torch.bool)
        head[1:] = ids[1:] != ids[:-1]
        starts = head.nonzero().flatten()
        U = starts.numel()
        order[:N].fill_(-1)
        order[:M] = pos.to(order.dtype)
        seg[:N + 1].fill_(M)
        seg[:U] = starts.to(seg.dtype)
        uniq[:N].fill_(-1)
        uniq[:U] = ids[starts]
        count[0] = U
        return order, seg, uniq, count

    def row_segment_sum(self, X, order, seg, count, G, workspace):
        U = min(int(count[0]), G.size(0))
        G.zero_()
        Xd = X.detach().double()
        for u in range(U):
            rows = order[int(seg[u]):int(seg[u + 1])].long()
            G[u] = Xd[rows].sum(0).to(G.dtype)
        return G

    def rows_scatter(self, R, uniq, count, out, accumulate=False):
        U = min(int(count[0]), R.size(0))
        ids = uniq[:U]
        assert ids.unique().numel() == U and (U == 0 or (int(ids.min()) >= 0 and int(ids.max()) < out.size(0)))
        if accumulate:
            out[ids] += R[:U]
        else:
            out[ids] = R[:U]
        return out
