"""Detailed evaluation: the attention of an eval forward, per layer, and its trace out of the QA context node.

The reference's `eval_detail` mode (qagnn.py:343-430) calls `model(*input_data, detail=True)`, which hands the graphs back so that the
attention can be laid over them: the interpretability half of QA-GNN.  On the fast path no `GATConvE.forward` is entered (all k hops are
one native call), so there is nothing to hook; this module is the way to the attention instead.

  * `trace(model, *inputs)` runs ONE eval forward on the inference path under `ops.attention_capture()` and follows the attention of
    its k hops out of the context node (node slot 0) of every subgraph, on the device (qagnn_attn_trace_f32, include/qagnn_hip_explain.h):
        flow_{l+1}[t] = sum over the edges s -> t of abar_l[edge] * flow_l[s]      the share of the context node's attention mass on t
        best_{l+1}[t] = max over the edges s -> t of abar_l[edge] * best_l[s]      the weight of the heaviest (l + 1)-edge path to t
        pred_l[t]     = the edge id that attains it (the lowest among equals), -1 where t is not reachable
    with abar the mean of the four heads (head=-1) or one head.  The softmax runs over the out-edges of a source, so every flow_l sums
    to 1 over a subgraph.
  * `edges=True` also returns every layer's attention in the reference's own `(edge_index, alpha)` format -- what
    `GATConvE.forward(return_attention_weights=True)` returns: the caller's edges first, then one self loop per node row.

Off the GPU, or with a kernel provider that lacks the two kernels, the same results come from stock torch ops in fp32 (`trace_torch`,
`export_torch`)."""
import torch

from . import ops

BIG = 2 ** 62


class Trace:
    """What trace() returns.  B = all subgraphs of the batch (questions x choices), n node slots each, k layers.
    logits, pool_attn: the forward's outputs;  flow, best [k + 1, B, n] fp32;  pred [k, B, n] int32 edge ids (caller order; E + v is the
    self loop of node row v), pred_src [k, B, n] the source SLOT of that edge (-1 where pred is -1);  concept_ids, node_type_ids [B, n],
    adj_lengths [B];  with edges=True edge_index [2, E + N], alpha [k, E + N, 4], edge_type [E], else None."""
    __slots__ = ('logits', 'pool_attn', 'flow', 'best', 'pred', 'pred_src', 'concept_ids', 'node_type_ids', 'adj_lengths', 'edge_index',
                 'alpha', 'edge_type')

    def __init__(self, **kw):
        for name in self.__slots__:
            setattr(self, name, kw.get(name))

    def path(self, b, node, layer=None):
        """The heaviest `layer`-edge path from the context node to node slot `node` of subgraph b, backtracked through pred: the list of
        (edge id, source slot, target slot) from the context node outwards; [] where the node is not reachable in `layer` hops."""
        pred, src = self.pred.cpu(), self.pred_src.cpu()
        layer = pred.size(0) if layer is None else int(layer)
        assert 0 <= layer <= pred.size(0)
        out, t = [], int(node)
        for l in range(layer - 1, -1, -1):
            e, s = int(pred[l, b, t]), int(src[l, b, t])
            if e < 0:
                return []
            out.append((e, s, t))
            t = s
        return out[::-1]

    def top_nodes(self, b, m, layer=None):
        """The m node slots of subgraph b that hold most of the context node's attention mass after `layer` hops, heaviest first (the
        lower slot among equals): the list of (slot, concept id, flow)."""
        flow = self.flow.cpu()
        layer = flow.size(0) - 1 if layer is None else int(layer)
        f = flow[layer, b]
        order = torch.sort(f, descending=True, stable=True).indices[:int(m)].tolist()
        cids = self.concept_ids.cpu()[b]
        return [(j, int(cids[j]), float(f[j])) for j in order]


# -- the graph's arrays, whichever provider built it -------------------------------------------------------------------------------------
def _garr(graph, name, length):
    return graph.array(name, length) if hasattr(graph, 'array') else getattr(graph, name)[:length]


def _live(graph):
    """-> (cnt: the live positions rowptr_s[N] as a one-element int64 tensor, pos [Ep], live [Ep] bool)"""
    cnt = _garr(graph, 'rowptr_s', graph.N + 1)[graph.N:].long()
    pos = torch.arange(graph.Ep, device=cnt.device)
    return cnt, pos, pos < cnt


def _by_edge_id(graph, values, pos, live):
    """values [Ep, ...] in source order -> the same rows by edge id.  Positions behind the live ones (a graph with an edge capacity) hold no
    edge: they keep their own index, which lies behind every live id, so the scatter stays a permutation without a look at the count."""
    eid = torch.where(live, _garr(graph, 'eid_s', graph.Ep).long(), pos)
    out = torch.empty_like(values)
    out[eid] = values
    return out


def head_mean(a, head):
    """[..., 4] -> [...]: the mean of the four heads as the kernel adds them, ((a0 + a1) + (a2 + a3)) / 4, or one head"""
    return ((a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])) * 0.25 if head < 0 else a[..., head]


def export_torch(graph, a):
    """Kernels.attn_export with stock torch ops: alpha[l][eid_s[p]] = a[l][p]"""
    _, pos, live = _live(graph)
    return _by_edge_id(graph, a.transpose(0, 1), pos, live).transpose(0, 1).contiguous() if a.size(0) else a.clone()


def trace_torch(graph, a, B, n, root=0, head=-1):
    """Kernels.attn_trace with stock torch ops, in the dtype of a (fp32 in use): the definitions of include/qagnn_hip_explain.h, one
    index_add / scatter_reduce per layer.  -> (flow [k + 1, N], best [k + 1, N], pred [k, N] int32)"""
    N, Ep, k, dev = graph.N, graph.Ep, a.size(0), a.device
    assert N == B * n and 1 <= n and 0 <= root < n and -1 <= head <= 3
    _, pos, live = _live(graph)
    tgt = torch.where(live, _garr(graph, 'tgt_t', Ep).long(), pos.clamp(max=N - 1)).clamp(0, N - 1)
    base = tgt // n * n
    src = base + (_garr(graph, 'src_t', Ep).long() - base).clamp(0, n - 1)  # (a source outside the block: clamped into it, as in the kernel)
    p_t = torch.where(live, _garr(graph, 'pos_t', Ep).long(), pos).clamp(0, Ep - 1)
    eid_t = _garr(graph, 'eid_s', Ep).long()[p_t]
    zero = torch.zeros((), dtype=a.dtype, device=dev)
    flow = torch.zeros((k + 1, N), dtype=a.dtype, device=dev)
    flow[0, root::n] = 1
    best = flow.clone()
    pred = torch.full((k, N), -1, dtype=torch.int32, device=dev)
    for l in range(k):
        ab = head_mean(a[l], head)[p_t]
        flow[l + 1].index_add_(0, tgt, torch.where(live, ab * flow[l][src], zero))
        c = ab * best[l][src]
        c = torch.where(live & (c > 0), c, zero)  # (a NaN or non-positive candidate never beats the running maximum, which starts at 0)
        best[l + 1] = torch.zeros(N, dtype=a.dtype, device=dev).scatter_reduce(0, tgt, c, 'amax', include_self=True)
        first = torch.full((N,), BIG, dtype=torch.long, device=dev).scatter_reduce(
            0, tgt, torch.where((c > 0) & (c == best[l + 1][tgt]), pos, torch.full_like(pos, BIG)), 'amin', include_self=True)
        pred[l] = torch.where(first < BIG, eid_t[first.clamp(max=Ep - 1)], torch.full_like(first, -1)).int()
    return flow, best, pred


# -- one traced forward ---------------------------------------------------------------------------------------------------------------------
def _forward(model, inputs):
    """-> (logits, pool_attn, concept_ids [B, n], node_type_ids [B, n], adj_lengths [B]) of an LM_QAGNN (nested inputs) or a QAGNN (flat)"""
    if hasattr(model, 'decoder'):
        logits, attn, cids, nt = model(*inputs, detail=True)[:4]
        return logits, attn, cids.reshape(-1, cids.size(-1)), nt.reshape(-1, nt.size(-1)), inputs[-3].reshape(-1)
    logits, attn = model(*inputs)
    cids, nt, _, al = inputs[1:5]
    if cids is None and nt is None:
        cids, nt, _, al = inputs[5].fields()  # (a StoreBatch: the batch's own rows of the device store)
    return logits, attn, cids, nt, al


def _block_flag(graph, device):
    """one int64 word: the graph's device flag err[1] (some edge leaves its subgraph's block of node rows), 0 for a provider without flags"""
    return graph.array('err', 4)[1:2].long() if hasattr(graph, 'array') else torch.zeros(1, dtype=torch.long, device=device)


def check_block_flag(word):
    if word:
        raise RuntimeError('attention trace: an edge of this batch leaves its subgraph\'s block of node rows (its source was clamped into the '
                           'block): the traced values of that subgraph mean nothing')


def trace_nosync(model, inputs, head=-1, edges=False):
    """trace() without its synchronisation: -> (Trace, words), words a small int64 device tensor [block flag, live positions] the caller
    reads when it next synchronises (check_block_flag(words[0])).  With edges=True the edge tensors are still laid out for the graph's
    edge capacity: trace() cuts them to words[1] rows."""
    K = ops.kernels()
    with ops.inference_path(), ops.attention_capture() as cap:
        logits, pool_attn, cids, nt, al = _forward(model, inputs)
    graph, a = cap.graph, cap.a
    assert graph is not None, 'the forward ran no QAGNN_Message_Passing'
    n = nt.size(-1)
    B = graph.N // n
    native = a.is_cuda and hasattr(K, 'attn_trace') and hasattr(K, 'attn_export')
    flow, best, pred = (K.attn_trace if native else trace_torch)(graph, a, B, n, 0, head)
    k = a.size(0)
    cnt, pos, live = _live(graph)
    src_by_id = _by_edge_id(graph, _garr(graph, 'src_s', graph.Ep).long(), pos, live)
    pl = pred.long()
    pred_src = torch.where(pl >= 0, src_by_id[pl.clamp(min=0)] % n, pl)
    rec = Trace(logits=logits, pool_attn=pool_attn, flow=flow.view(k + 1, B, n), best=best.view(k + 1, B, n), pred=pred.view(k, B, n),
                pred_src=pred_src.view(k, B, n), concept_ids=cids, node_type_ids=nt, adj_lengths=al)
    if edges:
        rec.alpha = K.attn_export(graph, a) if native else export_torch(graph, a)
        tgt_by_id = _by_edge_id(graph, _garr(graph, 'tgt_s', graph.Ep).long(), pos, live)
        rec.edge_index = torch.stack([src_by_id, tgt_by_id])
        rec.edge_type = _by_edge_id(graph, _garr(graph, 'cls_s', graph.Ep).long(), pos, live) // (graph.T * graph.T)
    return rec, torch.cat([_block_flag(graph, cnt.device), cnt])


def trace(model, *inputs, head=-1, edges=False):
    """One eval forward of `model` -- an LM_QAGNN (the nested inputs of its forward, any graph holder) or a QAGNN decoder (flat inputs) --
    with the attention of its k hops traced from the context node: -> Trace.  head: -1 the mean of the four attention heads, or one head.
    Call it in eval mode under torch.no_grad() (anything else is refused).  One host synchronisation, behind the kernels."""
    rec, words = trace_nosync(model, inputs, head, edges)
    flag, cnt = words.tolist()
    check_block_flag(flag)
    if edges:
        N = rec.flow.size(1) * rec.flow.size(2)
        rec.alpha, rec.edge_index, rec.edge_type = rec.alpha[:, :cnt], rec.edge_index[:, :cnt], rec.edge_type[:cnt - N]
    return rec
