"""Float64 numpy twin of the attention trace (include/qagnn_hip_explain.h).  TEST INFRASTRUCTURE ONLY.

Written from the header's definitions, one node at a time, with none of the package's code: the expected value of the torch fallback
(`-m "not gpu"`) and of qagnn_attn_trace_f32 (`-m gpu`) on the SAME attention values.  The head mean is taken exactly (float64 sums of
four fp32 numbers are exact), so the twin is exact arithmetic on `a` up to float64 rounding, 2^-29 of the fp32 unit."""
import numpy as np

U = 2.0 ** -24  # the fp32 unit roundoff


def graph_arrays(graph):
    """the arrays of a prepared graph (a HipGraph or the emulation's), cut to the live positions, as int64 numpy"""
    def arr(name, length):
        t = graph.array(name, length) if hasattr(graph, 'array') else getattr(graph, name)[:length]
        return t.cpu().numpy().astype(np.int64)
    N = graph.N
    rowptr_s = arr('rowptr_s', N + 1)
    cnt = int(rowptr_s[N])
    g = dict(N=N, cnt=cnt, rowptr_s=rowptr_s, rowptr_t=arr('rowptr_t', N + 1))
    for name in ('eid_s', 'src_s', 'tgt_s', 'src_t', 'pos_t'):
        g[name] = arr(name, cnt)
    return g


def head_mean(a, head):
    a = np.asarray(a, dtype=np.float64)
    return a.sum(-1) / 4.0 if head < 0 else a[..., head]


def trace(g, a, n, root=0, head=-1):
    """g: graph_arrays(); a [k, >= cnt, 4].  -> dict(flow [k+1, N], best [k+1, N], pred [k, N], second [k, N], m)
    second: the largest candidate of a node other than its winning edge (0 where there is none); m: the largest in-degree."""
    N, rp, src_t, pos_t, eid_s = g['N'], g['rowptr_t'], g['src_t'], g['pos_t'], g['eid_s']
    k = len(a)
    flow = np.zeros((k + 1, N))
    best = np.zeros((k + 1, N))
    pred = np.full((k, N), -1, dtype=np.int64)
    second = np.zeros((k, N))
    flow[0, root::n] = 1.0
    best[0, root::n] = 1.0
    for l in range(k):
        ab = head_mean(a[l], head)
        for t in range(N):
            lo, hi = rp[t], rp[t + 1]
            w = ab[pos_t[lo:hi]]
            s = src_t[lo:hi]
            flow[l + 1, t] = np.sum(w * flow[l, s])
            run, win = 0.0, -1
            c = w * best[l, s]
            for i in range(hi - lo):
                if c[i] > run:  # (strict: the earlier edge among equals; False for a NaN)
                    run, win = c[i], i
            best[l + 1, t] = run
            if win >= 0:
                pred[l, t] = eid_s[pos_t[lo + win]]
                rest = np.delete(c, win)
                rest = rest[rest == rest]
                second[l, t] = max(rest.max(), 0.0) if rest.size else 0.0
    return dict(flow=flow, best=best, pred=pred, second=second, m=int(np.max(rp[1:] - rp[:-1])))


def bounds(k, m):
    """(flow, best): the relative error bounds of the header over k layers"""
    return k * (m + 6) * U, 6 * k * U


def walks(g, a, n, root, head, b=0):
    """Brute force for ONE subgraph b of a small graph: every walk of 1..k edges from the root, by edge id.
    -> {length: {end node: [(product, [edge ids])]}}"""
    k = len(a)
    src = np.empty(g['cnt'], dtype=np.int64)
    tgt = np.empty(g['cnt'], dtype=np.int64)
    w = np.empty((k, g['cnt']))
    src[g['eid_s']], tgt[g['eid_s']] = g['src_s'], g['tgt_s']
    for l in range(k):
        w[l, g['eid_s']] = head_mean(a[l], head)[:g['cnt']]
    out = {}
    front = [(b * n + root, 1.0, [])]
    for l in range(k):
        nxt = []
        for node, prod, path in front:
            for e in np.nonzero(src == node)[0]:
                nxt.append((int(tgt[e]), prod * w[l, e], path + [int(e)]))
        front = nxt
        ends = {}
        for node, prod, path in front:
            ends.setdefault(node, []).append((prod, path))
        out[l + 1] = ends
    return out
