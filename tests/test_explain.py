"""Detailed evaluation (include/qagnn_hip_explain.h, qagnn_amd/explain.py, inference.evaluate_detail): per-layer attention in the
reference's format and its trace out of the context node.

Without a GPU: the header and the binding; the float64 twin (tests/explain_twin.py) against brute-force walk enumeration; the stock-torch
fallback against the twin within the header's bounds; mass conservation; the module on the emulation provider against the float64 oracle;
the record's helpers; evaluate_detail on a stub model.  `-m gpu`: the two kernels against the twin ON THE SAME attention values, and the
module against the oracle and the twin.

Bounds: those of the header -- flow k (m + 6) 2^-24, best 6 k 2^-24, relative, m the largest in-degree.  The twin's own float64 error
(2^-53 per operation) is 2^-29 of them."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import emu_kernels
import explain_twin as TW
import helpers
from emu_explain import EmuExplainKernels
from emu_infer import EmuInferKernels
from qagnn_amd import _lib, data_utils, explain, inference, ops
from qagnn_amd import modeling_qagnn as MQ

U = TW.U
LOG = os.environ.get('QAGNN_EXPLAIN_TEST_LOG')  # file that collects the measured figures of the GPU tests
R_, T_ = 5, 4  # relation and node-type counts of the synthetic graphs

# Deeper layers' attention against the float64 oracle (layer 0 stands at the existing layer_alpha bar, rtol 1e-4 / atol 1e-7): layer l reads
# node features that went through l hops in fp32, so its softmax inherits their forward deviation.  Measured on the GPU over the cases of
# test_module_against_oracle_and_twin (profiles/explain_gpu_tests.txt): worst 5.92e-5 relative beyond atol (layer 2 of the 41 x 200 batch;
# nothing beyond atol at 4 x 16, nor on the CPU emulation); the bar is twice that.
DEEP_ALPHA_RTOL = 1.2e-4
ALPHA_ATOL = 1e-7


def note(line):
    print(line)
    if LOG:
        with open(LOG, 'a') as f:
            f.write(line + '\n')


@contextlib.contextmanager
def provider(K):
    old = ops.set_kernels(K)
    try:
        yield K
    finally:
        ops.set_kernels(old)


def hip():
    ops.set_kernels(None)
    return ops.kernels()


# =================================================================================================================================
# graphs and attention values
# =================================================================================================================================
def make_graph(B, n, seed, e_rand=None, hub_deg=0, hub_root=False, pad=None, star=True):
    """B subgraphs of n node slots; slot 0 is the context node.  The last `pad` slots keep only their self loop (PAD slots); e_rand random
    edges among the others, drawn with replacement (parallel edges, explicit self loops); star: the context node's edges to and from a
    third of the slots; one hub target -- slot 0 (hub_root) or the last real slot -- brought to in-degree hub_deg, self loop included.
    -> (edge_index [2, E], edge_type [E], node_type [B * n])"""
    g = torch.Generator().manual_seed(seed)
    pad = (n // 4 if n >= 8 else 0) if pad is None else pad
    real = n - pad
    e_rand = 4 * real if e_rand is None else e_rand
    src, tgt = [], []
    for b in range(B):
        s = torch.randint(0, real, (e_rand,), generator=g)
        t = torch.randint(0, real, (e_rand,), generator=g)
        if star and real > 1:
            out = torch.nonzero(torch.rand(real - 1, generator=g) < 0.34).flatten() + 1
            s = torch.cat([s, torch.zeros_like(out), out])
            t = torch.cat([t, out, torch.zeros_like(out)])
        if hub_deg > 1:
            hub = 0 if hub_root else real - 1
            have = int((t == hub).sum()) + 1
            more = max(hub_deg - have, 0)
            s = torch.cat([s, torch.randint(0, real, (more,), generator=g)])
            t = torch.cat([t, torch.full((more,), hub, dtype=torch.long)])
            if have > hub_deg:  # drop the surplus
                drop = torch.nonzero(t == hub).flatten()[:have - hub_deg]
                keep = torch.ones_like(t, dtype=torch.bool)
                keep[drop] = False
                s, t = s[keep], t[keep]
        perm = torch.randperm(s.numel(), generator=g)
        src.append(s[perm] + b * n)
        tgt.append(t[perm] + b * n)
    ei = torch.stack([torch.cat(src), torch.cat(tgt)]) if src else torch.zeros((2, 0), dtype=torch.long)
    et = torch.randint(0, R_, (ei.size(1),), generator=g)
    nt = torch.randint(0, T_, (B * n,), generator=g)
    nt[::n] = 3
    return ei, et, nt


def softmax_a(g, k, seed, scale=2.0):
    """a [k, cnt, 4] fp32: a true per-source softmax of random scores, in source order (g: TW.graph_arrays)"""
    rng = np.random.default_rng(seed)
    sc = rng.normal(size=(k, g['cnt'], 4)) * scale
    seg = np.repeat(np.arange(g['N']), np.diff(g['rowptr_s']))
    a = np.empty_like(sc)
    for l in range(k):
        m = np.full((g['N'], 4), -np.inf)
        np.maximum.at(m, seg, sc[l])
        e = np.exp(sc[l] - m[seg])
        s = np.zeros((g['N'], 4))
        np.add.at(s, seg, e)
        a[l] = e / (s[seg] + 1e-16)
    return torch.from_numpy(a.astype(np.float32))


def emu_graph(ei, et, nt, n):
    return emu_kernels.EmuGraph(ei, et, nt, R_, T_, block_n=n)


def check_trace(got, tw, k, what, a=None, g=None, n=None, head=-1, cap=0.01):
    """got = (flow, best, pred) as float64 / int64 numpy against the twin's dict: the header's bounds; pred self-consistent, -1 exactly where
    best is 0, equal to the twin's outside the near-ties, whose share of the reachable nodes stays under `cap`"""
    flow, best, pred = got
    bf, bb = TW.bounds(max(k, 1), tw['m'])
    tiny = 2.0 ** -149 * k * (tw['m'] + 6)
    for name, x, ref, bound in (('flow', flow, tw['flow'], bf), ('best', best, tw['best'], bb)):
        fin = ref == ref
        assert np.array_equal(np.isnan(x), ~fin), f'{what}: {name} is NaN elsewhere than the twin'
        big = fin & (ref >= 1e-30)
        rel = np.abs(x[big] - ref[big]) / ref[big]
        worst = rel.max() if rel.size else 0.0
        print(f'FIGURE {what}: {name} worst relative error {worst:.3e} (bound {bound:.3e})')
        assert worst <= bound * (1 + 1e-6), f'{what}: {name} relative error {worst:.3e} above {bound:.3e}'
        small = fin & ~big
        assert np.all(np.abs(x[small] - ref[small]) <= bound * 1e-30 + tiny), f'{what}: {name} below 1e-30'
    assert np.array_equal(pred == -1, best[1:] == 0), f'{what}: pred is -1 exactly where best is 0'
    if a is not None and k:
        # (i) pred against the candidate's OWN best: abar[pred] * best_l[src(pred)] is best_{l+1}[t] within one layer's share of the bound
        inv = np.empty(g['cnt'], dtype=np.int64)
        inv[g['eid_s']] = np.arange(g['cnt'])
        for l in range(k):
            t = np.nonzero(pred[l] >= 0)[0]
            p = inv[pred[l, t]]
            assert np.array_equal(g['tgt_s'][p], t), f'{what}: pred names an edge into another node'
            c = TW.head_mean(a[l], head)[p] * best[l, g['src_s'][p]]
            assert np.all(np.abs(c - best[l + 1, t]) <= 6 * U * best[l + 1, t] + 2.0 ** -149), f'{what}: layer {l} pred is not the winner'
    reach = tw['pred'] >= 0
    clear = reach & (tw['second'] < tw['best'][1:] * (1 - 64 * U))
    assert np.array_equal(pred[clear], tw['pred'][clear]), f'{what}: pred differs from the twin outside the near-ties'
    exempt, total = int((reach & ~clear).sum()), int(reach.sum())
    assert exempt <= cap * total, f'{what}: {exempt} of {total} reachable nodes are near-ties of the twin: pick another seed'
    return exempt, total


def f64(*ts):
    return tuple(t.detach().cpu().numpy().astype(np.int64 if t.dtype in (torch.int32, torch.long) else np.float64) for t in ts)


# =================================================================================================================================
# Without a GPU
# =================================================================================================================================
def test_explain_header_bindings_and_build_hash():
    """qagnn_hip_explain.h declares exactly EXPORTS_EXPLAIN; the built library exports them; the version is 1; the build hash covers the
    header and explain.hip; ABI 25 and the four existing lists are where they were; no name is in two lists."""
    from qagnn_amd import build as B
    hdr = open(os.path.join(helpers.ROOT, 'include', 'qagnn_hip_explain.h')).read()
    declared = sorted(set(re.findall(r'^int (qagnn_[a-z0-9_]+)\(', hdr, flags=re.M)))
    assert declared == sorted(_lib.EXPORTS_EXPLAIN) and len(declared) == 3
    B.build(verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f'{name} declared in qagnn_hip_explain.h but not exported'
    lib = _lib.load_library()  # prototypes resolve
    assert lib.qagnn_explain_version() == 1
    hashed = {os.path.realpath(p) for p in B.hashed_files()}
    assert os.path.realpath(os.path.join(helpers.ROOT, 'include', 'qagnn_hip_explain.h')) in hashed
    assert os.path.realpath(os.path.join(B.CSRC, 'explain.hip')) in hashed and 'explain.hip' in B.SOURCES
    assert _lib.ABI_VERSION == 25 and len(_lib.EXPORTS) == 63 and len(_lib.EXPORTS_TN) == 4 and len(_lib.EXPORTS_INFER) == 5 and len(_lib.EXPORTS_LOSS) == 3
    lists = [_lib.EXPORTS, _lib.EXPORTS_TN, _lib.EXPORTS_INFER, _lib.EXPORTS_LOSS, _lib.EXPORTS_EXPLAIN]
    assert sum(len(set(e)) for e in lists) == len(set().union(*lists))
    assert [str(_lib.TRACE_MAX_N)] == re.findall(r'#define QAGNN_TRACE_MAX_N (\d+)', hdr)


@pytest.mark.parametrize('seed,head', [(0, -1), (1, 2), (2, -1)])
def test_twin_against_brute_force(seed, head):
    """n = 5, k = 3, parallel edges and explicit self loops: flow is the sum of the walk products over every walk from the root, best their
    maximum, and backtracking pred reproduces a walk that attains it."""
    B, n, k = 2, 5, 3
    ei, et, nt = make_graph(B, n, seed, e_rand=9, pad=1, star=False)
    assert (ei[0] == ei[1]).any() and len({(int(s), int(t)) for s, t in ei.t()}) < ei.size(1), 'want explicit self loops and parallel edges'
    g = TW.graph_arrays(emu_graph(ei, et, nt, n))
    a = softmax_a(g, k, seed).numpy()
    tw = TW.trace(g, a, n, root=0, head=head)
    src = np.empty(g['cnt'], dtype=np.int64)
    src[g['eid_s']] = g['src_s']
    for b in range(B):
        W = TW.walks(g, a, n, 0, head, b)
        for l in range(1, k + 1):
            for t in range(b * n, (b + 1) * n):
                ws = W[l].get(t, [])
                total, top = sum(p for p, _ in ws), max([p for p, _ in ws], default=0.0)
                assert abs(tw['flow'][l, t] - total) <= 1e-12 * max(total, 1e-300) + 1e-300
                assert abs(tw['best'][l, t] - top) <= 1e-12 * top
                assert (tw['pred'][l - 1, t] == -1) == (top == 0)
                if top > 0:  # backtrack
                    path, node = [], t
                    for ll in range(l - 1, -1, -1):
                        e = tw['pred'][ll, node]
                        path.append(int(e))
                        node = src[e]
                    assert node == b * n
                    prods = [p for p, w in ws if w == path[::-1]]
                    assert len(prods) == 1 and abs(prods[0] - top) <= 1e-12 * top


FALLBACK_CASES = [(1, 1, 1, -1), (2, 2, 3, -1), (3, 65, 5, 2), (2, 200, 5, -1)]


@pytest.mark.parametrize('B,n,k,head', FALLBACK_CASES)
def test_torch_fallback_against_twin(B, n, k, head):
    ei, et, nt = make_graph(B, n, 100 + n, hub_deg=min(70, 2 * n), hub_root=n % 2 == 0)
    G = emu_graph(ei, et, nt, n)
    g = TW.graph_arrays(G)
    a = softmax_a(g, k, 7 + n)
    got = f64(*explain.trace_torch(G, a, B, n, 0, head))
    check_trace(got, TW.trace(g, a.numpy(), n, 0, head), k, f'fallback B={B} n={n} k={k}', a.numpy(), g, n, head)
    alpha = explain.export_torch(G, a)
    want = torch.empty_like(a)
    want[:, G.eid_s.long()] = a
    assert torch.equal(alpha, want)


def tie_case():
    """B = 1, n = 2: two parallel edges root -> 1 (edge ids 0 and 1) at exactly 0.5 in every head, the self loops at 0.25"""
    ei = torch.tensor([[0, 0], [1, 1]])
    et, nt = torch.zeros(2, dtype=torch.long), torch.tensor([3, 0])
    return ei, et, nt


def tie_a(g, k=1):
    a = torch.full((k, g['cnt'], 4), 0.25)
    for e in (0, 1):
        a[:, int(np.nonzero(g['eid_s'] == e)[0][0])] = 0.5
    return a


def test_torch_fallback_ties_and_nan():
    """two equal candidates: the lower edge id.  A NaN candidate never wins and leaves best finite; in flow it propagates, inside its own
    subgraph only."""
    ei, et, nt = tie_case()
    G = emu_graph(ei, et, nt, 2)
    g = TW.graph_arrays(G)
    a = tie_a(g)
    flow, best, pred = explain.trace_torch(G, a, 1, 2)
    tw = TW.trace(g, a.numpy(), 2)
    assert pred[0].tolist() == [2, 0] == tw['pred'][0].tolist() and best[1].tolist() == [0.25, 0.5] and flow[1].tolist() == [0.25, 1.0]
    B, n, k = 3, 9, 3
    ei, et, nt = make_graph(B, n, 5)
    G = emu_graph(ei, et, nt, n)
    g = TW.graph_arrays(G)
    a = softmax_a(g, k, 3)
    clean = explain.trace_torch(G, a, B, n)
    p = int(g['rowptr_s'][n])  # the first out-edge of subgraph 1's context node
    a[0, p, 1] = float('nan')
    got = f64(*explain.trace_torch(G, a, B, n))
    tw = TW.trace(g, a.numpy(), n)
    assert np.isnan(tw['flow'][:, n:2 * n]).any() and not np.isnan(tw['best']).any()
    check_trace(got, tw, k, 'fallback NaN')
    for x, c in zip(got, f64(*clean)):
        for b in (0, 2):
            assert np.array_equal(x[:, b * n:(b + 1) * n], c[:, b * n:(b + 1) * n])


@pytest.mark.parametrize('B,n,E,hub', [(6, 200, 1000, 0), (4, 200, 1500, 150), (8, 64, 300, 0)])
def test_mass_is_conserved(B, n, E, hub):
    """a true per-source softmax moves the context node's unit of mass and loses none: |sum_t flow_l - 1| per subgraph within the flow bound
    + 1e-6 (fp32 a, the softmax's 1e-16)"""
    k = 5
    ei, et, nt = make_graph(B, n, 0, e_rand=E, hub_deg=hub)
    G = emu_graph(ei, et, nt, n)
    g = TW.graph_arrays(G)
    a = softmax_a(g, k, 0)
    flow = explain.trace_torch(G, a, B, n)[0].double().view(k + 1, B, n)
    m = int(np.diff(g['rowptr_t']).max())
    dev = (flow.sum(2) - 1).abs().max().item()
    print(f'FIGURE mass B={B} n={n} E={E}: worst |sum flow - 1| = {dev:.2e}')
    assert dev <= TW.bounds(k, m)[0] + 1e-6


def small_case(nq=4, n=16, shape='tiny', k=3, seed=31):
    return dict(shape=shape, nq=nq, nc=1, n=n, n_rel=17, std=0.8, train=False, seed=seed,
                cfg=helpers.model_cfg(d=32, k=k, sent_dim=24, n_concept=300, concept_in_dim=16))


def build_model(case):
    cfg = case['cfg']
    torch.manual_seed(0)
    model = MQ.QAGNN(None, cfg['k'], cfg['n_ntype'], cfg['n_etype'], cfg['sent_dim'], cfg['n_concept'], cfg['concept_dim'],
                     cfg['concept_in_dim'], cfg['n_attention_head'], cfg['fc_dim'], cfg['n_fc_layer'], cfg['p_emb'], cfg['p_gnn'], cfg['p_fc'],
                     pretrained_concept_emb=None, freeze_ent_emb=True, init_range=cfg['init_range'])
    helpers.det_fill_(model, case['seed'], case['std'])
    model.pooler.dropout.p = model.pooler.attention.dropout.p = 0.0
    return model.eval()


def case_args(case):
    inp = helpers.make_case_inputs(case)
    B, n = case['nq'] * case['nc'], case['n']
    return [inp['sent_vecs'], inp['concept_ids'].view(B, n), inp['node_type_ids'].view(B, n), inp['node_scores'].view(B, n, 1),
            inp['adj_lengths'].view(B), inp['edge_index'], inp['edge_type']]


_ORACLE = {}


def oracle_alpha(case, args, monkeypatch):
    """per-layer attention of the float64 oracle in the reference's format ([E + N, 4] per layer, the caller's edges, then the self loops),
    recorded at its segment_softmax; computed once per case"""
    key = (case['nq'], case['n'], case['shape'], case['cfg']['k'])
    if key not in _ORACLE:
        from oracle import qagnn_oracle as O
        rec, inner = [], O.segment_softmax

        def spy(src, index, num_groups):
            out = inner(src, index, num_groups)
            rec.append(out.detach().clone())
            return out
        monkeypatch.setattr(O, 'segment_softmax', spy)
        model = helpers.build_oracle(case).double()
        torch.set_default_dtype(torch.float64)
        O.PIN_FP32_SCORES = True
        try:
            sv, cids, nt, ns, al, ei, et = args
            with torch.no_grad():
                model(sv.double(), cids, nt, ns.double(), al, (ei, et))
        finally:
            torch.set_default_dtype(torch.float32)
            O.PIN_FP32_SCORES = False
            monkeypatch.undo()
        assert len(rec) == case['cfg']['k']
        _ORACLE[key] = torch.stack(rec) if rec else torch.zeros((0, ei.size(1) + nt.numel(), 4), dtype=torch.float64)
    return _ORACLE[key]


def check_alpha(alpha, ref, what):
    """layer 0 at the layer_alpha bar of tests/test_hip_parity.py, deeper layers at DEEP_ALPHA_RTOL; -> the measured worst of the deeper ones"""
    alpha = alpha.detach().cpu().double()
    assert alpha.shape == ref.shape, (alpha.shape, ref.shape)
    worst = 0.0
    for l in range(alpha.size(0)):
        err = (alpha[l] - ref[l]).abs()
        rel = ((err - ALPHA_ATOL).clamp(min=0) / ref[l].abs().clamp(min=1e-300)).max().item()
        note(f'FIGURE {what}: alpha layer {l} worst relative error beyond atol {rel:.3e}')
        assert rel <= (1e-4 if l == 0 else DEEP_ALPHA_RTOL), f'{what}: alpha of layer {l} is {rel:.3e} from the float64 oracle'
        worst = max(worst, rel if l else 0.0)
    return worst


def check_record_against_twin(rec, graph_of, k, what, head=-1):
    """flow / best / pred of a record against the twin on the record's OWN alpha (edges=True)"""
    B, n = rec.flow.shape[1:]
    ei, alpha = rec.edge_index.cpu(), rec.alpha.cpu()
    N = B * n
    E = ei.size(1) - N
    assert torch.equal(ei[:, E:], torch.arange(N).repeat(2, 1)) and rec.edge_type.shape == (E,)
    G = emu_kernels.EmuGraph(ei[:, :E], rec.edge_type.cpu(), rec.node_type_ids.cpu().reshape(-1), graph_of.R, graph_of.T, block_n=n)
    g = TW.graph_arrays(G)
    a = alpha[:, G.eid_s.long()].numpy()
    got = f64(rec.flow.reshape(k + 1, N), rec.best.reshape(k + 1, N), rec.pred.reshape(k, N))
    check_trace(got, TW.trace(g, a, n, 0, head), k, what, a, g, n, head)
    src = np.where(got[2] >= 0, ei[0].numpy()[np.maximum(got[2], 0)] % n, -1)
    assert np.array_equal(src, rec.pred_src.cpu().numpy().reshape(k, N))
    return ei[:, :E]


def test_module_on_the_emulation_against_the_oracle(monkeypatch):
    """explain.trace(edges=True) on the emulation provider: alpha against the float64 oracle's per-layer attention; the trace against the
    twin; the forward-only stack with an attention buffer per hop where the provider has it, the per-layer loop where it has not -- the
    same record either way, and the same logits as the plain inference-path forward."""
    case = small_case()
    args = case_args(case)
    flat = args[:5] + [(args[5], args[6])]
    ref = oracle_alpha(case, args, monkeypatch)
    recs = []
    for K, route in ((EmuExplainKernels(), ['stack_infer+attn']), (EmuInferKernels(), None)):
        with provider(K), torch.no_grad():
            model = build_model(case)
            rec = explain.trace(model, *flat, edges=True)
            with ops.inference_path():
                logits, attn = model(*flat)
            if route is not None:
                assert K.calls == route + ['stack_infer']
            assert ops.ATTN_CAPTURE is None and ops.INFERENCE_PATH is False
        assert torch.equal(rec.logits, logits) and torch.equal(rec.pool_attn, attn)
        assert torch.equal(rec.edge_index[:, :args[5].size(1)], args[5]) and torch.equal(rec.edge_type, args[6])
        check_alpha(rec.alpha, ref, 'emulation')
        check_record_against_twin(rec, ops_graph_dims(case), case['cfg']['k'], 'emulation module')
        recs.append(rec)
    for name in ('flow', 'best', 'pred', 'alpha'):
        assert torch.equal(getattr(recs[0], name), getattr(recs[1], name)), name
    # refused outside an evaluation forward
    with provider(EmuExplainKernels()):
        model = build_model(case)
        with pytest.raises(RuntimeError, match='torch.no_grad'):
            explain.trace(model, *flat)
        with torch.no_grad(), pytest.raises(RuntimeError, match='model.eval'):
            explain.trace(model.train(), *flat)


def test_module_without_hops_on_the_emulation():
    """k = 0: layer 0 only -- the unit of mass on the context node, no pred, an empty alpha over the right edge list"""
    case = small_case(k=0)
    args = case_args(case)
    flat = args[:5] + [(args[5], args[6])]
    B, n = case['nq'], case['n']
    with provider(EmuExplainKernels()), torch.no_grad():
        model = build_model(case)
        rec = explain.trace(model, *flat, edges=True)
        with ops.inference_path():
            logits, _ = model(*flat)
    assert torch.equal(rec.logits, logits) and rec.flow.shape == (1, B, n) and rec.pred.shape == (0, B, n)
    assert rec.alpha.shape == (0, args[5].size(1) + B * n, 4) and torch.equal(rec.edge_index[:, :args[5].size(1)], args[5])
    assert rec.flow[0, :, 0].tolist() == [1.0] * B and float(rec.flow.sum()) == B and rec.path(0, 0) == [] and rec.top_nodes(1, 1)[0][0] == 0


class _Dims:
    def __init__(self, R, T):
        self.R, self.T = R, T


def ops_graph_dims(case):
    return _Dims(case['cfg']['n_etype'], case['cfg']['n_ntype'])


def test_path_and_top_nodes_on_a_hand_written_record():
    """B = 1, n = 4, k = 2: 0 -> 1 (edge 0), 0 -> 2 (edge 1), 1 -> 3 (edge 2), self loops 3 + v"""
    pred = torch.tensor([[[3, 0, 1, -1]], [[3, 0, 1, 2]]], dtype=torch.int32)
    src = torch.tensor([[[0, 0, 0, -1]], [[0, 0, 0, 1]]])
    flow = torch.tensor([[[1, 0, 0, 0]], [[0.5, 0.3, 0.2, 0]], [[0.25, 0.25, 0.25, 0.25]]])
    rec = explain.Trace(pred=pred, pred_src=src, flow=flow, best=flow.clone(), concept_ids=torch.tensor([[7, 11, 13, 17]]))
    assert rec.path(0, 3) == [(0, 0, 1), (2, 1, 3)]
    assert rec.path(0, 3, layer=1) == [] and rec.path(0, 2, layer=1) == [(1, 0, 2)] and rec.path(0, 0, layer=0) == []
    assert rec.path(0, 0) == [(3, 0, 0), (3, 0, 0)]
    assert rec.top_nodes(0, 2, layer=1) == [(0, 7, 0.5), (1, 11, pytest.approx(0.3))]
    assert [s for s, _, _ in rec.top_nodes(0, 3)] == [0, 1, 2]  # equal flow: the lower slot first
    assert not hasattr(rec, '__dict__') and rec.alpha is None and rec.edge_index is None


def test_trace_and_evaluate_detail_through_lm_qagnn_on_the_emulation(tmp_path):
    """an LM_QAGNN with the nested inputs of its forward: the record is the decoder's on the flattened batch; evaluate_detail with
    trace=True returns one record per batch and the argmax of the model's logits"""
    from test_oracle_golden import golden_inputs
    case = 'small_train'
    c, fix = helpers.GOLDEN_CASES[case], helpers.load_golden(case)
    cfg, nq, nc, n = c['cfg'], c['nq'], c['nc'], c['n']
    with provider(EmuExplainKernels()):
        torch.manual_seed(0)
        model = MQ.LM_QAGNN(None, 'stub', cfg['k'], cfg['n_ntype'], cfg['n_etype'], cfg['n_concept'], cfg['concept_dim'], cfg['concept_in_dim'],
                            cfg['n_attention_head'], cfg['fc_dim'], cfg['n_fc_layer'], 0.0, 0.0, 0.0, init_range=0.02,
                            encoder=helpers.StubTextEncoder(sent_dim=cfg['sent_dim'], in_dim=helpers.LM_CASES[case]['in_dim'])).eval()
        helpers.det_fill_(model, 5, 0.8)
        _, cids, nt, ns, al, ei, et = golden_inputs(case, fix)
        nei, net = helpers.nested_graph_lists(case, fix)
        inp = [helpers.lm_inputs(case), cids.view(nq, nc, n), nt.view(nq, nc, n), ns.view(nq, nc, n, 1), al.view(nq, nc), nei, net]
        with torch.no_grad():
            rec = explain.trace(model, *inp, edges=True)
            sent = model.encoder(inp[0].reshape(nq * nc, -1))[0]
            dec = explain.trace(model.decoder, sent, cids, nt, ns, al, (ei, et), edges=True)
            logits = model(*inp)[0]
        assert rec.logits.shape == (nq, nc) and torch.equal(rec.logits.view(-1), dec.logits.view(-1)) and torch.equal(rec.logits, logits)
        for f in ('flow', 'best', 'pred', 'pred_src', 'alpha', 'edge_index', 'edge_type', 'concept_ids', 'node_type_ids', 'adj_lengths'):
            assert torch.equal(getattr(rec, f), getattr(dec, f)), f
        assert rec.flow.shape == (cfg['k'] + 1, nq * nc, n) and torch.equal(rec.edge_index[:, :ei.size(1)], ei)
        es = [([f'a{i}', f'b{i}'], torch.tensor([l0, l1]), *inp) for i, (l0, l1) in enumerate(((0, 1), (2, 2)))]
        acc, results, traces = inference.evaluate_detail(es, model, preds_path=str(tmp_path / 'p.csv'), trace=True)
        pred = logits.argmax(1).tolist()
        assert results == [('a0', pred[0]), ('b0', pred[1]), ('a1', pred[0]), ('b1', pred[1])] and len(traces) == 2 and traces[0].alpha is None
        assert acc == sum(int(p == l) for p, l in zip(pred * 2, (0, 1, 2, 2))) / 4 == inference.evaluate_accuracy(es, model)
        assert torch.equal(traces[1].flow, rec.flow) and torch.equal(traces[1].pred, rec.pred)
        assert (tmp_path / 'p.csv').read_text() == ''.join(f'{q},{"ABC"[p]}\n' for q, p in results)


class _StubModel(torch.nn.Module):
    """logits = the batch's own scores: a decoder-shaped model for the host logic of evaluate_detail"""

    def forward(self, scores):
        return scores.reshape(-1, 1), None


def _stub_set(sizes, nc, seed=0):
    g = torch.Generator().manual_seed(seed)
    out, q = [], 0
    for Q in sizes:
        scores = torch.randn(Q * nc, generator=g)
        labels = torch.randint(0, nc, (Q,), generator=g)
        out.append(([f'q{q + i}' for i in range(Q)], labels, scores))
        q += Q
    return out


def test_evaluate_detail_with_a_stub_model(tmp_path):
    nc = 5
    es = _stub_set([4, 4, 3], nc)
    path = tmp_path / 'preds.csv'
    with provider(EmuInferKernels()):
        model = _StubModel().train()
        acc, results, traces = inference.evaluate_detail(es, model, preds_path=str(path))
        assert not model.training and traces is None
        assert acc == inference.evaluate_accuracy(es, model)
        want = [(qid, int(s.view(-1, nc)[i].argmax())) for qids, _, s in es for i, qid in enumerate(qids)]
        assert results == want and len(want) == 11
        assert acc == sum(int(p == int(l)) for (_, p), l in zip(want, torch.cat([b[1] for b in es]))) / 11
        assert path.read_text() == ''.join(f'{qid},{"ABCDE"[p]}\n' for qid, p in want)
        with pytest.raises(ZeroDivisionError):
            inference.evaluate_detail([], model)


# =================================================================================================================================
# On the GPU
# =================================================================================================================================
def dev_graph(K, ei, et, nt, n, e_cap=None):
    if e_cap is None:
        return K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R_, T_, block_n=n)
    E = ei.size(1)
    b = data_utils.EdgeListBatch(torch.nn.functional.pad(ei, (0, e_cap - E)), torch.nn.functional.pad(et, (0, e_cap - E)), E, e_cap).to('cuda')
    return K.graph_prep_cap(b, nt.cuda(), R_, T_, block_n=n)


CANARY = 2.0 ** 100


@pytest.mark.gpu
@pytest.mark.parametrize('k', [1, 5])
@pytest.mark.parametrize('B,n,E', [(1, 1, 0), (3, 65, 100), (2, 200, 2000)])
@pytest.mark.parametrize('cap', [False, True])
def test_attn_export(B, n, E, k, cap):
    """bit-exact against alpha[eid_s] = a; with an edge capacity above the count the rows behind E + N of every layer keep their canary;
    a layer stride above 4 Ep with 2^100 in the gap, of which nothing reaches the output"""
    K = hip()
    ei, et, nt = make_graph(B, n, 11 + n, e_rand=E, star=False, pad=0)
    E = ei.size(1)
    G = dev_graph(K, ei, et, nt, n, e_cap=E + 37 if cap else None)
    g = TW.graph_arrays(G)
    cnt, Ep = g['cnt'], G.Ep
    assert cnt == E + B * n and Ep == cnt + (37 if cap else 0)
    src = torch.full((k, Ep + 3, 4), CANARY, device='cuda')
    a = src[:, :Ep]
    a[:, :cnt] = softmax_a(g, k, 5).cuda()
    dst = torch.full((k, Ep + 5, 4), -CANARY, device='cuda')
    out = K.attn_export(G, a, out=dst[:, :Ep])
    want = torch.full_like(dst, -CANARY)
    eid = torch.from_numpy(g['eid_s']).cuda()
    assert torch.equal(torch.sort(eid).values, torch.arange(cnt, device='cuda'))
    want[:, eid] = a[:, :cnt]
    assert torch.equal(dst, want) and out.data_ptr() == dst.data_ptr()
    assert torch.equal(K.attn_export(G, a.contiguous())[:, :cnt], want[:, :cnt])


HUBS = [63, 64, 65, 257, None]  # in-degree of the hub target, self loop included (None: n)
TRACE_CASES = [(n, B, k, head) for n in (1, 2, 63, 64, 65, 200, 1024) for B in (1, 3) for k in (1, 5) for head in (-1, 2)]


def trace_graph(i, n, B):
    hub = HUBS[i % 5] or n
    return make_graph(B, n, 1000 + i, hub_deg=hub if n > 1 else 0, hub_root=(i // 5) % 2 == 0)


def guarded(shape, dtype, fill):
    """a contiguous tensor of that shape in the middle of a buffer of canaries -> (tensor, buffer)"""
    numel = int(np.prod(shape))
    buf = torch.full((numel + 256,), fill, dtype=dtype, device='cuda')
    return buf[128:128 + numel].view(shape), buf


def guards_intact(buf, fill):
    return bool((buf[:128] == fill).all()) and bool((buf[-128:] == fill).all())


def run_trace(K, G, a, B, n, k, root=0, head=-1):
    N = G.N
    outs = [guarded((k + 1, N), torch.float32, CANARY), guarded((k + 1, N), torch.float32, CANARY), guarded((k, N), torch.int32, -7)]
    K.attn_trace(G, a, B, n, root, head, out=tuple(t for t, _ in outs))
    torch.cuda.synchronize()
    for (_, buf), fill in zip(outs, (CANARY, CANARY, -7)):
        assert guards_intact(buf, fill), 'a canary around an output was overwritten'
    return tuple(t for t, _ in outs)


@pytest.mark.gpu
@pytest.mark.parametrize('i,case', list(enumerate(TRACE_CASES)), ids=[f'n{n}-B{B}-k{k}-h{h}' for n, B, k, h in TRACE_CASES])
def test_attn_trace_against_twin(i, case):
    """the kernel against the float64 twin on the SAME a (read back from the device): PAD slots, parallel edges, a hub target of in-degree
    63 / 64 / 65 / 257 / n (the context node itself in every other case); canaries around the outputs; two calls, the same bits"""
    n, B, k, head = case
    K = hip()
    ei, et, nt = trace_graph(i, n, B)
    G = dev_graph(K, ei, et, nt, n)
    g = TW.graph_arrays(G)
    a = softmax_a(g, k, 2000 + i).cuda()
    got = run_trace(K, G, a, B, n, k, 0, head)
    again = run_trace(K, G, a, B, n, k, 0, head)
    for x, y in zip(got, again):
        assert torch.equal(x, y)
    a_host = a.cpu().numpy()
    tw = TW.trace(g, a_host, n, 0, head)
    if n > 1:
        want_m = HUBS[i % 5] or n
        assert tw['m'] >= want_m and (np.diff(g['rowptr_t']) == want_m).any()
    exempt, total = check_trace(f64(*got), tw, k, f'trace n={n} B={B} k={k} head={head}', a_host, g, n, head)
    note(f'FIGURE trace n={n} B={B} k={k} head={head}: {exempt} of {total} reachable nodes exempt as near-ties')


@pytest.mark.gpu
@pytest.mark.parametrize('n,B', [(1, 3), (65, 3), (200, 2)])
def test_attn_trace_without_real_edges(n, B):
    """only self loops: the mass stays on the context node at every layer, along its self loop"""
    K = hip()
    k = 5
    G = dev_graph(K, torch.zeros((2, 0), dtype=torch.long), torch.zeros(0, dtype=torch.long), torch.full((B * n,), 2), n)
    a = torch.ones((k, G.Ep, 4), device='cuda')
    flow, best, pred = run_trace(K, G, a, B, n, k)
    want = torch.zeros((k + 1, B * n), device='cuda')
    want[:, ::n] = 1
    wp = torch.full((k, B * n), -1, dtype=torch.int32, device='cuda')
    wp[:, ::n] = torch.arange(0, B * n, n, dtype=torch.int32, device='cuda')
    assert torch.equal(flow, want) and torch.equal(best, want) and torch.equal(pred, wp)
    f0, b0, _ = K.attn_trace(G, a[:0], B, n)  # k = 0: layer 0 only
    assert torch.equal(f0, want[:1]) and torch.equal(b0, want[:1])


@pytest.mark.gpu
def test_attn_trace_refusals():
    """n = 1025, block_n != n, N != B n, head = 4, root = n: QAGNN_EINVAL before anything is enqueued, the outputs untouched"""
    K = hip()
    B, n, k = 2, 8, 2
    ei, et, nt = make_graph(B, n, 3)
    G = dev_graph(K, ei, et, nt, n)
    G1025 = dev_graph(K, torch.zeros((2, 0), dtype=torch.long), torch.zeros(0, dtype=torch.long), torch.zeros(1025, dtype=torch.long), 1025)
    a = torch.ones((k, G.Ep, 4), device='cuda')
    for what, graph, args in (('n = 1025', G1025, (1, 1025, 0, -1)), ('block_n != n', G, (4, 4, 0, -1)), ('N != B n', G, (3, 8, 0, -1)),
                              ('head = 4', G, (2, 8, 0, 4)), ('root = n', G, (2, 8, 8, -1)), ('root = -1', G, (2, 8, -1, -1))):
        N = graph.N
        outs = (torch.full((k + 1, N), CANARY, device='cuda'), torch.full((k + 1, N), CANARY, device='cuda'),
                torch.full((k, N), -7, dtype=torch.int32, device='cuda'))
        with pytest.raises(RuntimeError, match='attn_trace'):
            K.attn_trace(graph, torch.ones((k, graph.Ep, 4), device='cuda'), *args, out=outs)
        torch.cuda.synchronize()
        assert bool((outs[0] == CANARY).all()) and bool((outs[1] == CANARY).all()) and bool((outs[2] == -7).all()), what
    # (the binding refuses a short layer stride itself: the library's own check is reached directly, with outputs it must not touch)
    out = torch.full((3 * (k + 1) * G.N,), CANARY, device='cuda')
    rc = K.lib.qagnn_attn_trace_f32(ctypes.byref(G.c), a.data_ptr(), 4 * G.Ep - 4, k, B, n, 0, -1, out.data_ptr(), out.data_ptr(), out.data_ptr(), None)
    assert rc == 1 and b'layer_stride' in K.lib.qagnn_last_error()
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())


@pytest.mark.gpu
def test_attn_trace_ties():
    """two parallel root edges at exactly 0.5: pred is the lower edge id"""
    K = hip()
    ei, et, nt = tie_case()
    G = dev_graph(K, ei, et, nt, 2)
    g = TW.graph_arrays(G)
    flow, best, pred = run_trace(K, G, tie_a(g, 2).cuda(), 1, 2, 2)
    assert pred.tolist() == [[2, 0], [2, 0]] and best.tolist() == [[1, 0], [0.25, 0.5], [0.0625, 0.125]]
    assert flow.tolist() == [[1, 0], [0.25, 1.0], [0.0625, 0.5]]


@pytest.mark.gpu
def test_attn_trace_nan():
    """one NaN in one subgraph's a: its flow is NaN where the twin's is, its pred stays in [-1, Ep), every other subgraph keeps its bits"""
    K = hip()
    B, n, k = 3, 65, 5
    ei, et, nt = make_graph(B, n, 77, hub_deg=65, hub_root=True)
    G = dev_graph(K, ei, et, nt, n)
    g = TW.graph_arrays(G)
    a = softmax_a(g, k, 9).cuda()
    clean = run_trace(K, G, a, B, n, k)
    a[1, int(g['rowptr_s'][n]) + 1, 2] = float('nan')  # an out-edge of subgraph 1's context node, layer 1
    got = run_trace(K, G, a, B, n, k)
    tw = TW.trace(g, a.cpu().numpy(), n)
    assert np.isnan(tw['flow'][:, n:2 * n]).any()
    check_trace(f64(*got), tw, k, 'trace NaN', cap=0.02)
    assert int(got[2].min()) >= -1 and int(got[2].max()) < G.Ep and not bool(torch.isnan(got[1]).any())
    for x, c in zip(got, clean):
        for b in (0, 2):
            assert torch.equal(x[:, b * n:(b + 1) * n], c[:, b * n:(b + 1) * n])


@pytest.mark.gpu
def test_attn_kernels_inside_a_captured_graph():
    """attn_trace and attn_export inside one torch.cuda.graph (a single chain), replayed twice with a rewritten between the replays, equal
    the eager calls bit for bit"""
    K = hip()
    B, n, k = 3, 65, 5
    ei, et, nt = make_graph(B, n, 21, hub_deg=64)
    G = dev_graph(K, ei, et, nt, n)
    g = TW.graph_arrays(G)
    As = [softmax_a(g, k, s).cuda() for s in (1, 2)]
    a = As[0].clone()
    outs = (torch.empty((k + 1, G.N), device='cuda'), torch.empty((k + 1, G.N), device='cuda'), torch.empty((k, G.N), dtype=torch.int32, device='cuda'))
    alpha = torch.empty((k, G.Ep, 4), device='cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the capture
        K.attn_trace(G, a, B, n, out=outs)
        K.attn_export(G, a, out=alpha)
    torch.cuda.current_stream().wait_stream(side)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        K.attn_trace(G, a, B, n, out=outs)
        K.attn_export(G, a, out=alpha)
    for src in As[::-1]:
        a.copy_(src)
        for t in outs + (alpha,):
            t.fill_(-3)
        cg.replay()
        torch.cuda.synchronize()
        for x, y in zip(outs, K.attn_trace(G, src, B, n)):
            assert torch.equal(x, y)
        assert torch.equal(alpha, K.attn_export(G, src))


MODULE_CASES = {'4x16': dict(nq=4, n=16, shape='tiny'), '41x200': dict(nq=41, n=200, shape='csqa')}


def cu(args):
    return [t.cuda() for t in args]


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(MODULE_CASES))
def test_module_against_oracle_and_twin(name, monkeypatch):
    """d = 32, k = 3: 4 x 16 node rows, and 41 x 200, above the packed-image threshold (the three-MFMA form is on).  Logits and pool_attn bit
    for bit those of the plain inference-path forward; alpha against the float64 oracle; flow / best / pred against the twin on the
    returned alpha; the plain pair, a PackedGraphBatch and a StoreBatch give one trace bit for bit."""
    K = hip()
    case = small_case(**MODULE_CASES[name])
    k, B, n = case['cfg']['k'], case['nq'], case['n']
    args = case_args(case)
    if name == '41x200':
        assert B * n >= K.PACK_MIN_M and K.gemm_split == 2
    model = build_model(case).cuda()
    d = cu(args)
    flat = d[:5] + [(d[5], d[6])]
    with torch.no_grad():
        with ops.inference_path():
            logits, attn = model(*flat)
        rec = explain.trace(model, *flat, edges=True)
        lean = explain.trace(model, *flat)
    assert torch.equal(rec.logits, logits) and torch.equal(rec.pool_attn, attn)
    assert lean.alpha is None and all(torch.equal(getattr(lean, f), getattr(rec, f)) for f in ('logits', 'flow', 'best', 'pred', 'pred_src'))
    assert torch.equal(rec.edge_index[:, :d[5].size(1)], d[5]) and torch.equal(rec.edge_type, d[6])
    worst = check_alpha(rec.alpha, oracle_alpha(case, args, monkeypatch), f'module {name}')
    note(f'FIGURE module {name}: deeper-layer alpha worst relative error {worst:.3e} (bar DEEP_ALPHA_RTOL = {DEEP_ALPHA_RTOL:.1e})')
    check_record_against_twin(rec, ops_graph_dims(case), k, f'module {name}')
    mass = (rec.flow.double().sum(2) - 1).abs().max().item()
    assert mass <= TW.bounds(k, n + 1)[0] + 1e-6
    # the same batch through the other graph holders
    recs = {}
    for kind, fl in holders_of(case, d).items():
        with torch.no_grad():
            recs[kind] = explain.trace(model, *fl, edges=True)
    for kind in ('blobs', 'store'):
        for f in ('logits', 'pool_attn', 'flow', 'best', 'pred', 'pred_src', 'alpha', 'edge_index', 'edge_type', 'concept_ids', 'node_type_ids'):
            assert torch.equal(getattr(recs[kind], f), getattr(recs['pair'], f)), (kind, f)
    for f in ('logits', 'pool_attn', 'flow', 'best'):  # (the blobs keep the caller's edges per sample: the same graph as the lists')
        assert torch.equal(getattr(recs['pair'], f), getattr(rec, f)), f


def holders_of(case, d):
    """the batch as the plain pair, a PackedGraphBatch and a StoreBatch, all out of ONE blob store -> {kind: flat decoder inputs}"""
    B, n, nc, cfg = case['nq'] * case['nc'], case['n'], case['nc'], case['cfg']
    inp = helpers.make_case_inputs(case)
    store = data_utils.GraphBlobStore.build(inp['edge_index_list'], inp['edge_type_list'], inp['node_type_ids'], cfg['n_etype'], cfg['n_ntype'])
    ids = list(range(B))
    buf, Bb, E = store.pack(ids)
    packed = data_utils.PackedGraphBatch(buf.cuda(), Bb, E, store, ids, nc)
    dstore = data_utils.DeviceGraphStore.from_host(store, inp['concept_ids'].view(B, n), inp['node_type_ids'].view(B, n),
                                                   inp['node_scores'].view(B, n, 1), inp['adj_lengths'].view(B), 'cuda')
    return {'pair': d[:5] + [packed.batched(device='cuda')], 'blobs': d[:5] + [packed], 'store': [d[0], None, None, None, None, dstore.batch(ids, nc)]}


@pytest.mark.gpu
def test_module_k0_and_refusals():
    case = small_case(k=0)
    model = build_model(case).cuda()
    d = cu(case_args(case))
    flat = d[:5] + [(d[5], d[6])]
    with torch.no_grad():
        rec = explain.trace(model, *flat, edges=True)
        with ops.inference_path():
            logits, _ = model(*flat)
    B, n = case['nq'], case['n']
    assert torch.equal(rec.logits, logits) and rec.flow.shape == (1, B, n) and rec.pred.shape == (0, B, n) and rec.alpha.shape == (0, d[5].size(1) + B * n, 4)
    assert rec.flow[0, :, 0].tolist() == [1.0] * B and float(rec.flow.sum()) == B and rec.path(0, 0) == []
    model = build_model(small_case()).cuda()
    with pytest.raises(RuntimeError, match='torch.no_grad'):
        explain.trace(model, *flat)
    with torch.no_grad(), pytest.raises(RuntimeError, match='model.eval'):
        explain.trace(model.train(), *flat)
    assert ops.ATTN_CAPTURE is None and ops.INFERENCE_PATH is False


@pytest.mark.gpu
def test_evaluate_detail(tmp_path):
    """three batches with a ragged last one: predictions = argmax of the eager logits, accuracy = evaluate_accuracy's, the file's text;
    with trace=True one Trace per batch, equal to explain.trace on that batch"""
    hip()
    nc, n = 2, 16
    sets, want, g = [], [], torch.Generator().manual_seed(3)
    model = build_model(small_case()).cuda()
    q = 0
    for i, Q in enumerate((3, 3, 2)):
        case = small_case(nq=Q * nc, n=n, seed=40 + i)
        d = cu(case_args(case))
        flat = d[:5] + [(d[5], d[6])]
        labels = torch.randint(0, nc, (Q,), generator=g)
        sets.append(([f'id-{q + j}' for j in range(Q)], labels, *flat))
        with torch.no_grad():
            want += model(*flat)[0].view(Q, nc).argmax(1).tolist()
        q += Q
    path = tmp_path / 'preds.csv'
    acc, results, traces = inference.evaluate_detail(sets, model, preds_path=str(path), trace=True, head=1)
    assert [p for _, p in results] == want and [qid for qid, _ in results] == [f'id-{j}' for j in range(8)]
    assert acc == inference.evaluate_accuracy(sets, model) == sum(int(p == int(l)) for p, l in zip(want, torch.cat([s[1] for s in sets]))) / 8
    assert path.read_text() == ''.join(f'id-{j},{"AB"[p]}\n' for j, p in enumerate(want))
    assert len(traces) == 3
    with torch.no_grad():
        for rec, s in zip(traces, sets):
            one = explain.trace(model, *s[2:], head=1)
            assert all(torch.equal(getattr(rec, f), getattr(one, f)) for f in ('logits', 'flow', 'best', 'pred'))
    plain = inference.evaluate_detail(sets, model)
    assert plain[0] == acc and plain[1] == results and plain[2] is None
