"""The int64 edge-list protocol in capacity form: qagnn_graph_prep_cap, data_utils.EdgeListBatch, and graphed.GraphedStep on edge lists.

CPU: EdgeListBatch.from_lists == batch_graph; the holder through QAGNN.forward == the plain pair (emulation provider, which has no
capacity call: the holder is sliced).  `-m gpu`, kernel level: qagnn_graph_prep_cap == qagnn_graph_from_blobs at the same capacity, bit
for bit over every array's defined range, whatever the unread tail [E, cap) of the edge buffers holds; a count outside [0, cap] is
clamped and flagged; the host rejections.  Module level: a replayed step on edge lists == the eager step on blobs at the same capacity.
"""
import ctypes as C

import pytest
import torch

import helpers
from qagnn_amd import data_utils, graphed, ops, synthetic
from qagnn_amd import modeling_qagnn as MQ

T = 4
EP_ARRAYS = ('tgt_s', 'src_s', 'cls_s', 'eid_s', 'src_t', 'tgt_t', 'cls_t', 'pos_t', 'src_c', 'tgt_c', 'pos_c')
TAIL_FILLS = (2 ** 40, -1, 0)  # out of range high, out of range low, and in range: a read of the tail would ADD edges, not raise a flag


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nc', [4, 5])
def test_from_lists_equals_batch_graph(nc):
    nq, n = 3, 60
    recs = synthetic.make_records(nq * nc, seed=nc, shape='csqa', n_rel=17, n_concept_vocab=2000)
    ei, et = data_utils.records_to_tensors(recs, n, nc)[5:7]
    ei[nc + 1], et[nc + 1] = torch.zeros((2, 0), dtype=torch.long), torch.zeros((0,), dtype=torch.long)  # one sample without edges
    nest = lambda flat: [flat[q * nc:(q + 1) * nc] for q in range(nq)]  # noqa: E731
    want_ei, want_et = data_utils.batch_graph(ei, et, n)
    b = data_utils.EdgeListBatch.from_lists(nest(ei), nest(et), n)
    assert b.E == want_ei.size(1) and b.e_cap is None and b.count is None
    assert torch.equal(b.edge_index, want_ei) and torch.equal(b.edge_type, want_et)
    cap = b.E + 37
    p = data_utils.EdgeListBatch.from_lists(nest(ei), nest(et), n, e_cap=cap)
    assert (p.E, p.e_cap) == (b.E, cap) and p.edge_index.shape == (2, cap) and p.edge_type.shape == (cap,)
    assert all(torch.equal(x, y) for x, y in zip(p.pair(), (want_ei, want_et)))
    assert p.edge_index.dtype == torch.long and p.edge_type.dtype == torch.long


@pytest.mark.parametrize('with_cap', [False, True])
def test_holder_through_the_model_equals_the_pair_on_the_emulation_provider(with_cap):
    from emu_kernels import EmuKernels
    from test_host_logic_emu import build
    case = 'small_train'
    c = helpers.GOLDEN_CASES[case]
    inp = helpers.make_case_inputs(case)
    n, B = c['n'], c['nq'] * c['nc']
    ei, et = inp['edge_index'], inp['edge_type']
    E, cap = ei.size(1), ei.size(1) + 23
    ei_buf, et_buf = torch.full((2, cap), 2 ** 40, dtype=torch.long), torch.full((cap,), -1, dtype=torch.long)  # a tail nobody may read
    ei_buf[:, :E], et_buf[:E] = ei, et
    holder = data_utils.EdgeListBatch(ei_buf, et_buf, E, cap if with_cap else None)
    args = (inp['sent_vecs'], inp['concept_ids'].view(B, n), inp['node_type_ids'].view(B, n), inp['node_scores'].view(B, n, 1),
            inp['adj_lengths'].view(B))
    old = ops.set_kernels(EmuKernels())
    try:
        outs = []
        for adj in ((ei, et), holder):
            model = build(case)
            logits, attn = model(*args, adj)
            logits.sum().backward()
            outs.append((logits.detach(), attn.detach(), {k: p.grad for k, p in model.named_parameters() if p.grad is not None}))
    finally:
        ops.set_kernels(old)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert set(outs[0][2]) == set(outs[1][2]) and len(outs[0][2]) > 10
    assert all(torch.equal(outs[0][2][k], outs[1][2][k]) for k in outs[0][2])


# ---------------------------------------------------------------------------------------------------------------------
# GPU, kernel level
# ---------------------------------------------------------------------------------------------------------------------
def hip():
    ops.set_kernels(None)
    return ops.kernels()


class _Graph:
    """One batch in both forms: per-sample local edge lists -> blob store (the reference side) and batch_graph's int64 pair."""

    def __init__(self, ei_list, et_list, nt, R):
        self.B, self.n, self.R = len(ei_list), nt.size(1), R
        self.nt = nt.reshape(-1).cuda()
        self.store = data_utils.GraphBlobStore.build(ei_list, et_list, nt, R, T)
        buf, B, E = self.store.pack(list(range(self.B)))
        self.E = E
        self.packed = data_utils.PackedGraphBatch(buf.cuda(), B, E, self.store, list(range(B)), 1)
        self.ei, self.et = data_utils.batch_graph(ei_list, et_list, self.n)
        assert self.ei.size(1) == E

    def reference(self, K, cap):
        self.packed.e_cap = cap
        return K.graph_from_blobs(self.packed, self.nt)

    def buffers(self, cap, fill, room=None):
        room = cap if room is None else room
        ei = torch.full((2, room), fill, dtype=torch.long)
        et = torch.full((room,), fill, dtype=torch.long)
        ei[:, :self.E], et[:self.E] = self.ei, self.et
        return ei.cuda(), et.cuda()


def _rand_graph(seed, B, n, counts, R=5):
    g = torch.Generator().manual_seed(seed)
    ei = [torch.randint(0, n, (2, c), generator=g) for c in counts]  # (parallel edges and self edges included)
    et = [torch.randint(0, R, (c,), generator=g) for c in counts]
    return _Graph(ei, et, torch.randint(0, T, (B, n), generator=g), R)


def _hub_graph():
    g = torch.Generator().manual_seed(5)
    n, R = 16, 5
    rnd = lambda c: torch.randint(0, n, (c,), generator=g)  # noqa: E731
    src = torch.cat([torch.full((70,), 3), torch.full((130,), 9), rnd(70)])
    tgt = torch.cat([rnd(70), rnd(130), torch.full((70,), 12)])
    perm = torch.randperm(270, generator=g)  # the hubs' edges interleaved in the caller's order
    ei = torch.stack([src, tgt])[:, perm]
    return _Graph([ei], [torch.randint(0, R, (270,), generator=g)], torch.randint(0, T, (1, n), generator=g), R)


def _csqa_graph():
    n = 200
    recs = synthetic.make_records(2, seed=3, shape='csqa', n_rel=17, n_concept_vocab=2000)
    _, _, nt, _, _, ei, et, _ = data_utils.records_to_tensors(recs, n, 1)
    return _Graph(ei, et, nt, 38)


def _same_graph(g, ref, E, what, err0=0):
    """every array of the contract over its defined range; g and ref are laid out for the same capacity, E is the batch's true count"""
    torch.cuda.synchronize()
    assert (g.N, g.E, g.Ep, g.C, g.max_chunks, g.c.n_groups, g.c.block_n) == (ref.N, ref.E, ref.Ep, ref.C, ref.max_chunks, ref.c.n_groups, ref.c.block_n), what
    N, Ept = g.N, E + g.N
    for arr in ('rowptr_s', 'rowptr_t'):
        assert torch.equal(g.array(arr, N + 1), ref.array(arr, N + 1)), f'{what}: {arr}'
    assert int(g.array('rowptr_s', N + 1)[-1]) == Ept and int(g.array('rowptr_t', N + 1)[-1]) == Ept, what
    for arr in EP_ARRAYS:
        assert torch.equal(g.array(arr, Ept), ref.array(arr, Ept)), f'{what}: {arr}'
    assert torch.equal(g.array('eid_s', Ept).sort().values, torch.arange(Ept, dtype=torch.int32, device='cuda')), f'{what}: edge ids'
    assert torch.equal(g.array('cls_count', g.C), ref.array('cls_count', g.C)), f'{what}: cls_count'
    nch = int(g.array('n_chunks', 1).item())
    assert nch == int(ref.array('n_chunks', 1).item()), f'{what}: n_chunks'
    for arr in ('chunk_cls', 'chunk_beg', 'chunk_len'):
        assert torch.equal(g.array(arr, nch), ref.array(arr, nch)), f'{what}: {arr}'
    pairs = g.c.n_groups * g.C
    assert torch.equal(g.array('chunkptr', pairs + 1), ref.array('chunkptr', pairs + 1)), f'{what}: chunkptr'
    assert ref.array('err', 4).tolist() == [0, 0, 0, 0], what
    assert g.array('err', 4).tolist() == [err0, 0, 0, 0], f'{what}: flags {g.array("err", 4).tolist()}'
    assert torch.equal(g.array('err', 13)[4:], ref.array('err', 13)[4:]), f'{what}: XCD partition'


CAP_CASES = {
    'no edges': lambda: (_rand_graph(1, 3, 8, [0, 0, 0]), 16),
    'full': lambda: (_rand_graph(2, 2, 16, [23, 17]), 40),
    'one short': lambda: (_rand_graph(3, 2, 16, [23, 16]), 40),
    'block straddle': lambda: (_rand_graph(4, 2, 16, [120, 110]), 300),
    'hubs': lambda: (_hub_graph(), 270 + 57),
    'many relations': lambda: (_csqa_graph(), None),
}


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CAP_CASES))
def test_graph_prep_cap_bit_identical_to_blobs_at_the_same_capacity(name):
    K = hip()
    G, cap = CAP_CASES[name]()
    cap = graphed.edge_capacity(G.E) if cap is None else cap
    assert G.E <= cap and G.E == {'no edges': 0, 'full': 40, 'one short': 39, 'block straddle': 230, 'hubs': 270}.get(name, G.E)
    ref = G.reference(K, cap)
    for fill in TAIL_FILLS:
        ei, et = G.buffers(cap, fill)
        batch = data_utils.EdgeListBatch(ei, et, G.E, cap)
        g = K.graph_prep_cap(batch, G.nt, G.R, T, block_n=G.n)
        assert g.dynamic and g.E == cap and g.keep[0] is ei
        _same_graph(g, ref, G.E, f'{name}, tail = {fill}')
    if G.E == cap:  # the plain sorting path at the true count
        plain = K.graph_prep(G.ei.cuda(), G.et.cuda(), G.nt, G.R, T, block_n=G.n)
        _same_graph(g, plain, G.E, f'{name}: against graph_prep')


@pytest.mark.gpu
def test_graph_prep_cap_reuses_storage_and_buffers_like_a_replay():
    """Two calls on one stream into the same storage, out of the same edge buffers and count word, E = 230 then E = 97: nothing of the
    first call (counters, orders, the 133 edges left behind in the tail) may reach the second."""
    K = hip()
    cap = 300
    G1, G2 = _rand_graph(4, 2, 16, [120, 110]), _rand_graph(6, 2, 16, [50, 47])
    ref = G2.reference(K, cap)
    for fill in TAIL_FILLS:
        ei, et = G1.buffers(cap, fill)
        batch = data_utils.EdgeListBatch(ei, et, G1.E, cap)
        storage = torch.empty(K.lib.qagnn_graph_storage_elems(G1.nt.numel(), cap, G1.R, T), dtype=torch.int32, device='cuda')
        K.graph_prep_cap(batch, G1.nt, G1.R, T, block_n=16, storage=storage)
        ei[:, :G2.E].copy_(G2.ei, non_blocking=True)
        et[:G2.E].copy_(G2.et, non_blocking=True)
        batch.count.fill_(G2.E)
        batch.E = G2.E
        g = K.graph_prep_cap(batch, G2.nt, G2.R, T, block_n=16, storage=storage)
        assert g.storage is storage
        _same_graph(g, ref, G2.E, f'second call, tail = {fill}')


@pytest.mark.gpu
def test_graph_prep_cap_clamps_and_flags_a_bad_count():
    K = hip()
    cap, room = 40, 45
    from qagnn_amd import _lib
    _lib.ERR_WATCH.poll(block=True)
    G = _rand_graph(2, 2, 16, [23, 17])
    G0 = _Graph([torch.zeros((2, 0), dtype=torch.long)] * 2, [torch.zeros((0,), dtype=torch.long)] * 2, G.nt.view(2, 16).cpu(), G.R)  # same rows, no edges
    refs = {cap + 5: (G.reference(K, cap), G.E), -3: (G0.reference(K, cap), 0)}  # a count above the capacity: E = cap; below zero: E = 0
    for fill in TAIL_FILLS:
        for word, (ref, E) in refs.items():
            ei, et = G.buffers(cap, fill, room=room)  # buffers and storage with room for the bad count: no implementation can leave them
            storage = torch.empty(K.lib.qagnn_graph_storage_elems(G.nt.numel(), room, G.R, T), dtype=torch.int32, device='cuda')
            batch = data_utils.EdgeListBatch(ei, et, G.E, cap)
            batch.count.fill_(word)
            g = K.graph_prep_cap(batch, G.nt, G.R, T, block_n=16, storage=storage)
            _same_graph(g, ref, E, f'count word {word}, tail = {fill}', err0=1)
            with pytest.raises(RuntimeError, match='out-of-range input'):  # (the flag reaches the host like any other validation word)
                _lib.ERR_WATCH.poll(block=True)


@pytest.mark.gpu
def test_graph_prep_cap_host_rejections_launch_nothing():
    from qagnn_amd import _lib
    K = hip()
    cap = 40
    G = _rand_graph(2, 2, 16, [23, 17])
    ei, et = G.buffers(cap, 0)
    batch = data_utils.EdgeListBatch(ei, et, G.E, cap)
    N = G.nt.numel()
    storage = torch.full((K.lib.qagnn_graph_storage_elems(N, cap, G.R, T),), -7, dtype=torch.int32, device='cuda')
    g = _lib.qagnn_graph()
    call = lambda ld, cnt: K.lib.qagnn_graph_prep_cap(C.byref(g), storage.data_ptr(), ei.data_ptr(), ld, et.data_ptr(), G.nt.data_ptr(),  # noqa: E731
                                                      N, cap, cnt, G.R, T, 16, K._stream())
    assert call(cap - 1, batch.count.data_ptr()) != 0 and b'ld_edge' in K.lib.qagnn_last_error()
    assert call(cap, None) != 0 and b'count' in K.lib.qagnn_last_error()
    batch.E = cap + 1
    with pytest.raises(AssertionError, match='capacity'):
        K.graph_prep_cap(batch, G.nt, G.R, T, block_n=16, storage=storage)
    torch.cuda.synchronize()
    assert bool((storage == -7).all()), 'a rejected call wrote to the storage'


# ---------------------------------------------------------------------------------------------------------------------
# GPU, module level (the _model / _batch recipe of tests/test_graphed.py)
# ---------------------------------------------------------------------------------------------------------------------
def _model(p, seed=0):
    cfg = helpers.model_cfg(d=200, k=5, sent_dim=64, n_concept=2000, concept_in_dim=32)
    torch.manual_seed(seed)
    m = MQ.QAGNN(None, cfg['k'], 4, 38, cfg['sent_dim'], cfg['n_concept'], 200, cfg['concept_in_dim'], 2, 200, 0, p, p, p)
    helpers.det_fill_(m, 9, 0.6)
    if p == 0.0:
        m.pooler.dropout.p = m.pooler.attention.dropout.p = 0.0
    return m.cuda().train()


_BATCHES = {}


def _batch(nq, nc, n, seed):
    key = (nq, nc, n, seed)
    if key in _BATCHES:  # (built once, shared, never modified)
        return _BATCHES[key]
    recs = synthetic.make_records(nq * nc, seed=seed, shape='csqa', n_rel=17, n_concept_vocab=2000)
    _, cids, nt, ns, al, ei, et, _ = data_utils.records_to_tensors(recs, n, nc)
    store = data_utils.GraphBlobStore.build(ei, et, nt, 38, 4)
    buf, B, E = store.pack(list(range(nq * nc)))
    g = torch.Generator().manual_seed(seed)
    sent = torch.randn(nq * nc, 64, generator=g)
    labels = torch.randint(0, nc, (nq,), generator=g)
    bei, bet = data_utils.batch_graph(ei, et, n)
    nest = lambda flat: [flat[q * nc:(q + 1) * nc] for q in range(nq)]  # noqa: E731
    _BATCHES[key] = dict(sent=sent.cuda(), cids=cids.cuda(), nt=nt.cuda(), ns=ns.cuda(), al=al.cuda(), labels=labels.cuda(),
                         packed=data_utils.PackedGraphBatch(buf.cuda(), B, E, store, list(range(B)), nc),
                         ei=bei, et=bet, lists=(nest(ei), nest(et)), E=E, n=n)
    return _BATCHES[key]


def _blobs_at(b, nc, e_cap):
    packed = b['packed']
    if e_cap is None:
        return packed
    blob = torch.zeros(packed.head + 2 * packed.n * packed.B + 3 * e_cap, dtype=torch.int32, device='cuda')
    blob[:packed.buf.numel()] = packed.buf
    packed = data_utils.PackedGraphBatch(blob, packed.B, packed.E, packed.store, packed.sample_ids, nc)
    packed.e_cap = e_cap
    return packed


def _edges_at(b, e_cap, fill=2 ** 40):
    ei = torch.full((2, e_cap), fill, dtype=torch.long)
    et = torch.full((e_cap,), fill, dtype=torch.long)
    ei[:, :b['E']], et[:b['E']] = b['ei'], b['et']
    return data_utils.EdgeListBatch(ei.cuda(), et.cuda(), b['E'], e_cap)


def _eager(model, b, nc, adj, lw=1.0):
    for p in model.parameters():
        p.grad = None
    logits, _ = model(b['sent'], b['cids'], b['nt'], b['ns'], b['al'], adj)
    loss = torch.nn.functional.cross_entropy(logits.view(-1, nc), b['labels']) * lw
    loss.backward()
    return (logits.detach().clone(), loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
            {k: v.clone() for k, v in model.named_buffers()})


def _state(model, logits, loss):
    return (logits.detach().clone(), loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
            {k: v.clone() for k, v in model.named_buffers()})


def _same(a, b, what):
    la, sa, ga, ba = a
    lb, sb, gb, bb = b
    assert torch.equal(la, lb), f'{what}: logits differ by {(la - lb).abs().max().item():.3e}'
    assert torch.equal(sa, sb), f'{what}: loss'
    assert set(ga) == set(gb)
    bad = [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert not bad, f'{what}: {len(bad)} gradients differ, e.g. {bad[:3]}'
    badb = [k for k in ba if not torch.equal(ba[k], bb[k])]
    assert not badb, f'{what}: buffers differ: {badb[:3]}'


def _graph_input(b, form):
    if form == 'device':
        return b['ei'].cuda(), b['et'].cuda()
    if form == 'host':
        return b['ei'], b['et']
    return data_utils.EdgeListBatch.from_lists(*b['lists'], b['n'])


@pytest.mark.gpu
@pytest.mark.parametrize('form', ['device', 'host', 'from_lists'])
def test_replay_on_edge_lists_is_bit_identical_to_the_eager_step_on_blobs(form):
    ops.set_kernels(None)
    nq, nc, n = 2, 5, 200
    batches = [_batch(nq, nc, n, seed) for seed in (3, 4, 5)]
    m_eager, m_graph = _model(0.0), _model(0.0)
    step = graphed.GraphedStep(m_graph, nc)
    for i, b in enumerate(batches):
        cap = graphed.edge_capacity(b['E'])
        want = _eager(m_eager, b, nc, _blobs_at(b, nc, cap), lw=0.5)
        logits, loss = step(b['sent'], b['cids'], b['nt'], b['ns'], b['al'], _graph_input(b, form), b['labels'], 0.5)
        _same(_state(m_graph, logits, loss), want, f'batch {i} (E = {b["E"]}, capacity {cap}, {form})')
    assert step.n_graphs <= len({graphed.edge_capacity(b['E']) for b in batches})
    assert int(m_graph.gnn.gnn_layers[0].mlp[1].num_batches_tracked) == len(batches)


@pytest.mark.gpu
@pytest.mark.parametrize('prep_overlap', [True, False])
def test_edge_list_replays_enqueued_back_to_back_equal_the_eager_step(prep_overlap, monkeypatch):
    ops.set_kernels(None)
    from qagnn_amd import _lib
    monkeypatch.setattr(ops, 'PREP_OVERLAP', prep_overlap)
    _lib.ERR_WATCH.poll(block=True)
    nq, nc, n = 2, 5, 200
    b = _batch(nq, nc, n, 13)
    cap = graphed.edge_capacity(b['E'])
    m_ref, m = _model(0.0), _model(0.0)
    want = _eager(m_ref, b, nc, _blobs_at(b, nc, cap))
    step = graphed.GraphedStep(m, nc)
    adj = (b['ei'].cuda(), b['et'].cuda())
    call = lambda: step(b['sent'], b['cids'], b['nt'], b['ns'], b['al'], adj, b['labels'])  # noqa: E731

    def check(tag, logits, loss):
        torch.cuda.synchronize()
        got = (logits, loss, {k: q.grad for k, q in m.named_parameters() if q.grad is not None}, want[3])
        _same(got, want, tag)
        watched = next(iter(step._captured.values())).watched
        assert watched
        for flags, _, _ in watched:
            assert flags.tolist() == [0, 0, 0, 0], f'{tag}: validation words {flags.tolist()}'

    check('the capturing call', *call())
    for _ in range(12):
        out = call()
    check('12 calls with no synchronisation', *out)
    _lib.ERR_WATCH.poll(block=True)
    assert step.n_graphs == 1


@pytest.mark.gpu
def test_one_step_fed_blobs_and_edge_lists_in_alternation():
    ops.set_kernels(None)
    nq, nc, n = 2, 5, 200
    b = _batch(nq, nc, n, 13)
    cap = graphed.edge_capacity(b['E'])
    m_ref, m = _model(0.0), _model(0.0)
    twins = {'blobs': _eager(m_ref, b, nc, _blobs_at(b, nc, cap))}
    twins['edge lists'] = _eager(_model(0.0), b, nc, _edges_at(b, cap))
    step = graphed.GraphedStep(m, nc)
    adjs = {'blobs': b['packed'], 'edge lists': (b['ei'].cuda(), b['et'].cuda())}
    for i in range(6):
        kind = ('blobs', 'edge lists')[i % 2]
        logits, loss = step(b['sent'], b['cids'], b['nt'], b['ns'], b['al'], adjs[kind], b['labels'])
        got = (logits.detach().clone(), loss.detach().clone(), {k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None}, twins[kind][3])
        _same(got, twins[kind], f'call {i} ({kind})')  # (train-mode results do not depend on the running statistics the calls keep moving)
    assert step.n_graphs == 2


@pytest.mark.gpu
def test_eager_edge_list_capacity_changes_nothing():
    ops.set_kernels(None)
    b = _batch(2, 5, 200, 7)
    exact = _eager(_model(0.0), b, 5, (b['ei'].cuda(), b['et'].cuda()))
    roomy = _eager(_model(0.0), b, 5, _edges_at(b, graphed.edge_capacity(b['E']) + 4096))
    assert torch.equal(exact[0], roomy[0]) and torch.equal(exact[1], roomy[1])
    assert set(exact[2]) == set(roomy[2]) and all(torch.equal(exact[2][k], roomy[2][k]) for k in exact[2])
    for k in exact[3]:  # the edge encoder's running variance takes E'/(E'-1) as a device fp32 quotient instead of a host double: <= 1 ulp
        assert torch.allclose(exact[3][k].float(), roomy[3][k].float(), rtol=3e-7, atol=0), k


@pytest.mark.gpu
def test_corrupt_edge_list_raises_one_step_late_under_replay():
    ops.set_kernels(None)
    from qagnn_amd import _lib
    _lib.ERR_WATCH.poll(block=True)
    m = _model(0.0)
    step = graphed.GraphedStep(m, 5)
    good = _batch(2, 5, 200, 11)
    N = good['nt'].numel()
    ei, et = good['ei'].cuda(), good['et'].cuda()
    bad_ei = ei.clone()
    bad_ei[1, 17] = N  # one endpoint just past the node rows
    run = lambda e: step(good['sent'], good['cids'], good['nt'], good['ns'], good['al'], (e, et), good['labels'])  # noqa: E731
    run(ei)
    run(bad_ei)  # clamped on the device, flagged
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='out-of-range input'):
        run(ei)
    _lib.ERR_WATCH.poll(block=True)  # nothing left over
    run(ei)
    torch.cuda.synchronize()
    run(ei)  # the call after a clean batch does not raise
    torch.cuda.synchronize()
    _lib.ERR_WATCH.poll(block=True)
    assert step.n_graphs == 1
