"""The dataset's graphs resident on the device: data_utils.DeviceGraphStore / StoreBatch, qagnn_store_gather, qagnn_graph_from_store, and
graphed.GraphedStep on sample ids.

CPU: StoreBatch.fields() == host indexing, to_packed() == GraphBlobStore.pack(); the batch generator with device_store= yields what the
blob generator yields; QAGNN through the torch emulation on a StoreBatch == on the PackedGraphBatch; the host refusals.
`-m gpu`, kernel level: qagnn_graph_from_store == qagnn_graph_from_blobs on the packed batch, bit for bit, every array; the gather ==
host indexing with intact canaries, bad ids clamped and flagged; blob offsets behind 2^31 words.  Module level: the eager step and the
replayed step on a StoreBatch == the eager step on the PackedGraphBatch.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers  # noqa: F401  (puts the repository root on sys.path)
from qagnn_amd import data_utils, graphed, ops, synthetic
from qagnn_amd import modeling_qagnn as MQ
from qagnn_amd.data_utils import DeviceGraphStore, StoreBatch
from test_edge_list_capacity import _same, _same_graph, _state

T = 4


# ---------------------------------------------------------------------------------------------------------------------
# stores (built once, shared, never modified)
# ---------------------------------------------------------------------------------------------------------------------
class _Host:
    """per-sample local edge lists -> host blob store + the four node fields [S, n(, 1)] / [S]"""

    def __init__(self, ei, et, n, R, seed):
        g = torch.Generator().manual_seed(seed)
        S = len(ei)
        self.S, self.n, self.R = S, n, R
        self.nt = torch.randint(0, T, (S, n), generator=g)
        self.cids = torch.randint(1, 2000, (S, n), generator=g)
        self.cids[:, 0] = 0
        self.ns = torch.randn(S, n, 1, generator=g)
        self.al = torch.randint(2, n + 1, (S,), generator=g)
        self.store = data_utils.GraphBlobStore.build(ei, et, self.nt, R, T)

    def fields(self):
        return self.cids, self.nt, self.ns, self.al

    def device(self, device):
        return DeviceGraphStore.from_host(self.store, *self.fields(), device)


def _rand_edges(g, n, R, c):
    return torch.randint(0, n, (2, c), generator=g), torch.randint(0, R, (c,), generator=g)


def _hub(g, n, R, deg, by_source, extra=5):
    """one node with `deg` out-edges (or in-edges), `extra` random edges, shuffled into one caller order"""
    hub = torch.full((deg,), 7)
    other = torch.randint(0, n, (deg,), generator=g)
    ei = torch.stack([hub, other] if by_source else [other, hub])
    rei, _ = _rand_edges(g, n, R, extra)
    rei[0 if by_source else 1][rei[0 if by_source else 1] == 7] = 8  # the hub's degree stays exactly `deg`
    ei = torch.cat([ei, rei], dim=1)[:, torch.randperm(deg + extra, generator=g)]
    return ei, torch.randint(0, R, (deg + extra,), generator=g)


_STORES = {}


def _special(n=24):
    """9 samples where k_blob_assemble changes shape: no edges (the store's first sample, offset 0), one edge, a source with 63 / 64 / 65
    out-edges, a target with 65 in-edges, three plain ones (the last closes the store)"""
    if ('special', n) not in _STORES:
        g, R = torch.Generator().manual_seed(n), 3
        pairs = [(torch.zeros((2, 0), dtype=torch.long), torch.zeros((0,), dtype=torch.long)), _rand_edges(g, n, R, 1),
                 _hub(g, n, R, 63, True), _hub(g, n, R, 64, True), _hub(g, n, R, 65, True), _hub(g, n, R, 65, False),
                 _rand_edges(g, n, R, 40), _rand_edges(g, n, R, 17), _rand_edges(g, n, R, 30)]
        h = _Host([p[0] for p in pairs], [p[1] for p in pairs], n, R, seed=100 + n)
        assert h.store.edge_count.tolist() == [0, 1, 68, 69, 70, 70, 40, 17, 30] and h.store.off[0] == 0
        assert [int(np.bincount(np.asarray(pairs[i][0][0]), minlength=n).max()) for i in (2, 3, 4)] == [63, 64, 65]
        assert int(np.bincount(np.asarray(pairs[5][0][1]), minlength=n).max()) == 65
        _STORES[('special', n)] = h
    return _STORES[('special', n)]


def _csqa():
    if 'csqa' not in _STORES:
        n = 200
        recs = synthetic.make_records(8, seed=3, shape='csqa', n_rel=17, n_concept_vocab=2000)
        _, cids, nt, ns, al, ei, et, _ = data_utils.records_to_tensors(recs, n, 1)
        h = _Host(ei, et, n, 38, seed=1)
        h.cids, h.nt, h.ns, h.al = cids, nt, ns, al
        h.store = data_utils.GraphBlobStore.build(ei, et, nt, 38, T)
        _STORES['csqa'] = h
    return _STORES['csqa']


def _train_store():
    """12 samples at n = 24: ten of 0..80 edges (every batch of ten lies in the lowest capacity bucket, 1024) and two of 400 / 500"""
    if 'train' not in _STORES:
        g, n, R = torch.Generator().manual_seed(77), 24, 3
        pairs = [_rand_edges(g, n, R, c) for c in (30, 45, 60, 20, 0, 80, 55, 70, 33, 41, 400, 500)]
        _STORES['train'] = _Host([p[0] for p in pairs], [p[1] for p in pairs], n, R, seed=78)
    return _STORES['train']


def _packed(h, ids, nc=1, device=None):
    buf, B, E = h.store.pack(ids)
    return data_utils.PackedGraphBatch(buf if device is None else buf.to(device), B, E, h.store, ids, nc)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
BATCHES = {'B = 1': [4], 'unsorted': [6, 0, 8, 2, 5, 1, 3], 'one id twice': [3, 7, 1, 3, 8, 0, 4], 'reversed': list(range(8, -1, -1))}


@pytest.mark.parametrize('name', list(BATCHES))
def test_fields_and_packed_form_on_the_cpu_equal_host_indexing(name):
    h, ids = _special(), BATCHES[name]
    d = h.device('cpu')
    assert len(d) == 9 and d.nbytes == 4 * h.store.data.size + 8 * 10 + 9 * 24 * (8 + 8 + 4) + 9 * 8
    sb = d.batch(ids, 1)
    assert isinstance(sb, StoreBatch) and sb.ids.dtype == torch.int32 and sb.ids.tolist() == ids and sb.sample_ids == ids
    assert (sb.B, sb.n, sb.n_etype, sb.n_ntype, sb.e_cap) == (len(ids), 24, 3, T, None) and sb.E == int(h.store.edge_count[ids].sum())
    cids, nt, ns, al = sb.fields()
    assert ns.shape == (len(ids), 24, 1)
    for got, want in zip((cids, nt, ns, al), h.fields()):
        assert got.dtype == want.dtype and torch.equal(got, want[ids])
    assert sb.fields()[0] is cids, 'the gather is memoised on the batch'
    assert sb.gathered()[4].tolist() == [0] + np.cumsum(h.store.edge_count[ids]).tolist()
    want = h.store.pack(ids)
    p = sb.to_packed()
    assert (p.B, p.E) == want[1:] and p.buf.dtype == torch.int32 and torch.equal(p.buf, want[0])
    ei, et = sb.batched()
    wei, wet = _packed(h, ids).batched()
    assert torch.equal(ei, wei) and torch.equal(et, wet)


def test_from_host_takes_the_loaders_question_major_shapes():
    h = _train_store()
    flat = h.device('cpu')
    nested = DeviceGraphStore.from_host(h.store, h.cids.view(4, 3, 24), h.nt.view(4, 3, 24), h.ns.view(4, 3, 24, 1), h.al.view(4, 3), 'cpu')
    for name in ('concept_ids', 'node_type_ids', 'node_scores', 'adj_lengths', 'blob_off', 'blobs'):
        assert torch.equal(getattr(flat, name), getattr(nested, name)), name
    assert flat.blob_off.dtype == torch.long and flat.blob_off.tolist() == h.store.off.tolist()


def test_generator_with_a_device_store_yields_what_the_blob_generator_yields():
    h = _train_store()
    nq, nc, n = 4, 3, 24
    d = h.device('cpu')
    g = torch.Generator().manual_seed(5)
    lm = torch.randn(nq, nc, 6, generator=g)
    labels, qids = torch.randint(0, nc, (nq,), generator=g), [f'q{i}' for i in range(nq)]
    nested = [x.view(nq, nc, *x.shape[1:]) for x in h.fields()]
    indexes = torch.tensor([2, 0, 3])  # batches of 2: one full, one partial
    make = lambda **kw: data_utils.MultiGPUSparseAdjDataBatchGenerator(None, 'eval', 'cpu', 'cpu', 2, indexes, qids, labels, tensors0=[lm], **kw)  # noqa: E731
    want = list(make(tensors1=nested, graph_blobs=h.store, num_choice=nc))
    for gen in (make(tensors1=nested, device_store=d), make(device_store=d, num_choice=nc)):
        got = list(gen)
        assert len(got) == len(want) == 2 and len(gen) == 2
        for a, b in zip(got, want):
            assert len(a) == len(b) == 9 and a[0] == b[0] and a[-1] is None and b[-1] is None
            for x, y in zip(a[1:7], b[1:7]):
                assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
            sb, pk = a[7], b[7]
            assert isinstance(sb, StoreBatch) and sb.sample_ids == pk.sample_ids and (sb.B, sb.E, sb.num_choice) == (pk.B, pk.E, nc)
            got_buf, used = sb.to_packed().buf, 2 * (pk.B + 1)  # (words [used, head) are alignment padding pack() leaves unwritten)
            assert torch.equal(got_buf[:used], pk.buf[:used]) and torch.equal(got_buf[pk.head:], pk.buf[pk.head:])
            assert all(torch.equal(x, y) for r, s in zip(sb.nested_lists()[0], pk.nested_lists()[0]) for x, y in zip(r, s))
    assert got[1][7].B == nc  # the partial last batch: one question
    lazy = list(make(tensors1=nested, device_store=d, gather_fields=False))  # ids only: nothing gathered, None in the four places
    for a, b in zip(lazy, want):
        assert a[3:7] == (None,) * 4 and a[7]._gathered is None and a[7].sample_ids == b[7].sample_ids and torch.equal(a[2], b[2])
        assert all(torch.equal(x, y.reshape(x.shape)) for x, y in zip(a[7].fields(), b[3:7]))
    with pytest.raises(ValueError, match='num_choice'):
        make(device_store=d)


def _small_model(R, p=0.0, seed=0):
    torch.manual_seed(seed)
    m = MQ.QAGNN(None, 2, T, R, 64, 2000, 64, 32, 2, 64, 0, p, p, p)
    helpers.det_fill_(m, 9, 0.6)
    if p == 0.0:
        m.pooler.dropout.p = m.pooler.attention.dropout.p = 0.0
    return m


def _inputs(h, ids, nc, device='cpu'):
    g = torch.Generator().manual_seed(len(ids) + sum(ids))
    return dict(sent=torch.randn(len(ids), 64, generator=g).to(device), labels=torch.randint(0, nc, (len(ids) // nc,), generator=g).to(device),
                fields=[x[ids].to(device) for x in h.fields()])


def test_module_on_a_store_batch_equals_the_packed_batch_on_the_emulation_provider():
    from emu_kernels import EmuKernels
    h, ids, nc = _train_store(), [3, 9, 0, 4, 7, 3, 8, 1, 6, 2], 5
    x = _inputs(h, ids, nc)
    d = h.device('cpu')
    old = ops.set_kernels(EmuKernels())
    try:
        outs = []
        for adj, fields in ((_packed(h, ids, nc), x['fields']), (d.batch(ids, nc), None), (d.batch(ids, nc), [None] * 4)):
            m = _small_model(h.R).train()
            logits, attn = m(x['sent'], *(fields if fields is not None else adj.fields()), adj)
            torch.nn.functional.cross_entropy(logits.view(-1, nc), x['labels']).backward()
            outs.append((logits.detach(), attn.detach(), {k: q.grad for k, q in m.named_parameters() if q.grad is not None}))
    finally:
        ops.set_kernels(old)
    for o in outs[1:]:
        assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1])
        assert set(outs[0][2]) == set(o[2]) and len(o[2]) > 10
        assert all(torch.equal(outs[0][2][k], o[2][k]) for k in o[2])


TWIN_IDS = {'A': [5, 7, 2, 9], 'B': [4, 3, 0, 8], 'too large': [10, 11, 5, 7]}  # 251 edges, then 83, then 1050: against a capacity of 300
GRAPH_ARRAYS = ('rowptr_s', 'rowptr_t', 'eid_s', 'tgt_s', 'src_s', 'cls_s', 'src_t', 'tgt_t', 'cls_t', 'pos_t', 'pos_c', 'src_c', 'tgt_c', 'cls_count',
                'chunkptr', 'chunk_cls', 'chunk_beg', 'chunk_len')


def _holder(kind, h, d, ids, e_cap=None):
    """the batch `ids` of the store in one of the three forms graphed.GraphedStep accepts, laid out for `e_cap` edges"""
    if kind == 'store':
        sb = d.batch(ids, 2)
        sb.e_cap = e_cap
        return sb
    packed = _packed(h, ids, 2)
    packed.e_cap = e_cap
    return packed if kind == 'blobs' else data_utils.EdgeListBatch.from_lists(*packed.nested_lists(), h.n, e_cap=e_cap)


@pytest.mark.parametrize('kind', ['edge lists', 'blobs', 'store'])
def test_static_twin_refilled_twice_describes_the_second_batch(kind):
    """What graphed.GraphedStep does around a capture and before every replay, on the CPU: a twin at a capacity above both batches, refilled
    from A and then from B (fewer edges), is B -- in its own fields and in the graph ops.build_graph makes of it."""
    from emu_kernels import EmuKernels
    h, cap = _train_store(), 300
    d = h.device('cpu')
    A, B = _holder(kind, h, d, TWIN_IDS['A']), _holder(kind, h, d, TWIN_IDS['B'])
    assert (A.E, B.E) == (251, 83)
    twin = A.static_twin(4, h.n, cap, torch.device('cpu'))
    assert type(twin) is type(A) and twin.e_cap == cap and twin.capture_kind() == A.capture_kind() == B.capture_kind()
    assert twin.own_fields == (kind == 'store')
    twin.refill(A)
    assert twin.E == A.E
    twin.refill(B)
    assert twin.E == B.E and twin.e_cap == cap
    if kind == 'edge lists':
        assert twin.edge_index.shape == (2, cap) and twin.edge_type.shape == (cap,)
        assert all(torch.equal(x, y) for x, y in zip(twin.pair(), B.pair()))
        assert twin.count.dtype == torch.int32 and twin.count.tolist() == [B.E]
        assert torch.equal(twin.edge_index[:, B.E:A.E], A.edge_index[:, B.E:A.E]), 'the stale tail is left in place: nobody reads it'
    elif kind == 'blobs':
        assert twin.buf.numel() == twin.head + 2 * h.n * 4 + 3 * cap and twin.buf.dtype == torch.int32
        assert torch.equal(twin.buf[:B.buf.numel()], B.buf)
    else:
        assert torch.equal(twin.ids, B.ids) and twin.sample_ids == B.sample_ids and twin.dstore is d
        twin.reset()
        got, want = twin.gathered(), B.gathered()
        assert got[5] is None and want[5] is None and all(torch.equal(x, y) for x, y in zip(got[:5], want[:5]))
    nt = h.nt[TWIN_IDS['B']].reshape(-1)
    old = ops.set_kernels(EmuKernels())
    try:
        g = ops.build_graph(twin, nt, h.R, T, h.n)
        ref = ops.build_graph(_holder(kind, h, d, TWIN_IDS['B'], cap), nt, h.R, T, h.n)
    finally:
        ops.set_kernels(old)
    assert (g.N, g.E, g.n_groups, g.n_chunks, g.max_chunks) == (ref.N, ref.E, ref.n_groups, ref.n_chunks, ref.max_chunks) and g.E == B.E
    for name in GRAPH_ARRAYS:
        assert torch.equal(getattr(g, name), getattr(ref, name)), name
    with pytest.raises(AssertionError):
        twin.refill(_holder(kind, h, d, TWIN_IDS['too large']))
    assert twin.E == B.E


def test_host_refusals():
    h = _special()
    d = h.device('cpu')
    with pytest.raises(ValueError, match='empty'):
        DeviceGraphStore.from_host(data_utils.GraphBlobStore(np.zeros(0, np.int32), [0], [], 24, 3, T), *[x[:0] for x in h.fields()], 'cpu')
    with pytest.raises(AssertionError, match='device1'):
        data_utils.MultiGPUSparseAdjDataBatchGenerator(None, 'eval', 'cpu', 'meta', 2, torch.arange(3), [0, 1, 2], torch.zeros(3), device_store=d, num_choice=3)
    for bad in ([-1], [9], [0, 9, 1], []):
        with pytest.raises(IndexError):
            d.batch(bad, 1)
    off = h.store.off.copy()
    off[4], off[5] = off[5], off[4]  # not monotone
    with pytest.raises(ValueError, match='monotone'):
        DeviceGraphStore.from_host(data_utils.GraphBlobStore(h.store.data, off, h.store.edge_count, 24, 3, T), *h.fields(), 'cpu')
    with pytest.raises(ValueError, match='monotone'):  # does not end at W
        DeviceGraphStore.from_host(data_utils.GraphBlobStore(h.store.data[:-3], h.store.off, h.store.edge_count, 24, 3, T), *h.fields(), 'cpu')
    for i in range(3):  # a node-field tensor with the wrong n
        f = list(h.fields())
        f[i] = torch.cat([f[i], f[i][:, :1]], dim=1)
        with pytest.raises(ValueError, match='n = 24'):
            DeviceGraphStore.from_host(h.store, *f, 'cpu')
    with pytest.raises(ValueError, match='adj_lengths'):
        DeviceGraphStore.from_host(h.store, h.cids, h.nt, h.ns, h.al[:-1], 'cpu')


def test_new_entry_points_are_declared_and_bound():
    from qagnn_amd import _lib
    assert _lib.ABI_VERSION == 25 and len(_lib.EXPORTS) == 63
    assert 'qagnn_store_gather' in _lib.EXPORTS and 'qagnn_graph_from_store' in _lib.EXPORTS
    assert C.sizeof(_lib.qagnn_store) == 6 * 8 + 2 * 4 + 8


# ---------------------------------------------------------------------------------------------------------------------
# GPU, kernel level
# ---------------------------------------------------------------------------------------------------------------------
def hip():
    ops.set_kernels(None)
    return ops.kernels()


def _both_graphs(K, h, d, ids, cap, what):
    """qagnn_graph_from_store on the ids against qagnn_graph_from_blobs on the host-packed batch, both laid out for `cap` edges"""
    packed = _packed(h, ids, device='cuda')
    packed.e_cap = cap
    nt = h.nt[ids].reshape(-1).cuda()
    ref = K.graph_from_blobs(packed, nt)
    sb = d.batch(ids, 1)
    sb.e_cap = cap
    g = K.graph_from_store(sb, sb.fields()[1].reshape(-1))
    assert g.dynamic and g.E == cap and g.keep[1] is sb.ids
    _same_graph(g, ref, packed.E, what)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(BATCHES))
def test_graph_from_store_bit_identical_to_graph_from_blobs(name):
    K = hip()
    h, ids = _special(), BATCHES[name]
    d = h.device('cuda')
    E = int(h.store.edge_count[ids].sum())
    for cap in (E, graphed.edge_capacity(E)):
        _both_graphs(K, h, d, ids, cap, f'{name}, capacity {cap}')


@pytest.mark.gpu
def test_graph_from_store_at_the_csqa_shape():
    K = hip()
    h, ids = _csqa(), [5, 0, 7, 2, 2, 6, 1]
    d = h.device('cuda')
    E = int(h.store.edge_count[ids].sum())
    for cap in (E, graphed.edge_capacity(E)):
        _both_graphs(K, h, d, ids, cap, f'n = 200, R = 38, capacity {cap}')


CANARY = 64  # elements in front of and behind every output of the raw gather call


def _raw_gather(K, d, ids_dev):
    """qagnn_store_gather through the raw binding into outputs cut out of larger, canary-filled buffers -> (the five outputs, err words)"""
    B, n = ids_dev.numel(), d.n
    specs = [((B, n), torch.long), ((B, n), torch.long), ((B, n), torch.float32), ((B,), torch.long), ((B + 1,), torch.int32)]
    bufs, outs = [], []
    for shape, dt in specs:
        numel = int(np.prod(shape))
        buf = torch.full((numel + 2 * CANARY,), -77, dtype=dt, device='cuda')
        bufs.append(buf)
        outs.append(buf[CANARY:CANARY + numel].view(shape))
    err = torch.full((4 + 2 * CANARY,), -77, dtype=torch.int32, device='cuda')
    err[CANARY:CANARY + 4] = 0
    rc = K.lib.qagnn_store_gather(C.byref(K._cstore(d)), ids_dev.data_ptr(), B, *[o.data_ptr() for o in outs], err[CANARY:].data_ptr(), K._stream())
    assert rc == 0, K.lib.qagnn_last_error()
    torch.cuda.synchronize()
    for buf in bufs + [err]:
        assert bool((buf[:CANARY] == -77).all()) and bool((buf[-CANARY:] == -77).all()), 'a canary around an output was overwritten'
    return outs, err[CANARY:CANARY + 4].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize('n', [24, 23])
@pytest.mark.parametrize('B', [1, 300])
def test_store_gather_equals_host_indexing(n, B):
    K = hip()
    h = _special(n)
    d = h.device('cuda')
    ids = [5] if B == 1 else torch.randint(0, 9, (B,), generator=torch.Generator().manual_seed(B)).tolist()
    (cids, nt, ns, al, eoff), err = _raw_gather(K, d, torch.tensor(ids, dtype=torch.int32).cuda())
    assert err == [0, 0, 0, 0]
    for got, want in zip((cids, nt, ns.unsqueeze(2), al), h.fields()):
        assert torch.equal(got.cpu(), want[ids])
    assert eoff.tolist() == [0] + np.cumsum(h.store.edge_count[ids]).tolist()
    sb = d.batch(ids, 1)  # the data layer's call: the same values, memoised
    for got, want in zip(sb.fields(), h.fields()):
        assert got.is_cuda and torch.equal(got.cpu(), want[ids])
    assert sb.fields()[1] is sb.gathered()[1] and torch.equal(sb.gathered()[4], eoff) and sb.gathered()[5].tolist() == [0, 0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize('n', [24, 23])
def test_store_gather_clamps_and_flags_ids_outside_the_store(n):
    K = hip()
    h = _special(n)
    d = h.device('cuda')
    (cids, nt, ns, al, eoff), err = _raw_gather(K, d, torch.tensor([0, 9, -3], dtype=torch.int32).cuda())
    assert err == [1, 0, 0, 0]
    clamped = [0, 8, 0]
    for got, want in zip((cids, nt, ns.unsqueeze(2), al), h.fields()):
        assert torch.equal(got.cpu(), want[clamped])
    assert eoff.tolist() == [0] + np.cumsum(h.store.edge_count[clamped]).tolist()


@pytest.mark.gpu
def test_graph_from_store_clamps_and_flags_an_id_outside_the_store():
    from qagnn_amd import _lib
    K = hip()
    _lib.ERR_WATCH.poll(block=True)
    h = _special()
    d = h.device('cuda')
    clamped = [2, 8, 0]
    packed = _packed(h, clamped, device='cuda')
    ref = K.graph_from_blobs(packed, h.nt[clamped].reshape(-1).cuda())
    sb = StoreBatch(d, clamped, 1, torch.tensor([2, 9, -1], dtype=torch.int32).cuda(), packed.E)  # (batch() refuses such ids on the host)
    nt = sb.fields()[1].reshape(-1)
    with pytest.raises(RuntimeError, match='out-of-range input in the sample ids'):  # the gather reports the ids ...
        _lib.ERR_WATCH.poll(block=True)
    g = K.graph_from_store(sb, nt)
    _same_graph(g, ref, packed.E, 'ids [2, 9, -1]', err0=1)
    with pytest.raises(RuntimeError, match='out-of-range input in the graph of the store batch'):  # ... and so does the assembling kernel
        _lib.ERR_WATCH.poll(block=True)
    _lib.ERR_WATCH.poll(block=True)


@pytest.mark.gpu
def test_raw_calls_refuse_bad_arguments_before_launching():
    from qagnn_amd import _lib
    K = hip()
    h = _special()
    d = h.device('cuda')
    sb = d.batch([1, 2], 1)
    cids, nt, ns, al, eoff, flags = sb.gathered()
    st = K._cstore(d)
    gather = lambda st_, B: K.lib.qagnn_store_gather(st_, sb.ids.data_ptr(), B, cids.data_ptr(), nt.data_ptr(), ns.data_ptr(), al.data_ptr(),  # noqa: E731
                                                     eoff.data_ptr(), flags.data_ptr(), K._stream())
    assert gather(None, 2) != 0 and b'null store' in K.lib.qagnn_last_error()
    assert gather(C.byref(st), 0) != 0 and b'B=0' in K.lib.qagnn_last_error()
    empty = _lib.qagnn_store()
    assert gather(C.byref(empty), 2) != 0 and b'null pointer' in K.lib.qagnn_last_error()
    g = _lib.qagnn_graph()
    storage = torch.full((K.lib.qagnn_graph_storage_elems(48, 8, 3, T),), -7, dtype=torch.int32, device='cuda')
    call = lambda R: K.lib.qagnn_graph_from_store(C.byref(g), storage.data_ptr(), C.byref(st), sb.ids.data_ptr(), eoff.data_ptr(), nt.data_ptr(),  # noqa: E731
                                                  2, 8, R, T, K._stream())
    assert call(4096) != 0 and b'graph_from_store' in K.lib.qagnn_last_error()  # R * T * T = 65536: past the 16-bit class field
    assert call(600) != 0 and b'edge classes' in K.lib.qagnn_last_error()
    sb.e_cap = sb.E - 1
    with pytest.raises(AssertionError, match='capacity'):
        K.graph_from_store(sb, nt.reshape(-1))
    torch.cuda.synchronize()
    assert bool((storage == -7).all()), 'a rejected call wrote to the storage'


@pytest.mark.gpu
def test_blob_offsets_behind_two_to_the_31_words():
    """A store of 2^31 + 8192 int32 words (8.6 GB, uninitialised): one real blob at word 0, two behind word 2^31; the span between is one
    filler sample no batch names.  The batch of the three real samples equals the same batch out of the small store."""
    K = hip()
    if torch.cuda.mem_get_info()[0] < 20e9:
        pytest.skip('needs 20 GB of free device memory')
    h = _special()
    small = h.device('cuda')
    real = [4, 5, 8]
    blobs = [torch.from_numpy(np.array(h.store.sample(i))) for i in real]
    W = 2 ** 31 + 8192
    off = [0, blobs[0].numel(), 2 ** 31 + 5, 2 ** 31 + 5 + blobs[1].numel(), 2 ** 31 + 5 + blobs[1].numel() + blobs[2].numel()]
    assert off[-1] <= W and off[2] > 2 ** 31
    big = torch.empty(W, dtype=torch.int32, device='cuda')
    for o, b in zip((off[0], off[2], off[3]), blobs):
        big[o:o + b.numel()] = b.cuda()
    pick = [real[0], 0, real[1], real[2]]  # (sample 1, the filler, carries some sample's node fields: never read)
    counts = np.array([h.store.edge_count[real[0]], 0, h.store.edge_count[real[1]], h.store.edge_count[real[2]]])
    host = data_utils.GraphBlobStore(np.zeros(0, np.int32), np.array(off), counts, 24, 3, T)
    d = DeviceGraphStore(host, big, torch.tensor(off, dtype=torch.long).cuda(), h.cids[pick].cuda(), h.nt[pick].cuda(),
                         h.ns[pick].reshape(4, 24).cuda(), h.al[pick].cuda())
    sb, want = d.batch([3, 0, 2], 1), small.batch([8, 4, 5], 1)
    assert sb.E == want.E
    for a, b in zip(sb.gathered()[:5], want.gathered()[:5]):
        assert torch.equal(a, b)
    g = K.graph_from_store(sb, sb.fields()[1].reshape(-1))
    ref = K.graph_from_store(want, want.fields()[1].reshape(-1))
    _same_graph(g, ref, sb.E, 'blobs behind word 2^31')
    assert sb.gathered()[5].tolist() == [0, 0, 0, 0]
    del big, d, sb, g
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# GPU, module level
# ---------------------------------------------------------------------------------------------------------------------
NC = 5
TRAIN_IDS = {'captured': [3, 9, 0, 4, 7, 3, 8, 1, 6, 2], 'same bucket': [5, 5, 1, 7, 2, 9, 0, 6, 8, 5], 'fewer edges': [4, 3, 4, 0, 8, 4, 9, 3, 0, 4],
             'next bucket': [10, 11, 3, 9, 0, 4, 10, 7, 1, 2]}


def _eager(model, x, adj, fields, lw=1.0):
    for p in model.parameters():
        p.grad = None
    logits, _ = model(x['sent'], *fields, adj)
    loss = torch.nn.functional.cross_entropy(logits.view(-1, NC), x['labels']) * lw
    loss.backward()
    return _state(model, logits, loss)


@pytest.mark.gpu
def test_eager_step_on_a_store_batch_equals_the_packed_batch():
    hip()
    h, ids = _train_store(), TRAIN_IDS['captured']
    d = h.device('cuda')
    x = _inputs(h, ids, NC, 'cuda')
    want = _eager(_small_model(h.R).cuda().train(), x, _packed(h, ids, NC, 'cuda'), x['fields'])
    for form in ('fields of the batch', 'None'):
        sb = d.batch(ids, NC)
        got = _eager(_small_model(h.R).cuda().train(), x, sb, sb.fields() if form != 'None' else [None] * 4)
        _same(got, want, f'StoreBatch, node fields: {form}')


@pytest.mark.gpu
def test_replay_on_store_batches_is_bit_identical_to_the_eager_step():
    from qagnn_amd import _lib
    hip()
    _lib.ERR_WATCH.poll(block=True)
    h = _train_store()
    d = h.device('cuda')
    E = {k: int(h.store.edge_count[v].sum()) for k, v in TRAIN_IDS.items()}
    caps = {k: graphed.edge_capacity(e) for k, e in E.items()}
    assert caps['captured'] == caps['same bucket'] == caps['fewer edges'] != caps['next bucket'] and E['fewer edges'] < E['captured']
    m_eager, m_graph = _small_model(h.R).cuda().train(), _small_model(h.R).cuda().train()
    step = graphed.GraphedStep(m_graph, NC)
    for i, name in enumerate(('captured', 'same bucket', 'fewer edges', 'captured', 'next bucket')):
        ids = TRAIN_IDS[name]
        x = _inputs(h, ids, NC, 'cuda')
        packed = _packed(h, ids, NC, 'cuda')
        packed.e_cap = caps[name]
        want = _eager(m_eager, x, packed, x['fields'], lw=0.5)
        sb = d.batch(ids, NC)
        fields = [None] * 4 if i % 2 == 0 else sb.fields()
        logits, loss = step(x['sent'], *fields, sb, x['labels'], 0.5)
        _same(_state(m_graph, logits, loss), want, f'call {i}: {name} (E = {E[name]}, capacity {caps[name]})')
        assert step.n_graphs == (1 if name != 'next bucket' else 2)
    torch.cuda.synchronize()
    _lib.ERR_WATCH.poll(block=True)
    assert int(m_graph.gnn.gnn_layers[0].mlp[1].num_batches_tracked) == 5


@pytest.mark.gpu
def test_replays_of_the_same_ids_draw_different_dropout_masks():
    hip()
    h, ids = _train_store(), TRAIN_IDS['captured']
    d = h.device('cuda')
    x = _inputs(h, ids, NC, 'cuda')
    step = graphed.GraphedStep(_small_model(h.R, p=0.2).cuda().train(), NC)
    outs = [step(x['sent'], None, None, None, None, d.batch(ids, NC), x['labels'])[0].clone() for _ in range(3)]
    assert step.n_graphs == 1
    assert not torch.equal(outs[1], outs[2]) and not torch.equal(outs[0], outs[1]), 'the seed epoch did not advance between replays'
