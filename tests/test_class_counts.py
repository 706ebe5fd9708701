"""The admitted node-type and edge-class counts: T = 1 .. 4 node types for the hop and the grouped column reductions, any R > 0 relations with
C = R T^2 + T <= 8192 edge classes for the graph preparation and the edge kernels (include/qagnn_hip.h).  Every other numeric test runs at
T = 4, groups in {1, 4} and C = 548 or 612.

The ladder of (R, T) follows from the constants the class passes rest on, read out of the sources: the strides of the loops over c < C
(64 lanes of k_cls_scatter, 256 threads of k_cls_hist, the 1024-thread blocks of k_chunk_counts), the entries per round of
block_exclusive_scan against pairs = n_groups C, CLS_BLK positions per group, and the limit C <= 8192.  A handful of classes hold exactly
1, 63, 64, 65 and 129 edges (around one and two QAGNN_CLS_CHUNK chunks), nearly every other class is empty.

  * `-m "not gpu"`: the constants are found and the ladder follows from them; every entry holds on EmuGraph what it was built for; the
    comparison helpers reject a grouped sum with a 4-row output whatever `groups`, class ids formed with 4 for T, and a class-table
    gradient whose empty rows were never written -- the first two pass at the counts the suite ran before; the module refuses n_ntype = 5.
  * `-m gpu`: graph preparation bit-exact through all three entry points, edge attention against float64 with canaried outputs, the grouped
    reductions at 2 and 3 groups with a guard row, the row table of the NN products at 1 .. 3 rows, the hop at T = 1, 2, 3 on both dTT
    routes, the module against the oracle.  (test_gemm_tn_group_counts lives in test_hip_kernels.py, where the pinned fp32 family runs it too.)
"""
import ctypes as C
import functools
import os
import types

import pytest
import torch

import helpers
import test_hip_kernels as THK
import test_row_counts as TRC
from emu_kernels import CLS_BLK, CLS_CHUNK, CLS_GROUPS, EmuGraph
from test_hip_kernels import EDGE_OUTPUTS, EMU, EPS, GRAPH_ARRAYS, GUARD, check_edge_outputs, check_grouped_sums, hip, print_figures

# ---- the constants, read from the sources -------------------------------------------------------------------------------------------------
_HDR = os.path.join('..', '..', 'include', 'qagnn_hip.h')
CONSTANT_PATTERNS = dict(
    {k: TRC.CONSTANT_PATTERNS[k] for k in ('SCAN_ITEMS', 'SCAN_THREADS')},
    CLS_BLK=('graph_prep.hip', r'#define CLS_BLK (\d+)'),
    QAGNN_CLS_CHUNK=(_HDR, r'#define QAGNN_CLS_CHUNK (\d+)'),
    QAGNN_CLS_GROUPS=(_HDR, r'#define QAGNN_CLS_GROUPS (\d+)'),
    QAGNN_CLS_SLICES=(_HDR, r'#define QAGNN_CLS_SLICES (\d+)'),
    C_MAX=('graph_prep.hip', r'C64 <= (\d+),'),                                                # (both entry families: the same literal)
    HOP_T_MAX=('hop.hip', r'h->T >= 1 && h->T <= (\d+),'),
    COLREDUCE_GROUPS_MAX=('elementwise.hip', r'groups >= 1 && groups <= (\d+) &&'),
    TN_GROUPS_MAX=('gemm_dispatch.hip', r'p\.groups >= 1 && p\.groups <= (\d+) &&'),
    HIST_STRIDE=('graph_prep.hip', r'for \(int c = threadIdx\.x; c < C; c \+= (\d+)\)'),       # k_cls_hist (both loops: the same literal)
    SCATTER_STRIDE=('graph_prep.hip', r'for \(int c = lane; c < C; c \+= (\d+)\)'),            # k_cls_scatter
    CHUNK_COUNT_THREADS=('graph_prep.hip', r'k_chunk_counts<<<cdiv\(pairs, (\d+)\), \d+, 0, stream>>>'),
)
CONST = {name: TRC._find(name, CONSTANT_PATTERNS) for name in CONSTANT_PATTERNS}


def special_counts(chunk):
    """edges of the classes with an exact count: two chunks + 1, one chunk + 1, one chunk, one chunk - 1, one edge"""
    return [2 * chunk + 1, chunk + 1, chunk, chunk - 1, 1]


Entry = types.SimpleNamespace


def _ladder(c):
    """[(label, R, T, N, E, what it reaches)] from the constants (empty while one is missing: the `not gpu` test names it)"""
    if any(v is None for v in c.values()):
        return []
    scan, cmax, blk, sp = c['SCAN_THREADS'] * c['SCAN_ITEMS'], c['C_MAX'], c['CLS_BLK'], special_counts(c['QAGNN_CLS_CHUNK'])
    below = lambda stride, T: (stride - T - 1) // (T * T)  # noqa: E731  the largest R with R T^2 + T < stride
    small_n, small_e = 37, 400                          # E' = 437: one position group
    rows = [
        ('min', 1, 1, small_n, sp[0], 'C = 2, the minimum: one real class, one self-loop class'),
        ('four_real', 1, 2, small_n, sum(sp[:4]), 'C = 6'),
        ('below_lanes', 3, 3, small_n, small_e, 'C = 30: below one 64-lane stride of k_cls_scatter'),
        ('lanes-1', below(c['SCATTER_STRIDE'], 2), 2, small_n, small_e, 'one class pair below the 64-lane stride'),
        ('lanes+1', below(c['SCATTER_STRIDE'], 2) + 1, 2, small_n, small_e, 'just above the 64-lane stride'),
        ('threads-1', below(c['HIST_STRIDE'], 2), 2, small_n, small_e, 'just below the 256-thread stride of k_cls_hist'),
        ('threads+1', below(c['HIST_STRIDE'], 2) + 1, 2, small_n, small_e, 'just above the 256-thread stride'),
        ('two_blocks', 70, 4, small_n, small_e, 'C above one 1024-thread block of k_chunk_counts, four node types'),
        ('round-2', (cmax - 2) // 4, 2, 40, 500, 'one group; pairs two short of a scan round'),
        ('max', cmax - 1, 1, 40, blk - 40, 'the admitted maximum; E + N = CLS_BLK: one group, pairs exactly one scan round'),
        ('two_groups', scan // 2, 1, 100, blk + 400, 'two groups; pairs two entries into the second scan round'),
        ('max_three_groups', cmax - 1, 1, 200, 2 * blk + 500, 'three groups at the maximum: pairs exactly three scan rounds'),
    ]
    return [Entry(label=l, R=R, T=T, N=N, E=E, C=R * T * T + T, what=w) for l, R, T, N, E, w in rows]


LADDER = _ladder(CONST)
LABELS = [en.label for en in LADDER]
ENTRY = {en.label: en for en in LADDER}


def _build_graph(label):
    """(ei, et, nt, R, T) of a ladder entry: node v has type v % T (every type occurs); the special classes 0, 1, R T^2 / 2, R T^2 - 2 and
    R T^2 - 1 hold exactly special_counts() edges, in that order (with five real classes or fewer: every class, and nothing else); the rest
    of the E edges are spread at random over the other classes, so that nearly all of them stay empty at large C.  An edge of class c =
    r T^2 + a T + b gets relation r, a random source of type a and a random target of type b."""
    en = ENTRY[label]
    R, T, N, E = en.R, en.T, en.N, en.E
    gen = torch.Generator().manual_seed(1000 * R + T)
    RTT, sp = R * T * T, special_counts(CONST['QAGNN_CLS_CHUNK'])
    if RTT <= len(sp):
        classes, counts = list(range(RTT)), sp[:RTT]
        assert E == sum(counts)
        rest = torch.zeros(0, dtype=torch.long)
    else:
        classes, counts = [0, 1, RTT // 2, RTT - 2, RTT - 1], sp
        assert len(set(classes)) == 5 and E >= sum(counts) and N <= 400 and E <= 3000
        rest = torch.randint(0, RTT - 5, (E - sum(counts),), generator=gen)
        for s in sorted(classes):  # skip the special ids
            rest = rest + (rest >= s).long()
    cls = torch.cat([torch.full((n,), c) for c, n in zip(classes, counts)] + [rest])[torch.randperm(E, generator=gen)]
    r, a, b = cls // (T * T), (cls // T) % T, cls % T
    pick = lambda ty: ty + T * (torch.rand(E, generator=gen) * ((N - ty + T - 1) // T)).long().clamp(max=(N - 1 - ty) // T)  # noqa: E731
    nt = torch.arange(N) % T
    ei = torch.stack([pick(a), pick(b)])
    assert bool((nt[ei[0]] == a).all()) and bool((nt[ei[1]] == b).all()) and int(ei.max()) < N
    return ei, r, nt, R, T


graph_of = functools.lru_cache(maxsize=None)(_build_graph)
emu_of = functools.lru_cache(maxsize=None)(lambda label, e_cap=None: EmuGraph(*graph_of(label), e_cap=e_cap))
for _l in LABELS:
    THK.EXTRA_GRAPHS['cc:' + _l] = functools.partial(graph_of, _l)


def expected_class_counts(label):
    """class -> edges, from the construction alone (not from EmuGraph): the special classes, and the self loops of every node type"""
    en = ENTRY[label]
    RTT, sp = en.R * en.T * en.T, special_counts(CONST['QAGNN_CLS_CHUNK'])
    classes = list(range(RTT)) if RTT <= len(sp) else [0, 1, RTT // 2, RTT - 2, RTT - 1]
    want = dict(zip(classes, sp))
    want.update({RTT + t: len(range(t, en.N, en.T)) for t in range(en.T)})
    return want


# ---- the comparison of part 2 (the GPU cases and the `not gpu` checks call the same one) -------------------------------------------------------
class AsLibraryGraph:
    """An EmuGraph behind the accessors of _lib.HipGraph that check_graph reads: the `not gpu` checks hand it wrong graphs as if the library
    had built them."""

    def __init__(self, e, err=(0, 0, 0, 0)):
        self.e, self.N, self.C, self.max_chunks, self.c = e, e.N, e.C, e.max_chunks, types.SimpleNamespace(n_groups=e.n_groups)
        self.words = {'n_chunks': torch.tensor([e.n_chunks], dtype=torch.int32), 'err': torch.tensor(list(err) + e.xcd_base(), dtype=torch.int32)}

    def array(self, name, length):
        t = self.words[name] if name in self.words else getattr(self.e, name).int()
        return t[:length]


def check_graph(g, e, what, err=(0, 0, 0, 0)):
    """Every array of the qagnn_graph contract over its defined range, the chunk tables, n_chunks, cls_count, the flag words and the XCD
    partition of g (a _lib.HipGraph) against EmuGraph e at the same capacity: test_graph_prep_bit_exact's comparison plus
    test_edge_list_capacity._same_graph's flag and partition words."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    assert (g.N, g.C, g.max_chunks, g.c.n_groups) == (e.N, e.C, e.max_chunks, e.n_groups), f'{what}: sizes'
    sizes = {'N+1': e.N + 1, 'Ep': e.Ep, 'C': e.C, 'pairs+1': e.n_groups * e.C + 1}
    for arr, sz in GRAPH_ARRAYS:
        assert torch.equal(g.array(arr, sizes[sz]).cpu(), getattr(e, arr).int()), f'{what}: {arr} differs'
    nch = int(g.array('n_chunks', 1).item())
    assert nch == e.n_chunks, f'{what}: n_chunks'
    for arr in ('chunk_cls', 'chunk_beg', 'chunk_len'):
        assert torch.equal(g.array(arr, nch).cpu(), getattr(e, arr)), f'{what}: {arr} differs'
    words = g.array('err', 13).cpu().tolist()
    assert words[:4] == list(err), f'{what}: flag words {words[:4]}'
    assert words[4:] == e.xcd_base(), f'{what}: XCD partition {words[4:]}'


# ---- the comparison of part 3 ---------------------------------------------------------------------------------------------------------------
CANARY = -7.5


def check_edge_outputs_and_empty_classes(case, got, log=None):
    """check_edge_outputs (the bars of test_edge_attention_forward_backward), and the row of dEk | dEm of every class without an edge is
    exactly 0.0: a class pass that skips empty classes would leave whatever the buffer held."""
    check_edge_outputs(case, got, log)
    empty = case.e.cls_count == 0
    rows = got[4].detach().cpu()[empty]
    assert bool((rows == 0).all()), f'{int((rows != 0).any(1).sum())} of the {int(empty.sum())} rows of dEkEm of classes without an edge are not exactly 0'
    return int(empty.sum())


@functools.lru_cache(maxsize=None)
def edge_case_of(label, HP):
    return THK._build_edge_case('cc:' + label, HP, 'randn')  # (a plain name: the fixed bars EDGE_BARS, nothing added)


# ---- `not gpu` ------------------------------------------------------------------------------------------------------------------------------
def test_the_constants_are_found_and_the_ladder_follows_from_them():
    """`-m "not gpu"`.  A changed constant shows here, by name, not as quietly thinner coverage."""
    missing = [k for k, v in CONST.items() if v is None]
    assert not missing, f'not found in the sources (once, or with one value): {missing}'
    for name, want in dict(SCAN_ITEMS=8, SCAN_THREADS=1024, CLS_BLK=1024, QAGNN_CLS_CHUNK=64, QAGNN_CLS_GROUPS=32, QAGNN_CLS_SLICES=4, C_MAX=8192,
                           HOP_T_MAX=4, COLREDUCE_GROUPS_MAX=4, TN_GROUPS_MAX=4, HIST_STRIDE=256, SCATTER_STRIDE=64, CHUNK_COUNT_THREADS=1024).items():
        assert CONST[name] == want, f'{name} is {CONST[name]}: the ladder of tests/test_class_counts.py was derived for {want}'
    from qagnn_amd import _lib
    from qagnn_amd import modeling_qagnn as MQ
    assert (CLS_CHUNK, CLS_BLK, CLS_GROUPS) == (CONST['QAGNN_CLS_CHUNK'], CONST['CLS_BLK'], CONST['QAGNN_CLS_GROUPS'])  # the emulation's copies
    assert _lib.CLS_SLICES == CONST['QAGNN_CLS_SLICES'] and (MQ.MAX_NTYPE, MQ.MAX_EDGE_CLASSES) == (CONST['HOP_T_MAX'], CONST['C_MAX'])
    assert [(en.R, en.T) for en in LADDER] == [(1, 1), (1, 2), (3, 3), (15, 2), (16, 2), (63, 2), (64, 2), (70, 4), (2047, 2), (8191, 1), (4096, 1), (8191, 1)]
    assert [en.C for en in LADDER] == [2, 6, 30, 62, 66, 254, 258, 1124, 8190, 8192, 4097, 8192]
    assert special_counts(CONST['QAGNN_CLS_CHUNK']) == [129, 65, 64, 63, 1]
    assert all(en.N <= 400 and en.E <= 3000 for en in LADDER) and {en.T for en in LADDER} == {1, 2, 3, 4}
    # the group counts the other tests run (what this file adds to: 2 and 3)
    tn = [m for m in THK.test_gemm_tn_group_counts.pytestmark if m.name == 'parametrize' and m.args[0] == 'groups']
    assert tn[0].args[1] == [2, 3] and GROUPS == [1, 2, 3, 4] and TYPE_COUNTS == [1, 2, 3]


@pytest.mark.parametrize('label', LABELS)
def test_the_ladder_holds_the_counts_it_was_built_for(label):
    """`-m "not gpu"`.  On EmuGraph: C, the position groups, pairs against the scan round, the exact per-class counts, every node type in use,
    and n_chunks against the chunk counts that follow from the construction."""
    en, e = ENTRY[label], emu_of(label)
    ei, et, nt, R, T = graph_of(label)
    scan, blk, chunk = CONST['SCAN_THREADS'] * CONST['SCAN_ITEMS'], CONST['CLS_BLK'], CONST['QAGNN_CLS_CHUNK']
    assert (e.C, e.N, e.E) == (en.C, en.N, en.E) and e.C <= CONST['C_MAX'] and sorted(set(nt.tolist())) == list(range(T))
    assert int(et.max()) < R and int(et.min()) >= 0
    groups = {'two_groups': 2, 'max_three_groups': 3}.get(label, 1)
    assert e.n_groups == groups == -(-e.Ep // blk)
    pairs = e.n_groups * e.C
    want_pairs = {'round-2': scan - 2, 'max': scan, 'two_groups': scan + 2, 'max_three_groups': 3 * scan}
    assert pairs == want_pairs.get(label, pairs) and e.chunkptr.numel() == pairs + 1
    if label == 'max':
        assert e.Ep == blk  # the one position block is full
    if label == 'two_blocks':
        assert CONST['CHUNK_COUNT_THREADS'] < pairs <= 2 * CONST['CHUNK_COUNT_THREADS']
    for stride, lo, hi in ((CONST['SCATTER_STRIDE'], 'lanes-1', 'lanes+1'), (CONST['HIST_STRIDE'], 'threads-1', 'threads+1')):
        assert ENTRY[lo].C == stride - 2 and ENTRY[hi].C == stride + 2
    counts = e.cls_count.tolist()
    for c, n in expected_class_counts(label).items():
        assert counts[c] == n, f'class {c} holds {counts[c]} edges, built for {n}'
    assert sum(counts) == e.Ep
    if e.C > 1000:
        assert sum(1 for n in counts if n == 0) > 0.6 * e.C  # mostly empty
    per_class = sum(-(-n // chunk) for n in counts)  # chunks if every class sat in one group
    nonempty = sum(1 for n in counts if n)
    assert per_class <= e.n_chunks <= per_class + (groups - 1) * nonempty and (groups > 1 or e.n_chunks == per_class)
    assert e.n_chunks <= e.max_chunks
    check_graph(AsLibraryGraph(e), e, label)  # the comparison accepts the emulation itself
    roomy = emu_of(label, en.E + ROOM)
    assert roomy.n_groups == -(-(en.E + ROOM + en.N) // blk) and torch.equal(roomy.cls_s, e.cls_s)
    check_graph(AsLibraryGraph(roomy), roomy, label + ' with room')


def test_the_new_cases_reject_wrong_kernels_the_old_counts_accept():
    """`-m "not gpu"`.  The comparisons the GPU cases call, on three wrong kernels built from the emulation:
      (a) a grouped column sum that writes its four accumulator rows whatever `groups` (a [4][Cc] output): right at groups = 1 (no row
          index: one row) and 4, which is all the suite ran; at 2 and 3 groups it writes the row behind the output -- the guard row;
      (b) class ids formed with 4 in place of T: the very same graph at T = 4 (C = 548 and 612); another one at every T < 4;
      (c) a class-table gradient whose rows of empty classes keep what the buffer held: the canary, or a value below every bar."""
    g = torch.Generator().manual_seed(3)
    X = torch.randn(257, 32, generator=g).double()
    bar = 8 * EPS * X.abs().sum(0).max().item() + 1e-6

    def four_rows(groups, idx):
        buf = torch.full((groups + 1, 32), GUARD, dtype=torch.float64)
        rows = EMU.colsum(X, idx, 4) if idx is not None else EMU.colsum(X)
        n = min(rows.numel(), buf.numel())  # (what of the four rows falls into the buffer and its guard row)
        buf.view(-1)[:n] = rows.view(-1)[:n]
        return buf

    for groups in (1, 4):
        idx = None if groups == 1 else (torch.arange(257) % groups)
        check_grouped_sums(four_rows(groups, idx), EMU.colsum(X, idx, groups), bar, groups, 'old')
    for groups in (2, 3):
        idx = torch.arange(257) % groups
        with pytest.raises(AssertionError, match='behind the'):
            check_grouped_sums(four_rows(groups, idx), EMU.colsum(X, idx, groups), bar, groups, 'new')
    # (b)
    for R in (34, 38):
        ei, et, nt, _, T = THK.rand_graph(R, 50, 300, R=R)
        check_graph(AsLibraryGraph(EmuGraph(ei, et, nt, R, 4)), EmuGraph(ei, et, nt, R, T), f'old, C = {R * 16 + 4}')
    for label in LABELS:
        ei, et, nt, R, T = graph_of(label)
        if T < 4:
            with pytest.raises(AssertionError):
                check_graph(AsLibraryGraph(EmuGraph(ei, et, nt, R, 4)), emu_of(label), label)
    # (c)
    for label in ('below_lanes', 'max'):
        case = edge_case_of(label, 8)
        right = [case.ref[nm].float() for nm in EDGE_OUTPUTS]
        n_empty = check_edge_outputs_and_empty_classes(case, right)
        assert n_empty == int((case.e.cls_count == 0).sum()) > 0
        for stale in (CANARY, 1e-12 * case.ref['dEkEm'].abs().max().item()):
            wrong = list(right)
            wrong[4] = right[4].clone()
            wrong[4][case.e.cls_count == 0] = stale
            with pytest.raises(AssertionError, match='dEkEm'):
                check_edge_outputs_and_empty_classes(case, wrong)


def test_the_module_refuses_five_node_types():
    """`-m "not gpu"`.  n_ntype = 5 (and an edge-class count above 8192) raises at construction -- on every provider, the emulation included,
    which would otherwise compute numbers the library refuses to."""
    from qagnn_amd import modeling_qagnn as MQ
    cfg = helpers.model_cfg(d=28, k=2, sent_dim=40, n_concept=500, concept_in_dim=24)
    build = lambda T, R: MQ.QAGNN(None, cfg['k'], T, R, cfg['sent_dim'], cfg['n_concept'], 28, cfg['concept_in_dim'], 2, 200, 0, 0.0, 0.0, 0.0)  # noqa: E731
    build(4, 38), build(1, 8191)
    for T, R in ((5, 38), (0, 38), (1, 8192), (4, 512)):
        with pytest.raises(NotImplementedError, match='n_ntype'):
            build(T, R)
    with pytest.raises(NotImplementedError, match='n_ntype'):
        MQ.GATConvE(None, 28, 5, 38, None)


# ---- `gpu`: graph preparation ---------------------------------------------------------------------------------------------------------------------
ROOM = 777        # the larger capacity: E + ROOM (another position-group count at most entries)
TAIL = 2 ** 40    # what the unread tail [E, capacity) of the edge buffers holds
EUNSUPPORTED = 2
WAYS = ('blocked', 'cap_exact', 'cap_roomy', 'blobs', 'blobs_roomy')


def _blob_batch(ei, et, nt, R, T):
    from qagnn_amd import data_utils
    store = data_utils.GraphBlobStore.build([ei], [et], nt.view(1, -1), R, T)  # one sample of n = N node slots
    buf, B, E = store.pack([0])
    return data_utils.PackedGraphBatch(buf.cuda(), B, E, store, [0], 1)


def _edge_buffers(ei, et, cap):
    from qagnn_amd import data_utils
    E = ei.size(1)
    ei_b, et_b = torch.full((2, cap), TAIL, dtype=torch.long), torch.full((cap,), TAIL, dtype=torch.long)
    ei_b[:, :E], et_b[:E] = ei, et
    return data_utils.EdgeListBatch(ei_b.cuda(), et_b.cuda(), E, cap)


@pytest.mark.gpu
@pytest.mark.parametrize('way', WAYS)
@pytest.mark.parametrize('label', LABELS)
def test_graph_prep_at_the_class_counts(label, way):
    """qagnn_graph_prep_blocked, qagnn_graph_prep_cap (capacity E and E + 777) and qagnn_graph_from_blobs (GraphBlobStore; at E and at
    E + 777) against EmuGraph at the same capacity: every array, the chunk tables, n_chunks, cls_count, flags 0, the XCD partition."""
    ei, et, nt, R, T = graph_of(label)
    K, E = hip(), ei.size(1)
    cap = E + ROOM if way.endswith('roomy') else (E if way != 'blocked' else None)
    if way == 'blocked':
        g = K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R, T)
    elif way.startswith('cap'):
        g = K.graph_prep_cap(_edge_buffers(ei, et, cap), nt.cuda(), R, T)
    else:
        packed = _blob_batch(ei, et, nt, R, T)
        packed.e_cap = cap
        g = K.graph_from_blobs(packed, nt.cuda())
    check_graph(g, emu_of(label, cap), f'{label}, {way}')


@pytest.mark.gpu
def test_graph_prep_refuses_one_class_too_many():
    """C = 8193 (R = 8192, T = 1): QAGNN_EUNSUPPORTED from all three entry points, before anything is launched -- the storage keeps its marker."""
    from qagnn_amd import _lib
    K = hip()
    R, T, N, E = CONST['C_MAX'], 1, 16, 40
    gen = torch.Generator().manual_seed(1)
    ei, et, nt = torch.randint(0, N, (2, E), generator=gen), torch.randint(0, R, (E,), generator=gen), torch.zeros(N, dtype=torch.long)
    eic, etc, ntc = ei.cuda(), et.cuda(), nt.cuda()
    storage = torch.full((int(K.lib.qagnn_graph_storage_elems(N, E, R, T)),), -7, dtype=torch.int32, device='cuda')
    count = torch.tensor([E], dtype=torch.int32, device='cuda')
    packed = _blob_batch(ei, et, nt, R, T)
    base = packed.buf.data_ptr()
    g = _lib.qagnn_graph()
    calls = {
        'graph_prep': lambda: K.lib.qagnn_graph_prep_blocked(C.byref(g), storage.data_ptr(), eic.data_ptr(), etc.data_ptr(), ntc.data_ptr(), N, E, R, T, 0,
                                                             K._stream()),
        'graph_prep_cap': lambda: K.lib.qagnn_graph_prep_cap(C.byref(g), storage.data_ptr(), eic.data_ptr(), E, etc.data_ptr(), ntc.data_ptr(), N, E,
                                                             count.data_ptr(), R, T, 0, K._stream()),
        'graph_from_blobs': lambda: K.lib.qagnn_graph_from_blobs(C.byref(g), storage.data_ptr(), base + 4 * packed.head, base, base + 4 * (packed.B + 1),
                                                                 ntc.data_ptr(), 1, N, E, R, T, K._stream()),
    }
    for who, call in calls.items():
        assert call() == EUNSUPPORTED and b'8193 edge classes' in K.lib.qagnn_last_error(), (who, K.lib.qagnn_last_error())
    with pytest.raises(RuntimeError, match=r'\(code 2\)'):  # ... and through the binding
        K.graph_prep(eic, etc, ntc, R, T)
    torch.cuda.synchronize()
    assert bool((storage == -7).all()), 'a refused call wrote to the storage'
    K.graph_prep(eic, etc % (R - 1), ntc, R - 1, T)  # one relation fewer is admitted
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize('way', ['blocked', 'cap'])
def test_graph_prep_flags_an_edge_that_leaves_its_block(way):
    """err[1]: a blocked graph (block_n = 20) with one edge from block 0 into block 1.  The flag is set, nothing else changes: every array is
    the emulation's, err[0] stays 0 (the input is in range).  Without the edge the flag stays 0."""
    K = hip()
    gen = torch.Generator().manual_seed(5)
    n, B, R, T = 20, 2, 3, 2
    blk = torch.randint(0, B, (90,), generator=gen) * n
    ei = torch.stack([blk + torch.randint(0, n, (90,), generator=gen), blk + torch.randint(0, n, (90,), generator=gen)])
    et, nt = torch.randint(0, R, (90,), generator=gen), torch.arange(B * n) % T
    for crossing in (False, True):
        if crossing:
            ei[:, 41] = torch.tensor([7, 33])
        if way == 'blocked':
            g = K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R, T, block_n=n)
        else:
            g = K.graph_prep_cap(_edge_buffers(ei, et, 90 + 25), nt.cuda(), R, T, block_n=n)
        assert g.c.block_n == n
        check_graph(g, EmuGraph(ei, et, nt, R, T, n, e_cap=None if way == 'blocked' else 115), f'crossing = {crossing}', err=(0, int(crossing), 0, 0))


# ---- `gpu`: edge attention ----------------------------------------------------------------------------------------------------------------------
def _canary(*shape):
    return torch.full(shape, CANARY, device='cuda')


def run_edge_kernels_into_canaries(case):
    """forward and two backwards through the C ABI into buffers that hold the canary -> (aggr, a, alpha, dKMQ, dEkEm), the second backward's
    (dKMQ, dEkEm)"""
    (ei, et, nt, R, T), HP, DP = case.graph, case.HP, 4 * case.HP
    K = hip()
    g = K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R, T)
    KMQ, EkEm, G = case.KMQ.cuda(), case.EkEm.cuda(), case.G.cuda()
    score, a, alpha, aggr = _canary(g.Ep, 4), _canary(g.Ep, 4), _canary(g.Ep, 4), _canary(g.N, DP)
    rc = K.lib.qagnn_edge_attn_fwd_f32(C.byref(g.c), KMQ.data_ptr(), 3 * DP, EkEm.data_ptr(), 2 * DP, HP, case.qs, score.data_ptr(), a.data_ptr(),
                                       alpha.data_ptr(), aggr.data_ptr(), DP, K._stream())
    assert rc == 0, K.lib.qagnn_last_error().decode()
    runs = []
    for _ in range(2):
        outs = [_canary(g.N, 3 * DP), _canary(g.C, 2 * DP), _canary(g.Ep, 4), _canary(g.N, 4), _canary(g.cls_part_rows, 2 * DP)]
        rc = K.lib.qagnn_edge_attn_bwd_f32(C.byref(g.c), KMQ.data_ptr(), 3 * DP, EkEm.data_ptr(), 2 * DP, HP, case.qs, a.data_ptr(), alpha.data_ptr(),
                                           G.data_ptr(), DP, *[t.data_ptr() for t in outs], K._stream())
        assert rc == 0, K.lib.qagnn_last_error().decode()
        runs.append((outs[0], outs[1]))
    torch.cuda.synchronize()
    return (aggr, a, alpha) + runs[0], runs[1]


@pytest.mark.gpu
@pytest.mark.parametrize('HP', [8, 52])
@pytest.mark.parametrize('label', LABELS)
def test_edge_attention_at_the_class_counts(label, HP):
    """qagnn_edge_attn_{fwd,bwd}_f32 on the ladder's graphs against the float64 emulation under the fixed bars of
    test_edge_attention_forward_backward, every output buffer pre-filled with a canary; the rows of dEk | dEm of empty classes exactly 0;
    a second backward gives the same bits."""
    case, log = edge_case_of(label, HP), []
    try:
        got, again = run_edge_kernels_into_canaries(case)
        n_empty = check_edge_outputs_and_empty_classes(case, got, log)
        assert torch.equal(got[3], again[0]) and torch.equal(got[4], again[1]), 'two backward calls differ in bits'
        assert n_empty == int((case.e.cls_count == 0).sum())
    finally:
        print_figures(f'edge[cc:{label}-{HP}, C = {case.e.C}, {int((case.e.cls_count == 0).sum())} empty classes]', log)


# ---- `gpu`: the grouped reductions --------------------------------------------------------------------------------------------------------------
GROUPS = [1, 2, 3, 4]
COL_ROWS = [5, 257, 1000, 32769]   # one short block; the small form with a ragged tail; 32 blocks; the big form with a one-row last block
COL_WIDTHS = [32, 208, 624]


@pytest.mark.gpu
@pytest.mark.parametrize('Cc', COL_WIDTHS)
@pytest.mark.parametrize('R', COL_ROWS)
def test_grouped_column_sums_at_every_group_count(R, Cc):
    """qagnn_colreduce_f32 mode 0 at groups = 1 .. 4 with a row index that uses every group, with and without row weights, into a
    [groups + 1, Cc] buffer: the sums [groups][Cc] contiguous within 8 eps sum |x| of EMU.colsum in float64, the guard row untouched."""
    gen = torch.Generator().manual_seed(R * 7 + Cc)
    X, w = torch.randn(R, Cc, generator=gen), torch.rand(R, generator=gen) + 0.5
    Xc, wc, K, log = X.cuda(), w.cuda(), hip(), []
    for groups in GROUPS:
        idx = (torch.arange(R) % groups)[torch.randperm(R, generator=gen)]
        j = int((idx == groups - 1).nonzero()[0])
        idx[j], idx[-1] = idx[-1].item(), groups - 1  # the last row (the ragged tail's) in the last group, every group still in use
        assert sorted(set(idx.tolist())) == list(range(min(groups, R)))
        for roww in (None, w):
            buf = torch.full((groups + 1, Cc), GUARD, device='cuda')
            out = K.colsum(Xc, idx.cuda() if groups > 1 else None, groups, roww=None if roww is None else wc, out=buf[:groups])
            assert out.data_ptr() == buf.data_ptr()
            Xw = X.double() if roww is None else X.double() * w.double().unsqueeze(1)
            ref = EMU.colsum(Xw, idx if groups > 1 else None, groups)
            log.append(f'{groups}{"w" if roww is not None else ""} '
                       f'{check_grouped_sums(buf, ref, 8 * EPS * Xw.abs().sum(0).max().item() + 1e-6, groups, f"groups = {groups}, weighted = {roww is not None}"):.2e}')
    print(f'FIGURE colsum_groups[{R}x{Cc}] as fractions of the bound: ' + ' | '.join(log))


@pytest.mark.gpu
@pytest.mark.parametrize('split', [False, True])
@pytest.mark.parametrize('T', [1, 2, 3])
@pytest.mark.parametrize('M,K1,K2,No', [(130, 112, 0, 112), (2000, 208, 112, 624)])
def test_gemm_nn_with_a_row_table_of_1_to_3_rows(M, K1, K2, No, T, split):
    """The bias_tab variant of test_gemm_nn (a 4-row table there) with T = 1, 2, 3 rows, through qagnn_gemm_nn_f32 and
    qagnn_gemm_nn_split_f32, on the same bound."""
    gen = torch.Generator().manual_seed(M + K1 + No + T)
    A1, B1 = torch.randn(M, K1, generator=gen), torch.randn(K1, No, generator=gen)
    A2, B2 = (torch.randn(M, K2, generator=gen), torch.randn(K2, No, generator=gen)) if K2 else (None, None)
    kw = dict(bias=torch.randn(No, generator=gen), rowtab=torch.randn(T, No, generator=gen) * 3, rowidx=torch.arange(M) % T)
    K = hip()
    cu = lambda t: None if t is None else t.cuda()  # noqa: E731
    K.gemm_split = split
    try:
        nk = dict(B1n=cu(B1.t().contiguous()), B2n=cu(B2.t().contiguous()) if K2 else None) if split else {}
        got = K.gemm_nn(cu(A1), cu(B1), cu(A2), cu(B2), **{k: cu(v) for k, v in kw.items()}, **nk).cpu()
    finally:
        K.gemm_split = True
    d = lambda t: None if t is None else (t.double() if t.is_floating_point() else t)  # noqa: E731
    ref = EMU.gemm_nn(d(A1), d(B1), d(A2), d(B2), **{k: d(v) for k, v in kw.items()})
    bound = THK._bound(A1.abs().double(), B1.abs().double())
    if K2:
        bound = bound + 8 * EPS * (A2.abs().double() @ B2.abs().double())
    bound = bound + 4 * EPS * ref.abs()
    err = (got.double() - ref).abs()
    print(f'FIGURE gemm_nn_rowtab[{M}x{K1}+{K2}x{No}, T = {T}, split = {split}]: {(err / bound).max().item():.2e} of the bound')
    assert bool((err <= bound).all()), f'max err {err.max().item():.3e}, worst bound ratio {(err / bound).max().item():.2f}'


# ---- `gpu`: the hop at T = 1, 2, 3 ---------------------------------------------------------------------------------------------------------------
TYPE_COUNTS = [1, 2, 3]
HOP_GRAPHS = [('rand_small', 28, 25), ('degree_ladder', 52, 50)]


def hop_graph(name, T):
    """a graph of test_hip_kernels.GRAPH_CASES with T node types, all in use (R = 38 relations: C = 38 T^2 + T)"""
    ei, et, nt, R, _ = dict(THK.GRAPH_CASES)[name]()
    return ei, et, torch.arange(nt.numel()) % T, R, T


def hop_tab_col(HP, dh, T, route):
    """where the module puts the type indicators: behind the d / 2 live columns of S (modeling_qagnn.node_feature_extra), or -1"""
    h, SP = 2 * dh, THK.side_width(HP)
    assert SP - h >= T
    return h if route == 'rows_of_dWs_t' else -1


@pytest.mark.gpu
@pytest.mark.parametrize('route', ['rows_of_dWs_t', 'colsum'])
@pytest.mark.parametrize('T', TYPE_COUNTS)
@pytest.mark.parametrize('name,HP,dh', HOP_GRAPHS)
def test_fused_hop_equals_composed_path_at_the_type_counts(name, HP, dh, T, route, monkeypatch):
    """The body of test_fused_hop_equals_composed_path (every forward buffer, gradient and running statistic bit-identical) with a T-row
    type table and 38 T^2 + T class rows, on both routes of dTT: rows [tab_col, tab_col + T) of dWs_t, and the grouped column reduction
    with groups = T."""
    tab_col = hop_tab_col(HP, dh, T, route)
    grads = THK.fused_hop_vs_composed(hop_graph(name, T), 1.0 / dh ** 0.5, HP, dh, 'train', monkeypatch, tab_col)
    assert grads['dTT'].shape == (T, 12 * HP) and bool((grads['dTT'].abs().sum(1) > 0).all()), 'a type row of dTT is empty'


def _hop_operands(graph, HP, dh, tab_col):
    """test_head_widths._hop_operands on a graph of T node types (beta = 9 +- 1: no ReLU kink in play, asserted on the reference)"""
    ei, et, nt, R, T = graph
    gen = torch.Generator().manual_seed(77)
    N, DP, Cn, SP = nt.numel(), 4 * HP, R * T * T + T, THK.side_width(HP)
    mask = (torch.arange(DP) % HP < dh).float()
    rnd = lambda *shape, s=0.3: torch.randn(*shape, generator=gen) * s  # noqa: E731
    Wx_t, Ws_t, W1t, W2t = rnd(DP, 3 * DP, s=0.1), rnd(SP, 3 * DP, s=0.1), rnd(DP, DP, s=0.1), rnd(DP, DP, s=0.1)
    X, S, dy = rnd(N, DP, s=1.0), rnd(N, SP, s=1.0), rnd(N, DP, s=1.0)
    if tab_col >= 0:
        S[:, tab_col:tab_col + T] = torch.nn.functional.one_hot(nt, T).float()
        Ws_t[tab_col:tab_col + T] = 0
    prm = [Wx_t, None, Ws_t, None, rnd(T, 3 * DP), rnd(Cn, 2 * DP) * mask.repeat(2), W1t, None, rnd(DP), 1 + rnd(DP), 9 + rnd(DP), W2t, None, rnd(DP),
           rnd(DP), 0.5 + rnd(DP).abs()]
    return prm, X, S, dy


@pytest.mark.gpu
@pytest.mark.parametrize('route', ['rows_of_dWs_t', 'colsum'])
@pytest.mark.parametrize('T', TYPE_COUNTS)
@pytest.mark.parametrize('name,HP,dh', HOP_GRAPHS)
def test_composed_hop_against_float64_at_the_type_counts(name, HP, dh, T, route, monkeypatch):
    """ops.hop_{fwd,bwd}_composed on the library (the path the fused hop is bit-identical to) against the same composition on the emulation
    in float64, train mode, p = 0, by the rule of test_native_hop_against_float64_per_width: per tensor 4 x the error of the float32
    emulation, floored at the fixed forward bar.  dTT on the two routes is the same sum taken two ways: both are held to it."""
    from qagnn_amd import ops
    from test_head_widths import HOP_TENSORS
    from test_nonfinite import FWD, _prm
    graph = hop_graph(name, T)
    ei, et, nt, R, _ = graph
    qs, tab_col = 1.0 / dh ** 0.5, hop_tab_col(HP, dh, T, route)
    prm, X, S, dy = _hop_operands(graph, HP, dh, tab_col)

    def run(K, g, conv, ntype):
        args = (g, HP, qs, conv(X), conv(S), ntype, _prm(prm, conv), True, 1e-5, 0.0, 0, True)
        y, saved = ops.hop_fwd_composed(K, *args, None)
        grads = ops.hop_bwd_composed(K, *args, saved, conv(dy), True, True, None, None, tab_col)
        return [y] + list(saved[:5]) + list(saved[5][:5]) + list(grads)

    e = EmuGraph(ei, et, nt, R, T)
    ref, emu = run(EMU, e, lambda t: t.double(), nt), run(EMU, e, lambda t: t.float(), nt)
    pre = ref[4] * ref[9] + ref[10]
    assert pre.abs().min().item() > 1e-4 * pre.abs().max().item() and (pre > 0).double().mean().item() > 0.999
    K = hip()
    monkeypatch.setattr(K, 'gemm_split', 1)
    got = run(K, K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R, T), lambda t: t.cuda(), nt.cuda())
    torch.cuda.synchronize()
    assert len(ref) == len(emu) == len(got) == len(HOP_TENSORS)
    scale_of = {nm: r.abs().max().item() + 1e-300 for nm, r in zip(HOP_TENSORS, ref)}
    log, failures = [], []
    for nm, a, b, r in zip(HOP_TENSORS, got, emu, ref):
        scale = scale_of['dW1t' if nm == 'db1' else nm]
        err, yard = ((t.detach().cpu().double().reshape(r.shape) - r).abs().max().item() / scale for t in (a, b))
        bar = max(FWD['rtol'] + FWD['atol'] / scale, 4 * yard)
        log.append((nm, err, bar, yard))
        if not torch.isfinite(a).all() or not err <= bar:
            failures.append(f'{nm}: {err:.3e} of scale against {bar:.3e} (f32 {yard:.3e})')
    print_figures(f'hop[{name}-{HP}x{dh}, T = {T}, {route}]', log)
    assert not failures, '; '.join(failures)
    assert got[15].shape == (T, 12 * HP)


@pytest.mark.gpu
@pytest.mark.parametrize('entry', ['hop_fwd', 'hop_bwd'])
def test_hop_refuses_five_node_types(entry):
    """qagnn_hop_{fwd,bwd}_f32 with a 5-row type table: QAGNN_EUNSUPPORTED from check_hop before anything is enqueued -- every saved
    buffer, gradient and workspace element keeps its canary."""
    from test_head_widths import CANARY as HOP_CANARY, _canaried_hop
    K = hip()
    ei, et, nt, R, T = hop_graph('rand_small', 3)
    g, ntc = K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R, T), nt.cuda()
    h, guarded, keep = _canaried_hop(K, g, ntc, 16, entry.endswith('bwd'), T=CONST['HOP_T_MAX'] + 1)
    assert h.T == 5
    rc = getattr(K.lib, f'qagnn_{entry}_f32')(C.byref(h), K._stream())
    torch.cuda.synchronize()
    assert rc == EUNSUPPORTED and b'5 node types' in K.lib.qagnn_last_error(), (rc, K.lib.qagnn_last_error().decode())
    assert all(bool((t == HOP_CANARY).all()) for t in guarded), f'{entry}: a refused call wrote to a buffer'
    assert bool((keep[4] == 123).all())


# ---- the module against the oracle (`gpu`; the CPU twin is in tests/test_host_logic_emu.py) --------------------------------------------------------
# (d, T, R) -> the stack's _tab_col.  d = 28: roundup(14, 16) - 14 = 2 pad columns of S, so T = 1, 2 fit and T = 3, 4 do not -- T sits on the
# boundary of the branch.  d = 100: class tables of 1124 and 601 rows (C > 1024: more than one 1024-thread block of k_chunk_counts).
MODULE_CASES = {(28, 1, 1): 14, (28, 2, 3): 14, (28, 3, 5): -1, (28, 4, 38): -1, (100, 4, 70): 50, (100, 1, 600): 50}


def module_case(d, T, R, train):
    """test_hip_parity.tiny_case with n_ntype = T and n_etype = R; its inputs reach both sides through test_hip_parity.remap_to_counts"""
    return dict(shape='tiny', nq=3, nc=4, n=37, n_rel=17, std=0.6, train=train, seed=31,
                cfg=helpers.model_cfg(d=d, k=3, sent_dim=40, n_concept=500, concept_in_dim=24, n_ntype=T, n_etype=R))


def module_vs_oracle(d, T, R, train, device=None):
    import test_hip_parity as P
    seen = {}
    report = P.oracle_vs_package(module_case(d, T, R, train), device=device, seen=seen)
    (tab_col,) = {m._tab_col for m in seen['model'].modules() if hasattr(m, '_tab_col')}
    assert tab_col == MODULE_CASES[(d, T, R)], (d, T, R, tab_col)
    return report


@pytest.fixture
def form(request):
    yield from helpers.apply_form(request.param)


@pytest.mark.gpu
@pytest.mark.parametrize('d,T,R,train,form', [pytest.param(d, T, R, t, f, id=f'd{d}-T{T}-R{R}-{"train" if t else "eval"}-{f}')
                                              for d, T, R in MODULE_CASES for t in (True, False) for f in helpers.FORMS], indirect=['form'])
def test_oracle_parity_at_the_class_counts(d, T, R, train, form):
    """QAGNN.forward with n_ntype = T, n_etype = R against the CPU oracle: forward at FWD, every gradient on the float64 yardstick, under the
    unchanged bars of F64Ref.check_all (test_oracle_parity_odd_shapes at T = 4, R = 38)."""
    from qagnn_amd import ops
    import test_hip_parity as P
    ops.set_kernels(None)
    try:
        report = module_vs_oracle(d, T, R, train)
        assert ops.kernels().name == 'hip'
    finally:
        ops.set_kernels(None)
    P._report_line(f'module[d={d}, T={T}, R={R}-{"train" if train else "eval"}-{form}]', report)
