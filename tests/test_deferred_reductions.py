"""The stack backward that finishes dEkEm and db1 of all layers after its last hop (include/qagnn_hip_defer.h), and the live-class list the
class reduction of the edge backward takes its blocks from (csrc/graph_prep.hip: k_live_classes).

What is held, all of it bit for bit:
  * qagnn_stack_bwd_deferred_f32 with k = 1, 2, 3 against the same hops run one by one through qagnn_hop_bwd_f32, and against
    qagnn_stack_bwd_f32: every gradient of every layer (dEkEm and db1 among them), dX, dS, the gradients handed from hop to hop, and the
    hops' maximum words.  Every output, workspace and the deferral workspace is pre-filled with NaN; the row of dEkEm of a class without
    an edge must come back as exact zeros.
  * the graphs (DEFER_CASES) sit on the edges of the class reduction: a class with no chunk, classes of one chunk, more chunks than
    partitions in BOTH forms of the flagship width DP = 208 (P = 2 at 256 threads; P = 9 at 1024 threads, where 88 threads of the block
    idle and the rotation of the partitions across groups is no power of two) and at P = 64 (DP = 32), one position group and
    QAGNN_CLS_GROUPS of them, both thread counts of k_cls_reduce (E' below and at 65 536), N = 8 and N one row past the row count at
    which the column reductions change form (tests/test_row_counts.py: CR_SWITCH).  Where each case sits is read from the chunk table:
    the emulated one on the CPU, the prepared graph's own in the GPU test.
  * a stack the deferral cannot serve (more hops than QAGNN_DEFER_MAX_HOPS, hops on two graphs) is refused with its workspace before
    anything is written, and qagnn_stack_bwd_f32 serves it.
  * two deferred backwards in a row over one saved state and ONE deferral workspace, and a captured-then-replayed one: nothing leaks
    from a call into the next.
  * `-m "not gpu"`: the live-class list in the kernel's own order of work (rounds of 1024 classes, ballots per wave) equals numpy.unique
    of the classes present; on the GPU the device list equals the same.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import helpers
from emu_kernels import CLS_BLK, CLS_CHUNK, CLS_GROUPS, EmuGraph
from test_hip_kernels import hip, side_width
from test_row_counts import CONST as ROW_CONST

CR_SWITCH = ROW_CONST['CR_SWITCH']  # rows from which the column reductions take their big form


def _graph(seed, N, E, R, T, R_used=None, hub_class=False):
    """random graph; R_used < R: the relations R_used .. R-1 carry no edge (their classes have no chunk); hub_class: half the edges
    between type-0 nodes with relation 0 -- one class with many chunks"""
    g = torch.Generator().manual_seed(seed)
    src, tgt = torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)
    et = torch.randint(0, R_used or R, (E,), generator=g)
    nt = torch.randint(0, T, (N,), generator=g)
    if hub_class:
        zero = (nt == 0).nonzero().view(-1)
        half = E // 2
        src[:half] = zero[torch.randint(0, zero.numel(), (half,), generator=g)]
        tgt[:half] = zero[torch.randint(0, zero.numel(), (half,), generator=g)]
        et[:half] = 0
    return torch.stack([src, tgt]), et, nt, R, T


# name -> (graph builder, HP, hop counts, form_everywhere).  E' = E + N.
DEFER_CASES = {
    # N = 8, E' = 13: one position group, 256 threads; C = 14 classes of which most have no edge, the others one chunk
    'tiny': (lambda: _graph(11, 8, 5, 3, 2), 4, (1, 2, 3), False),
    # DP = 208, the width whose backward runs the three-MFMA form (the maximum words are live under form_everywhere); E' = 1500: two
    # position groups, 256 threads, P = 2 partitions; the hub class has ~600 edges = 5+ chunks per group; relation 2 carries no edge
    'mid_208': (lambda: _graph(12, 300, 1200, 3, 2, R_used=2, hub_class=True), 52, (1, 2, 3), True),
    # N = CR_SWITCH + 1 rows (the column reductions' big form with a one-row last block), E' = 65 536 exactly: the 1024-thread form of
    # k_cls_reduce (P = 64 partitions at DP = 32) and 64 position blocks in QAGNN_CLS_GROUPS = 32 groups; T = 1: ONE self-loop class of
    # 32 769 edges = 513+ chunks, 128+ in the fullest of the four slices; relation 3 carries no edge
    'switch_64k': (lambda: _graph(13, CR_SWITCH + 1, 65536 - (CR_SWITCH + 1), 4, 1, R_used=3), 8, (2,), False),
    # the class reduction as the flagship batch runs it: DP = 208 (DP2 = 416: 104 float4 columns), E' = 65 536: 1024 threads = 9
    # partitions with threads 936 .. 1023 idle, 14 976 B of dynamic LDS, 32 groups; the hub class holds ~28 800 edges = 450+ chunks,
    # 110+ in every slice; relation 2 carries no edge.  N = 8 000 is below the packed-rows threshold: form_everywhere
    'wide_208': (lambda: _graph(16, 8000, 65536 - 8000, 3, 2, R_used=2, hub_class=True), 52, (2, 3), True),
}
# name -> (position groups, threads of k_cls_reduce, its partitions P, the largest chunk count of a class in one slice against P)
EXPECT = {'tiny': (1, 256, 32, 'one'), 'mid_208': (2, 256, 2, 'more'), 'switch_64k': (CLS_GROUPS, 1024, 64, 'more'),
          'wide_208': (CLS_GROUPS, 1024, 9, 'more')}
CLS_SLICES = 4  # QAGNN_CLS_SLICES (qagnn_amd._lib.CLS_SLICES: asserted below)
CASE_IDS = [f'{nm}-k{k}' for nm, c in DEFER_CASES.items() for k in c[2]]
CASE_PARAMS = [(nm, k) for nm, c in DEFER_CASES.items() for k in c[2]]


def _groups(Ep):
    nblk = -(-Ep // CLS_BLK)
    gb = max(1, -(-nblk // CLS_GROUPS))
    return -(-nblk // gb)


def _cr_partitions(Ep, DP):
    """(threads, P) of k_cls_reduce as launch_cls_reduce (csrc/edge_attn.hip) chooses them"""
    threads = 256 if Ep < 65536 and 2 * DP // 4 <= 128 else 1024
    return threads, threads // (2 * DP // 4)


def where_the_case_sits(chunkptr, n_groups, Cn, Ep, HP):
    """(groups, threads, P, most): `most` = the largest number of chunks one block of k_cls_reduce sums -- a class's chunks in the groups
    g = s, s + S, ... of one slice -- read from the chunk table (chunkptr [n_groups * C + 1])"""
    per_pair = (chunkptr[1:] - chunkptr[:-1]).view(n_groups, Cn).long()
    most = max(int(per_pair[sl::CLS_SLICES].sum(0).max()) for sl in range(min(CLS_SLICES, n_groups)))
    return (n_groups,) + _cr_partitions(Ep, 4 * HP) + (most,)


def check_where(name, groups, threads, P, most):
    g, t, p, rel = EXPECT[name]
    assert (groups, threads, P) == (g, t, p), (name, groups, threads, P)
    assert most == 1 if rel == 'one' else most > P, f'{name}: {most} chunks in the fullest (class, slice) against P = {P}'


# ---- CPU: the live-class list --------------------------------------------------------------------------------------------------------

def live_list_emulation(cls_count):
    """k_live_classes (csrc/graph_prep.hip) step by step: rounds of 1024 classes, one thread per class; a live class's slot is the count of
    the rounds before + the counts of the waves (64 threads) before its own + its rank among the live lanes of its wave"""
    cnt = np.asarray(cls_count)
    Cn, base = cnt.size, 0
    out = np.full(Cn, -1, dtype=np.int64)
    for c0 in range(0, Cn, 1024):
        live = np.zeros(1024, dtype=bool)
        m = min(1024, Cn - c0)
        live[:m] = cnt[c0:c0 + m] > 0
        wc = live.reshape(16, 64).sum(1)
        for t in np.nonzero(live)[0]:
            w, lane = divmod(int(t), 64)
            out[base + wc[:w].sum() + live[w * 64:w * 64 + lane].sum()] = c0 + t
        base += int(wc.sum())
    return out[:base], base


LIVE_GRAPHS = {nm: c[0] for nm, c in DEFER_CASES.items() if nm != 'switch_64k'}
LIVE_GRAPHS.update({
    'all_classes_dead_but_the_loops': lambda: _graph(14, 40, 0, 5, 3),
    # C = 4 x 300 + 2 = 1202 classes: two rounds of the kernel, live classes on both sides of the round boundary and in most waves
    'two_rounds': lambda: _graph(15, 500, 3000, 300, 2),
})


@pytest.mark.parametrize('name', list(LIVE_GRAPHS))
def test_live_class_list_equals_the_classes_present(name):
    """`-m "not gpu"`.  The emulation of the kernel's slots against numpy.unique of the edge classes (self loops included) of the emulated
    graph: ascending, each live class once, the count right; a class is live exactly when it owns a chunk."""
    ei, et, nt, R, T = LIVE_GRAPHS[name]()
    e = EmuGraph(ei, et, nt, R, T)
    want = np.unique(e.ec.numpy())
    got, n = live_list_emulation(e.cls_count.numpy())
    assert n == want.size and np.array_equal(got, want), (n, want.size)
    assert 0 < n <= e.C and (name == 'two_rounds') == (e.C > 1024)
    owns_chunk = np.unique(e.chunk_cls.numpy())
    assert np.array_equal(owns_chunk, want), 'a class is live exactly when it has a chunk'
    assert all(int(x) <= CLS_CHUNK for x in e.chunk_len)


def test_the_cases_sit_where_the_docstring_says():
    """`-m "not gpu"`.  Group counts, thread counts, partitions against chunks and dead classes of DEFER_CASES, each from the chunk table of
    the emulated graph (the GPU test reads the prepared graph's)."""
    from qagnn_amd import _lib
    assert _lib.CLS_SLICES == CLS_SLICES and set(EXPECT) == set(DEFER_CASES)
    for nm, (build, HP, ks, _) in DEFER_CASES.items():
        ei, et, nt, R, T = build()
        e = EmuGraph(ei, et, nt, R, T)
        assert e.n_groups == _groups(e.Ep) and bool((e.cls_count == 0).any())
        check_where(nm, *where_the_case_sits(e.chunkptr, e.n_groups, e.C, e.Ep, HP))
    assert _cr_partitions(65536, 208) == (1024, 9) and 9 * (2 * 208 // 4) == 936  # the flagship form: 88 idle threads
    assert {k for c in DEFER_CASES.values() for k in c[2]} == {1, 2, 3} and 3 in DEFER_CASES['wide_208'][2]


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------

def _nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


class _Stack:
    """k chained hops on one graph after qagnn_stack_fwd_f32, through the raw structs: backward(how) runs the backward into fresh
    NaN-filled buffers and returns every tensor it wrote, the maximum words last."""

    def __init__(self, name, k):
        from qagnn_amd import _lib
        self.lib_mod = _lib
        build, HP, _, _ = DEFER_CASES[name]
        ei, et, nt, R, T = build()
        K = self.K = hip()
        self.k, self.HP, self.DP, self.SP, self.T = k, HP, 4 * HP, side_width(HP), T
        self.g, self.nt = K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R, T), nt.cuda()
        g, DP, SP, N, Ep = self.g, self.DP, self.SP, nt.numel(), ei.size(1) + nt.numel()
        gen = torch.Generator().manual_seed(100 + k)
        rnd = lambda *shape, s=0.1: (torch.randn(*shape, generator=gen) * s).cuda()  # noqa: E731
        self.prms = []
        for _ in range(k):
            Wx_t, Ws_t, W1t, W2t = rnd(DP, 3 * DP), rnd(SP, 3 * DP), rnd(DP, DP), rnd(DP, DP)
            self.prms.append((Wx_t, Wx_t.t().contiguous(), Ws_t, Ws_t.t().contiguous(), rnd(T, 3 * DP), rnd(g.C, 2 * DP), W1t, W1t.t().contiguous(),
                              rnd(DP), 1 + rnd(DP), rnd(DP), W2t, W2t.t().contiguous(), rnd(DP), rnd(DP), 0.5 + rnd(DP).abs()))
        self.X, self.S, self.dy = rnd(N, DP, s=1.0), rnd(N, SP, s=1.0), rnd(N, DP, s=1.0)
        W = _lib.HOP_AMAX_WORDS
        self.saved = (_nan(k, N, 3 * DP), _nan(k, 2, Ep, 4), _nan(k, 4, N, DP), _nan(k, 5, DP))
        self.amax = torch.full((k, W), 0x7F000000, dtype=torch.int32, device='cuda')
        self.ys = self.saved[2][:, 3].unbind(0)
        ws = _nan(int(K.lib.qagnn_hop_fwd_workspace_elems(N, Ep, DP)))
        hops = self._chain(ws)
        assert K.lib.qagnn_stack_fwd_f32(hops, k, K._stream()) == 0, K.lib.qagnn_last_error()
        torch.cuda.synchronize()
        self.dws_elems = int(K.lib.qagnn_stack_bwd_defer_elems(N, DP, g.cls_part_rows, k))
        assert self.dws_elems >= k * g.cls_part_rows * 2 * DP

    def _chain(self, ws):
        return self.K._hop_chain(self.g, self.HP, 0.25, self.X, self.S, self.nt, self.prms, self.ys, self.saved, self.amax.data_ptr(), None, None, ws,
                                 True, 1e-5, 0.0, [0] * self.k, -1)

    def buffers(self):
        """fresh NaN-filled gradient buffers and workspace, and the hops chained onto them (as _lib.HipKernels.stack_bwd chains them)"""
        K, g, k, DP, SP, N = self.K, self.g, self.k, self.DP, self.SP, self.g.N
        sizes, offs = K._grad_sizes(DP, SP, self.T, g.C)
        per = offs[-1]
        flat, dxs, dS, dX = _nan(k * per), _nan(max(k - 1, 1), N, DP), _nan(N, SP), _nan(N, DP)
        ws = _nan(int(K.lib.qagnn_hop_bwd_workspace_elems(N, g.Ep, DP, SP, g.cls_part_rows)))
        hops = self._chain(ws)
        carved = []
        W, p_amax = self.lib_mod.HOP_AMAX_WORDS, self.amax.data_ptr()
        for l, h in enumerate(hops):
            h.dy = self.dy.data_ptr() if l == k - 1 else dxs.data_ptr() + l * N * DP * 4
            carved.append(K._carve_grads(h, flat[l * per:(l + 1) * per], sizes, offs, g.C))
            h.dX, h.accumulate_dX = (dxs.data_ptr() + (l - 1) * N * DP * 4, 0) if l > 0 else (dX.data_ptr(), 0)
            h.dS, h.accumulate_dS = dS.data_ptr(), (0 if l == k - 1 else 1)
            if l > 0:  # the words the stack shares along its chain (csrc/hop.hip: hop_amax_stack), named, so that a hop run alone reads them too
                h.x_amax = p_amax + ((l - 1) * W + self.lib_mod.HOP_AM_Y) * 4
                h.s_amax = p_amax + self.lib_mod.HOP_AM_S * 4
        return hops, carved, dict(flat=flat, dxs=dxs, dS=dS, dX=dX), ws

    def launch(self, how, hops, dws=None):
        K, k = self.K, self.k
        if how == 'hops':
            for l in range(k - 1, -1, -1):
                assert K.lib.qagnn_hop_bwd_f32(C.byref(hops[l]), K._stream()) == 0, K.lib.qagnn_last_error()
        elif how == 'stack':
            assert K.lib.qagnn_stack_bwd_f32(hops, k, K._stream()) == 0, K.lib.qagnn_last_error()
        else:
            assert K.lib.qagnn_stack_bwd_deferred_f32(hops, k, dws.data_ptr(), dws.numel(), K._stream()) == 0, K.lib.qagnn_last_error()

    def backward(self, how):
        hops, carved, out, ws = self.buffers()
        dws = _nan(self.dws_elems) if how == 'deferred' else None
        self.launch(how, hops, dws)
        torch.cuda.synchronize()
        out['amax'] = self.amax.clone()
        out['dEkEm'] = [c[3] for c in carved]
        out['db1'] = [c[5] for c in carved]
        return out


def _same(got, want, what):
    n = 0
    for nm in ('flat', 'dxs', 'dS', 'dX', 'amax'):
        a, b = helpers._bits(got[nm]), helpers._bits(want[nm])
        assert torch.equal(a, b), f'{what}: {nm}: {int((a != b).sum())} of {a.numel()} elements differ'
        n += a.numel()
    return n


@pytest.mark.gpu
@pytest.mark.parametrize('name,k', CASE_PARAMS, ids=CASE_IDS)
def test_deferred_stack_backward_equals_the_hops_one_by_one(name, k):
    """qagnn_stack_bwd_deferred_f32 against k calls of qagnn_hop_bwd_f32 and against qagnn_stack_bwd_f32, from NaN-filled buffers: all bits
    equal, the maximum words equal; the rows of dEkEm of the classes without an edge are exact zeros, the others and db1 hold no NaN."""
    form = DEFER_CASES[name][3]
    with helpers.form_everywhere() if form else contextlib.nullcontext():
        st = _Stack(name, k)
        want = st.backward('hops')
        plain = st.backward('stack')
        got = st.backward('deferred')
    n = _same(plain, want, 'qagnn_stack_bwd_f32 against the hops one by one')
    _same(got, want, 'the deferred stack against the hops one by one')
    dead = (st.g.cls_count == 0).cpu()
    assert bool(dead.any()) and not bool(dead.all())
    for l in range(k):
        dE = got['dEkEm'][l].cpu()
        assert torch.equal(dE[dead].view(torch.int32), torch.zeros_like(dE[dead]).view(torch.int32)), f'layer {l}: a dead class row is not +0.0'
        assert bool(torch.isfinite(dE).all()) and bool(torch.isfinite(got['db1'][l]).all())
        assert bool((dE[~dead].abs().amax(1) > 0).all()), f'layer {l}: a live class without a gradient'
    words = got['amax'][:, st.lib_mod.HOP_AM_DKMQ].tolist()
    assert not form or all(0 < w < 0x7F000000 for w in words), f'the backward maxima {words}: the three-MFMA form did not run'
    live, n_live = st.g.live_classes()
    want_live = np.nonzero(~dead.numpy())[0]
    assert int(n_live) == want_live.size and np.array_equal(live[:want_live.size].cpu().numpy(), want_live)
    # where the case sits, from the chunk table the kernels walked
    NG = int(st.g.c.n_groups)
    sits = where_the_case_sits(st.g.array('chunkptr', NG * st.g.C + 1).cpu(), NG, st.g.C, st.g.Ep, st.HP)
    check_where(name, *sits)
    print(f'FIGURE deferred[{name}-k{k}]: {n} elements equal three ways; {want_live.size} of {st.g.C} classes live; (groups, threads, P, most '
          f'chunks per block) = {sits}; words {[hex(w) for w in words]}')


EUNSUPPORTED = 2


@pytest.mark.gpu
@pytest.mark.parametrize('why', ['too_many_hops', 'two_graphs'])
def test_a_stack_the_deferral_cannot_serve_is_refused_before_anything_is_written(why):
    """QAGNN_DEFER_MAX_HOPS + 1 hops, and two hops on two (equal) prepared graphs: with a deferral workspace QAGNN_EUNSUPPORTED and every
    NaN-filled output, workspace and maximum word as it was; qagnn_stack_bwd_f32 serves the same stack, equal to the hops one by one."""
    from qagnn_amd import _lib
    k = _lib.DEFER_MAX_HOPS + 1 if why == 'too_many_hops' else 2
    st = _Stack('tiny', k)
    hops, carved, out, ws = st.buffers()
    keep = None
    if why == 'two_graphs':
        ei, et, nt, R, T = DEFER_CASES['tiny'][0]()
        keep = st.K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R, T)
        hops[1].g = C.pointer(keep.c)
    dws = _nan(max(st.dws_elems, 16))
    words = st.amax.clone()
    rc = st.K.lib.qagnn_stack_bwd_deferred_f32(hops, k, dws.data_ptr(), dws.numel(), st.K._stream())
    torch.cuda.synchronize()
    assert rc == EUNSUPPORTED, (rc, st.K.lib.qagnn_last_error())
    assert all(bool(torch.isnan(t).all()) for t in list(out.values()) + [ws, dws]) and torch.equal(st.amax, words), 'the refused call wrote'
    assert st.K.lib.qagnn_stack_bwd_f32(hops, k, st.K._stream()) == 0, st.K.lib.qagnn_last_error()
    torch.cuda.synchronize()
    out['amax'] = st.amax.clone()
    if why == 'two_graphs':
        hops[1].g = hops[0].g
    _same(out, st.backward('hops'), f'qagnn_stack_bwd_f32 on the refused stack ({why})')


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tiny', 'mid_208'])
def test_two_deferred_backwards_in_a_row_share_nothing(name):
    """Over one saved state, ONE deferral workspace and one set of gradient buffers: a backward of dy, then one of another gradient.  The
    second equals that gradient's backward from fresh NaN-filled buffers."""
    with helpers.form_everywhere():
        st = _Stack(name, 2)
        dy2 = (torch.randn(st.dy.shape, generator=torch.Generator().manual_seed(5)) * 0.37).cuda()
        hops, carved, out, ws = st.buffers()
        dws = _nan(st.dws_elems)
        st.launch('deferred', hops, dws)
        first = st.dy.clone()
        st.dy.copy_(dy2)  # (the hops hold dy's address)
        st.launch('deferred', hops, dws)
        torch.cuda.synchronize()
        out['amax'] = st.amax.clone()
        want = st.backward('deferred')
        st.dy.copy_(first)
        other = st.backward('deferred')
    _same(out, want, 'the second of two backwards')
    assert not torch.equal(helpers._bits(other['flat']), helpers._bits(want['flat'])), 'the two gradients give one result: nothing was tested'


@pytest.mark.gpu
def test_captured_deferred_backward_replays_to_the_eager_bits():
    """The deferred stack backward captured into a graph (one stream, no fork) and replayed twice, the second time on another dy: each replay
    equals the eager call on that dy."""
    with helpers.form_everywhere():
        st = _Stack('mid_208', 2)
        dy1 = st.dy.clone()
        dy2 = (torch.randn(st.dy.shape, generator=torch.Generator().manual_seed(6)) * 0.37).cuda()
        want1 = st.backward('deferred')
        st.dy.copy_(dy2)
        want2 = st.backward('deferred')
        st.dy.copy_(dy1)
        hops, carved, out, ws = st.buffers()
        dws = _nan(st.dws_elems)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # (a run outside the capture, on a side stream, as torch's capture recipe asks)
            st.launch('deferred', hops, dws)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for t in out.values():
            t.fill_(float('nan'))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            st.launch('deferred', hops, dws)
        graph.replay()
        torch.cuda.synchronize()
        out['amax'] = st.amax.clone()
        _same(out, want1, 'first replay')
        st.dy.copy_(dy2)
        graph.replay()
        torch.cuda.synchronize()
        out['amax'] = st.amax.clone()
        _same(out, want2, 'second replay, another dy')
