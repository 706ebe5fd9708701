"""The two-operand weight gradient [X | S]^T dK|dM|dQ balanced by LIVE k-tiles (csrc/common.h: tn_work, csrc/gemm_split.hip:
k_gemm_tn_ws<.., LIVE>, csrc/graph_prep.hip: k_live_tiles).

A 32-row k-tile is live if one of its node rows has an edge besides its self loop; in a dead tile dK = dQ = 0 exactly, so the K and Q
column blocks of the product walk lists of live tiles and the M block ranges of all tiles, the chunk slots divided so that every block
walks about the same number of tiles.  Held here: the flags, the partition (downloaded as the kernels compute it), and the product
itself at the smallest row count the dispatch sends down that route (asked from the library, not written down) and 17 rows above it
(a ragged last tile), in the six-MFMA and the three-MFMA form, on the bounds tests/test_hip_kernels.py holds the same entry points to:
    six MFMAs   (test_gemm_tn_two_operands)     |err| <= 16 eps |A|^T |B| + 1e-6
    three MFMAs (test_gemm_tn_three_mfma_form)  |err| <= 16 eps |A|^T |B| + 2^-38 R max|A_operand| max|B| + 1e-30
(the header of csrc/gemm_nn2.hip derives the second).  Operands are filled on the device and the float64 products taken there."""
import numpy as np
import pytest
import torch

from test_hip_kernels import EPS, hip, side_width

KA1, KA2, NO, DP = 208, 112, 624, 208
WS = 3  # TnFamily::WS in qagnn_gemm_tn_route_query's out[0]


# ---- graphs with a chosen set of lone rows ---------------------------------------------------------------------------------------
def ring_edges(lone):
    """edge list [2, E] that gives every row outside `lone` (bool [N]) an out- and an in-edge besides its self loop: a ring over those
    rows (a single such row gets a real edge onto itself)"""
    idx = torch.nonzero(~lone).flatten()
    return torch.stack([idx, torch.roll(idx, -1)])


def cpu_flags(ei, N):
    """live[t] from the edge list alone: some row of the tile has an out- or in-edge (rows past N have none)"""
    T = (N + 31) // 32
    busy = np.zeros(T * 32, dtype=bool)
    busy[ei.cpu().numpy().ravel()] = True
    return busy.reshape(T, 32).any(1).astype(np.int32)


def runs_mask():
    """runs of lone rows of 31 .. 65 rows starting 0, 1 and 31 rows into a tile, each in a window of five tiles; N no multiple of 32"""
    N = 18 * 160 + 7
    lone = torch.zeros(N, dtype=torch.bool)
    w = 0
    for length in (31, 32, 33, 63, 64, 65):
        for off in (0, 1, 31):
            lone[w * 160 + 32 + off: w * 160 + 32 + off + length] = True
            w += 1
    return lone


def bench_like_mask(N, n=200):
    """subgraphs of n rows whose tails of 1 .. 160 rows are lone (the PAD rows of a CommonsenseQA batch)"""
    row = torch.arange(N)
    tail = 1 + (row // n * 37) % 160
    return row % n >= n - tail


def one_live_mask(N, tile):
    lone = torch.ones(N, dtype=torch.bool)
    lone[tile * 32 + 3: min(N, tile * 32 + 5)] = False  # (two rows of the tile, or the one row a ragged last tile may have)
    lone[min(N - 1, tile * 32 + 3)] = False
    return lone


SMALL_MASKS = {'runs': runs_mask, 'none': lambda: torch.zeros(1000, dtype=torch.bool), 'all': lambda: torch.ones(1000, dtype=torch.bool),
               'ragged': lambda: bench_like_mask(3 * 200 + 13), 'bench_like': lambda: bench_like_mask(160 * 200)}


def prep(K, lone):
    N = lone.numel()
    ei = ring_edges(lone).cuda()
    et = torch.zeros(ei.size(1), dtype=torch.long, device='cuda')
    g = K.graph_prep(ei, et, torch.zeros(N, dtype=torch.long, device='cuda'), 2, 2)
    return g, ei


def graph_live(g):
    live, lst, n_live = g.live_tiles()
    return live.cpu().numpy(), lst.cpu().numpy(), int(n_live.item())


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(SMALL_MASKS))
def test_live_tile_flags_and_list(name):
    """qagnn_graph.live_tiles == the flags computed from the edge list on the CPU, exactly; live_list = the live tiles ascending, then the
    dead ones ascending; n_live their count."""
    K = hip()
    lone = SMALL_MASKS[name]()
    g, ei = prep(K, lone)
    ref = cpu_flags(ei, lone.numel())
    live, lst, L = graph_live(g)
    assert live.size == lst.size == (lone.numel() + 31) // 32 == ref.size
    assert np.array_equal(live, ref), np.nonzero(live != ref)[0][:10]
    assert L == int(ref.sum())
    assert np.array_equal(lst, np.concatenate([np.nonzero(ref)[0], np.nonzero(ref == 0)[0]]))
    if name == 'none':
        assert L == ref.size
    if name == 'all':
        assert L == 0
    if name == 'runs':  # whole tiles inside the runs: from offset 0 0|1|1|1|2|2, from 1 0|0|0|1|1|1, from 31 0|0|1|1|1|2 (lengths 31 .. 65)
        assert int((ref == 0).sum()) == 7 + 3 + 5


def check_table(tab, live, lst, S, chunk_tiles):
    """the invariants of the work table (qagnn_tn_work_table) against the graph's flags"""
    cK, cM, T, L = (int(v) for v in tab[:4])
    units = tab[4:].reshape(S, 5)
    assert T == live.size and L == int(live.sum()) and cM + 2 * cK == S and cK >= 1 and cM >= 1
    assert sorted(units[:, 4].tolist()) == list(range(S)), 'the units are no bijection onto the partial tiles'
    m_cover = np.zeros(T, dtype=int)
    kq_cover = {0: np.zeros(T, dtype=int), 2: np.zeros(T, dtype=int)}
    kq_len = {0: [], 2: []}
    for cb, is_list, beg, cnt, pslot in units.tolist():
        assert cb == (0 if pslot < cK else 2 if pslot < 2 * cK else 1)
        assert cnt >= 0 and beg >= 0 and beg + cnt <= T
        if cb == 1:
            assert not is_list
            m_cover[beg:beg + cnt] += 1
        else:
            tiles = lst[beg:beg + cnt] if is_list else np.arange(beg, beg + cnt)
            np.add.at(kq_cover[cb], tiles, 1)
            kq_len[cb].append(cnt)
            assert bool(is_list) == (L < T)
    assert (m_cover == 1).all(), 'every tile lies in exactly one M range'
    for cb in (0, 2):
        assert np.array_equal(kq_cover[cb], live), 'every live tile once in the K and once in the Q lists, no dead tile'
        assert len(kq_len[cb]) == cK
        if L < T:
            assert max(kq_len[cb]) - min(kq_len[cb]) <= 1
    if L == T:  # the partition of the launch without a table: S / 3 chunks of chunk_tiles for every column block
        assert cK == cM == S // 3
        for cb, is_list, beg, cnt, pslot in units.tolist():
            j = pslot - {0: 0, 2: cK, 1: 2 * cK}[cb]
            assert beg == min(j * chunk_tiles, T) and cnt == min(chunk_tiles, T - beg)
    else:  # cK = clamp(round(S L / (T + 2 L)), 1, (S - 1) / 2)
        assert cK == min(max((2 * S * L + T + 2 * L) // (2 * (T + 2 * L)), 1), (S - 1) // 2)
    return cK, cM


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(SMALL_MASKS))
def test_work_table_invariants(name):
    K = hip()
    g, _ = prep(K, SMALL_MASKS[name]())
    live, lst, L = graph_live(g)
    T = live.size
    for S in (9, 27, 84, 162):
        if T < S // 3:
            continue
        ct = -(-T // (S // 3))
        check_table(K.tn_work_table(g, S, ct).cpu().numpy(), live, lst, S, ct)


# ---- the product at the first row count of the route ----------------------------------------------------------------------------
_R0 = []


def first_ws_rows(K):
    """the smallest R the dispatch sends down the k_gemm_tn_ws route for (208, 112, 624): the route is monotone in R from the first long
    chunk on, so a bisection over the library's host-side answer finds it"""
    if not _R0:
        fam = lambda R: K.tn_route_query(R, KA1, KA2, NO)[0]  # noqa: E731
        lo, hi = 1024, 64000
        assert fam(lo) != WS and fam(hi) == WS
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if fam(mid) == WS else (mid, hi)
        assert fam(hi) == WS and fam(hi - 1) != WS and K.tn_route_query(hi, KA1, KA2, NO)[3] == 1
        _R0.append(hi)
    return _R0[0]


_OPS = {}


def operands(R):
    """A1, A2, B on the device (filled there), with |A| in float64 for the bounds -- once per row count, never changed"""
    if R not in _OPS:
        gen = torch.Generator(device='cuda').manual_seed(R)
        A1 = torch.randn(R, KA1, generator=gen, device='cuda')
        A2 = torch.randn(R, KA2, generator=gen, device='cuda') * 3.0
        B = torch.randn(R, NO, generator=gen, device='cuda') * 1e-3
        A64 = torch.cat([A1, A2], 1).double()
        _OPS[R] = (A1, A2, B, A64)
    return _OPS[R]


def masked_b(B, live):
    """B with its K and Q columns zero in every row of a dead tile -- exactly where the flags say so, nowhere else"""
    R = B.size(0)
    dead_row = torch.from_numpy(np.repeat(live == 0, 32)[:R]).cuda()
    Bm = B.clone()
    Bm[dead_row, :DP] = 0
    Bm[dead_row, 2 * DP:] = 0
    return Bm


def bound_of(np_, A1, A2, A64, B):
    absprod = A64.abs().t() @ B.double().abs()
    if np_ == 3:
        return 16 * EPS * absprod + 1e-6
    arow = torch.cat([torch.full((KA1,), A1.abs().max().item()), torch.full((KA2,), A2.abs().max().item())]).double().cuda()
    return 16 * EPS * absprod + 2.0 ** -38 * B.size(0) * arow[:, None] * B.abs().max().item() + 1e-30


def run_product(K, np_, A1, A2, B, graph):
    amax = None if np_ == 3 else (K.absmax(A1), K.absmax(A2), K.absmax(B))
    return K.gemm_tn_graph(A1, A2, B, graph=graph, pieces=np_, amax=amax)


PATTERNS = ['none', 'all', 'one_first', 'one_last_full', 'one_tail', 'bench_like']


@pytest.mark.gpu
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('extra', [0, 17])
@pytest.mark.parametrize('np_', [3, 2])
def test_product_on_live_tiles(np_, extra, pattern):
    K = hip()
    R = first_ws_rows(K) + extra
    fam, chunk_rows, nchunks, live_route = K.tn_route_query(R, KA1, KA2, NO)
    assert fam == WS and live_route == 1
    T = (R + 31) // 32
    lone = {'none': lambda: torch.zeros(R, dtype=torch.bool), 'all': lambda: torch.ones(R, dtype=torch.bool),
            'one_first': lambda: one_live_mask(R, 0), 'one_last_full': lambda: one_live_mask(R, R // 32 - 1),
            'one_tail': lambda: one_live_mask(R, T - 1), 'bench_like': lambda: bench_like_mask(R)}[pattern]()
    g, ei = prep(K, lone)
    live, lst, L = graph_live(g)
    assert np.array_equal(live, cpu_flags(ei, R))
    assert L == {'none': T, 'all': 0, 'bench_like': L}.get(pattern, 1)
    if pattern == 'bench_like':
        assert 0.5 * T < L < 0.9 * T, (L, T)  # (a quarter of the tiles dead, as on the training batch)
    cK, cM = check_table(K.tn_work_table(g, 3 * nchunks, chunk_rows // 32).cpu().numpy(), live, lst, 3 * nchunks, chunk_rows // 32)
    A1, A2, B, A64 = operands(R)
    Bm = masked_b(B, live)
    got = run_product(K, np_, A1, A2, Bm, g)
    ref = A64.t() @ Bm.double()
    bound = bound_of(np_, A1, A2, A64, Bm)
    err = (got.double() - ref).abs()
    print(f'np={np_} R={R} {pattern}: T={T} L={L} cK={cK} cM={cM} max err {err.max().item():.3e} worst bound ratio {(err / bound).max().item():.3f}')
    assert torch.isfinite(got).all()
    assert bool((err <= bound).all()), f'max err {err.max().item():.3e}, worst bound ratio {(err / bound).max().item():.2f}'
    again = run_product(K, np_, A1, A2, Bm, g)
    assert torch.equal(got, again), 'two calls on the same graph differ'
    plain = run_product(K, np_, A1, A2, Bm, None)
    if pattern == 'none':  # no dead tile: the partition, hence every bit, of the call without a graph
        assert torch.equal(got, plain)
    else:
        assert not torch.equal(got, plain), 'the live-tile form did not run'
        assert bool(((plain.double() - ref).abs() <= bound).all())
    if pattern == 'all':  # empty lists: partials of exact +0 (the bit pattern, not only the value)
        kq = torch.cat([got[:, :DP], got[:, 2 * DP:]], 1)
        assert bool((kq.view(torch.int32) == 0).all())
        assert got[:, DP:2 * DP].abs().max().item() > 0
    old = K.tn_live_tiles(0)  # the switch: the graph is ignored
    try:
        assert K.tn_route_query(R, KA1, KA2, NO)[3] == 0
        assert torch.equal(run_product(K, np_, A1, A2, Bm, g), plain)
    finally:
        K.tn_live_tiles(old)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [2, 1])
def test_native_hop_backward_on_live_tiles(mode, monkeypatch):
    """qagnn_hop_bwd_f32 at the smallest N on the route, on a batch-like graph: dWx_t | dWs_t (the node-type rows of dWs_t = dTT included)
    with the live tiles against the same hop with the table withheld (qagnn_tn_live_tiles(0)): each within its form's float64 bound of
    [X | S]^T dKMQ, so at most two bounds apart.  mode = gemm_split: 2 the three-MFMA form (gradient-sized dy), 1 the six-MFMA form.
    dKMQ, which the hop keeps in its workspace, is rebuilt from the saved forward tensors with the per-kernel entry points
    (ops.hop_bwd_composed's first steps): in mode 1 that is the hop's dKMQ bit for bit (test_fused_hop_equals_composed_path), and both runs
    are also held to the float64 product; in mode 2 it is the hop's to round-off, which is all the SIZE of the bound needs."""
    from qagnn_amd import ops
    K = hip()
    monkeypatch.setattr(K, 'gemm_split', mode)
    N = first_ws_rows(K)
    HP, Tn, Rr = 52, 4, 3
    SP, Cc = side_width(HP), Rr * Tn * Tn + Tn
    lone = bench_like_mask(N)
    ei = ring_edges(lone)
    gen = torch.Generator().manual_seed(5)
    busy = torch.nonzero(~lone).flatten()
    extra = torch.randint(0, busy.numel(), (2, 3 * N), generator=gen)
    ei = torch.cat([ei, busy[extra]], 1).cuda()  # more edges among the rows that have some (lone rows stay lone)
    et = torch.randint(0, Rr, (ei.size(1),), generator=gen).cuda()
    ntype = torch.randint(0, Tn, (N,), generator=gen).cuda()
    g = K.graph_prep(ei, et, ntype, Rr, Tn)
    live, _, L = graph_live(g)
    assert np.array_equal(live, cpu_flags(ei, N)) and 0 < L < live.size
    rnd = lambda *shape, s=0.3: (torch.randn(*shape, generator=gen) * s).cuda()  # noqa: E731
    tab_col = SP - Tn
    Wx_t, Ws_t, W1t, W2t = rnd(DP, 3 * DP, s=0.1), rnd(SP, 3 * DP, s=0.1), rnd(DP, DP, s=0.1), rnd(DP, DP, s=0.1)
    Ws_t[tab_col:] = 0
    prm = (Wx_t, Wx_t.t().contiguous(), Ws_t, Ws_t.t().contiguous(), rnd(Tn, 3 * DP), rnd(Cc, 2 * DP),
           W1t, W1t.t().contiguous(), rnd(DP), 1 + rnd(DP), 9 + rnd(DP), W2t, W2t.t().contiguous(), rnd(DP), rnd(DP), 0.5 + rnd(DP).abs())
    X, S, dy = rnd(N, DP, s=1.0), rnd(N, SP, s=1.0), rnd(N, DP, s=1e-6 if mode == 2 else 1.0)
    S[:, tab_col:] = torch.nn.functional.one_hot(ntype, Tn).float()
    args = (g, HP, 1.0 / 50 ** 0.5, X, S, ntype, prm, True, 1e-5, 0.2, 4321, True)
    y, saved = K.hop_fwd(*args, None)
    res = {}
    for on in (1, 0):
        old = K.tn_live_tiles(on)
        try:
            grads = K.hop_bwd(*args, saved, dy, True, True, None, None, tab_col)
            torch.cuda.synchronize()
        finally:
            K.tn_live_tiles(old)
        res[on] = torch.cat([grads[2], grads[3]], 0)  # dWx_t | dWs_t: [DP + SP, 3 DP]
        assert torch.equal(grads[4], grads[3][tab_col:tab_col + Tn])  # dTT IS those rows of dWs_t
        res[on, 'rest'] = [t for i, t in enumerate(grads) if i not in (2, 3, 4)]
    for a, b in zip(res[1, 'rest'], res[0, 'rest']):  # nothing else of the hop changes
        assert torch.equal(a, b)
    assert not torch.equal(res[1], res[0]), 'the live-tile form did not run inside the hop'
    KMQ, aa, aggr, h1, out, stats = saved[:6]
    dout = K.gelu_dropout_bwd(out, dy, 0.2, 4321)
    daggr = ops._mlp_bwd(K, False, aggr, h1, dout, stats[0], stats[2], stats[3], stats[4], prm[9], W1t, prm[7], W2t, prm[12], -1, True)[0]
    dKMQ = K.edge_attn_bwd(g, KMQ, prm[5], HP, args[2], aa[0], aa[1], daggr)[0]
    dead_row = torch.from_numpy(np.repeat(live == 0, 32)[:N]).cuda()
    assert bool((dKMQ[dead_row, :DP] == 0).all()) and bool((dKMQ[dead_row, 2 * DP:] == 0).all())  # what the form relies on
    A64 = torch.cat([X, S], 1).double()
    absprod = A64.abs().t() @ dKMQ.double().abs()
    if mode == 2:
        arow = torch.cat([torch.full((DP,), X.abs().max().item()), torch.full((SP,), S.abs().max().item())]).double().cuda()
        bound = 16 * EPS * absprod + 2.0 ** -38 * N * arow[:, None] * dKMQ.abs().max().item() + 1e-30
    else:
        bound = 16 * EPS * absprod + 1e-6
    diff = (res[1].double() - res[0].double()).abs()
    print(f'hop mode={mode} N={N} T={live.size} L={L}: live vs withheld max {diff.max().item():.3e}, worst ratio to 2 bounds {(diff / (2 * bound)).max().item():.3f}')
    assert bool((diff <= 2 * bound).all())
    if mode == 1:
        ref = A64.t() @ dKMQ.double()
        for on in (1, 0):
            err = (res[on].double() - ref).abs()
            print(f'hop mode=1 live={on}: max err {err.max().item():.3e} worst bound ratio {(err / bound).max().item():.3f}')
            assert bool((err <= bound).all()), (on, (err / bound).max().item())
