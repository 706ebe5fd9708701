"""The row-walking kernels (column reductions, BatchNorm tile merge, GELU / maxima, node preparation) at the row counts where their loops
change shape: the switch between the 8- and the 32-rows-per-wave form of the column reductions, ragged last blocks with their clamped
loads, the partitions of the final sums, the strided rounds of the tile merge, one block / one capped sweep of the elementwise kernels.

The LAST ROW of every row-walked operand is a marker that a kernel cannot lose unnoticed: 64.0 in the summed operand, mean + 20 std under
the ReLU mask (open there), mean + 10 std for the statistics, the maximum in the last float4 of the elementwise calls.

  * `-m "not gpu"`: the constants the ladders rest on are found in the sources and the ladders follow from them; the comparison helpers
    (the ones the GPU cases call) accept the float64 answer and its float32 emulation in the kernels' own summation order, and reject an
    answer without the rows of the ragged tail and one with the clamped duplicate counted, at every count that has a tail.
  * `-m gpu`: the kernels against the float64 emulation under the bars of the neighbouring tests in test_hip_kernels.py.
"""
import functools
import os
import re
import types

import pytest
import torch

import helpers
import test_hip_kernels as THK
from test_hip_kernels import EMU, EPS, hip

# ---- the constants, read from the sources -------------------------------------------------------------------------------------------------
CONSTANT_PATTERNS = {
    'CR_WR_SMALL': ('elementwise.hip', r'\bCR_WR_SMALL = (\d+);'),
    'CR_WR_BIG': ('elementwise.hip', r'constexpr int CR_WR_BIG = (\d+),'),
    'CR_SWITCH': ('elementwise.hip', r'cr_wr\(int R\) \{ return R < (\d+) \? CR_WR_SMALL : CR_WR_BIG; \}'),
    'CR_BATCH': ('elementwise.hip', r'for \(int rb = r0; rb < rend; rb \+= (\d+)\)'),  # (both reduction kernels: the same literal)
    'CF_Q': ('elementwise.hip', r'constexpr int CF_Q = (\d+);'),
    'ST_TILE': ('elementwise.hip', r'constexpr int ST_TILE = (\d+);'),
    'BF_PARTS': ('elementwise.hip', r'\bBF_PARTS = (\d+);'),
    'BF_FLIGHT': ('elementwise.hip', r't0 \+= (\d+) \* BF_PARTS'),
    'SCAN_ITEMS': ('graph_prep.hip', r'constexpr int SCAN_ITEMS = (\d+);'),
    'SCAN_THREADS': ('graph_prep.hip', r'base \+= (\d+) \* SCAN_ITEMS'),
    'TN_SPLIT_ROWS': ('gemm_dispatch.hip', r'p\.R >= (\d+) &&'),
    'TN_LONG_ROWS': ('gemm_dispatch.hip', r'tn_min_chunk\(int R, bool split\) \{ return R > (\d+) \?'),
    'GELU_THREADS': ('elementwise.hip', r'const int grid = cdiv\(n / 4, (\d+)\);'),
    'ABSMAX_THREADS': ('elementwise.hip', r'const int grid = \(int\)\(n4 / (\d+) \+ 1 < \d+ \?'),
    'ABSMAX_GRID': ('elementwise.hip', r'const int grid = \(int\)\(n4 / \d+ \+ 1 < (\d+) \? n4'),
    'NODE_STEP': ('elementwise.hip', r'for \(int v = tid; v < n; v \+= (\d+)\)'),  # (both loops of k_node_prep: the same literal)
}


def _find(name, patterns=None):
    fn, pattern = (patterns or CONSTANT_PATTERNS)[name]
    with open(os.path.join(helpers.ROOT, 'qagnn_amd', 'csrc', fn)) as f:
        found = set(re.findall(pattern, f.read()))
    return int(found.pop()) if len(found) == 1 else None


CONST = {name: _find(name) for name in CONSTANT_PATTERNS}


def _ladders(c):
    if any(v is None for v in c.values()):
        return types.SimpleNamespace(col_rows=[], stat_tiles=[], scan_n=[], tn_rows=[], elem_n=[], node_n=[])  # (the `not gpu` test names what is missing)
    b, sb, bb, sw, q, p, fl = c['CR_BATCH'], 4 * c['CR_WR_SMALL'], 4 * c['CR_WR_BIG'], c['CR_SWITCH'], c['CF_Q'], c['BF_PARTS'], c['BF_FLIGHT']
    col = {1, b - 1, b, b + 1,                   # below, at, above one batch of row loads
           sb - 1, sb, sb + 1,                   # ... one block of the small form
           q * sb, q * sb + 1, 2 * q * sb + 1,   # q, q + 1, 2 q + 1 chunks: a partition's single-chunk tail, its first paired step
           sw - 1, sw, sw + 1,                   # the last count of the small form, the first of the big one, a one-row last block
           sw + bb - 1, sw + bb + 1}             # bb - 1 and bb + 1 rows past the switch: a last block that lacks one row / holds one
    tiles = {1, 2, p - 1, p, p + 1, 2 * p, 2 * p + 1, fl * p - 1, fl * p, fl * p + 1}
    scan = c['SCAN_THREADS'] * c['SCAN_ITEMS']
    tn = {r + k for r in (c['TN_SPLIT_ROWS'], c['TN_LONG_ROWS']) for k in (-1, 0, 1)}
    # floats per block of float4 lanes (GELU / dropout and absmax: the same block); one float4; around one block; 257 blocks; around one
    # capped sweep of absmax (the last: one per-block maximum more than a 1024-float block of launch_amax_reduce takes)
    eb, sweep = 4 * c['GELU_THREADS'], 4 * c['ABSMAX_THREADS'] * c['ABSMAX_GRID']
    elem = [4, eb - 4, eb, eb + 4, 256 * eb + 4, sweep - 4, sweep, sweep + 4]
    st = c['NODE_STEP']  # around one wave and one step of k_node_prep; four steps
    node = [1, 63, 64, 65, st - 1, st, st + 1, 4 * st]
    return types.SimpleNamespace(col_rows=sorted(col), stat_tiles=sorted(tiles), scan_n=[scan - 1, scan, scan + 1], tn_rows=sorted(tn),
                                 elem_n=elem, node_n=node)


LADDERS = _ladders(CONST)
COL_ROWS, STAT_TILES = LADDERS.col_rows, LADDERS.stat_tiles
ELEM_N, NODE_N, NODE_B = LADDERS.elem_n, LADDERS.node_n, 3
COL_WIDE = 260        # two column blocks, the second holding one float4
COL_CASES = [(R, 32) for R in COL_ROWS] + [(R, COL_WIDE) for R in COL_ROWS if R <= 1025 or R == CONST['CR_SWITCH'] + 1]
STAT_CASES = [(t, tail) for t in STAT_TILES for tail in ('full', 'one_row')]
BN_MODES = ('batch', 'running', 'weighted')


def cr_block(R):
    """rows per block of the column reductions at R rows (cr_wr of csrc/elementwise.hip)"""
    return 4 * (CONST['CR_WR_SMALL'] if R < CONST['CR_SWITCH'] else CONST['CR_WR_BIG'])


# ---- the comparison helpers (GPU cases and the `not gpu` checks call the same ones) ---------------------------------------------------------
def _ratio(x, ref, bar):
    err = (x.double() - ref).abs()
    bar = torch.as_tensor(bar, dtype=torch.float64).expand_as(err)
    r = err / bar.clamp_min(1e-300)  # (a zero bar -- the variance of one row -- asks for the exact value)
    r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
    return r.max().item() if r.numel() else 0.0


def held(nm, got, ref, bar, log, emu=None):
    """|got - ref| <= bar everywhere.  log: the worst |d| / bar of the kernel, and of the float32 emulation where there is one."""
    r = _ratio(got, ref, bar)
    log.append(f'{nm} {r:.2e}' + ('' if emu is None else f' (f32 {_ratio(emu, ref, bar):.2e})'))
    assert got.shape == ref.shape and r <= 1.0, f'{nm}: {r:.3g} of the bar'


def _beyond(x, ref):
    return int((~((x.double() - ref).abs() <= 1e-4 * (1 + ref.abs()))).sum())


def few_beyond(nm, got, ref, log, emu=None, allowed=2):
    """at most `allowed` elements beyond 1e-4 (1 + |ref|): mask flips at |y| ~ 1e-7 are legal (test_column_reductions_and_bn_backward)"""
    n = _beyond(got, ref)
    log.append(f'{nm} {n} beyond' + ('' if emu is None else f' (f32 {_beyond(emu, ref)})'))
    assert got.shape == ref.shape and n <= allowed, f'{nm}: {n} elements differ beyond fp32 rounding'


def _allclose_bar(ref, rtol=1e-5, atol=1e-6):
    return atol + rtol * ref.abs()


# ---- column reductions ------------------------------------------------------------------------------------------------------------------------
def _col_reference(c, rows=None, dh_rows=None):
    """The float64 answers of every column-reduction call of a case.  rows: the rows a (wrong) reduction adds up, in order (default: all, once);
    dh_rows: the rows a (wrong) elementwise pass writes, the others stay zero."""
    R = c.R
    rows = torch.arange(R) if rows is None else rows
    d = lambda t: t.double()  # noqa: E731
    X, H, w, idx = d(c.X)[rows], d(c.H)[rows], d(c.w)[rows], c.idx[rows]
    stat = [d(t) for t in (c.mean, c.invstd, c.scale, c.shift)]
    out = {'colsum': EMU.colsum(X), 'colsum_grouped': EMU.colsum(X, idx, 4), 'colsum_weighted': EMU.colsum(X, roww=w),
           'colsum_scaled': EMU.colsum(H, scale=1.0 / R), 'colvar': EMU.colvar_sum(H, stat[0]),
           'colvar_weighted': EMU.colvar_sum(H, stat[0], roww=w), 'colvar_scaled': EMU.colvar_sum(H, stat[0], scale=1.0 / R),
           'bn_bwd_reduce': EMU.bn_bwd_reduce(X, H, *stat)}
    full = (d(c.X), d(c.H), *stat, d(c.gamma), d(c.red))
    for mode, (inv_rows, roww) in c.bn_modes.items():
        dH = EMU.bn_relu_bwd(*full, inv_rows, None if roww is None else d(roww))
        if dh_rows is not None:
            kept = torch.zeros_like(dH)
            kept[dh_rows] = dH[dh_rows]
            dH = kept
        out[f'dH[{mode}]'] = out[f'dHc[{mode}]'] = dH
        out[f'cs[{mode}]'] = out[f'cs_separate[{mode}]'] = dH[rows].sum(0)
    return out


def _build_col_case(R, C):
    g = torch.Generator().manual_seed(R * 7 + C)
    X, H = torch.randn(R, C, generator=g), torch.randn(R, C, generator=g) * 2 + 0.3
    idx = torch.randint(0, 4, (R,), generator=g)
    w = torch.rand(R, generator=g) + 0.1
    w = w / w.sum()
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)  # (gamma > 0: the mask opens at large H)
    mean, var = H.mean(0), H.double().var(0, unbiased=False).float()
    invstd = torch.rsqrt(var + 1e-5)
    # the marker row: 64.0 in every sum, mean + 20 std under the mask (hhat = 20: y = 20 gamma + beta > 0), group 3
    X[-1], H[-1], idx[-1] = 64.0, mean + 20.0 / invstd, 3
    scale, shift = gamma * invstd, beta - mean * gamma * invstd
    c = types.SimpleNamespace(R=R, C=C, X=X, H=H, idx=idx, w=w, gamma=gamma, mean=mean, invstd=invstd, scale=scale, shift=shift,
                              bn_modes={'batch': (1.0 / R, None), 'running': (0.0, None), 'weighted': (0.0, w)})
    c.red = EMU.bn_bwd_reduce(*[t.double() for t in (X, H, mean, invstd, scale, shift)]).float().contiguous()
    c.ref = _col_reference(c)
    hhat = ((H - mean) * invstd).abs()
    c.bars = {'colsum': 4 * EPS * X.abs().sum(0).max().item() + 1e-6,
              # mask flips at |y| ~ 1e-7 are legal; the bound has the size of a few elements (test_column_reductions_and_bn_backward)
              'bn_bwd_reduce': 8 * EPS * (X.abs() * (1 + hhat)).sum(0).max().item() + 3 * X.abs().max().item() * 4,
              'colvar': 8 * EPS * c.ref['colvar'] + 1e-6}
    c.bars['colsum_grouped'] = c.bars['colsum']
    # that bound is 768 with the marker's 64 in it: more than the whole marker row of out[0] = sum dy.  out[0] on its own: the colsum bar,
    # and two mask flips (the cap of the elementwise passes) of the largest element outside the marker row, whose mask is wide open
    c.bars['bn_bwd_reduce[0]'] = c.bars['colsum'] + 2 * (X[:-1].abs().max().item() if R > 1 else 0.0)
    for nm in ('colsum_weighted', 'colsum_scaled', 'colvar_weighted', 'colvar_scaled'):
        c.bars[nm] = _allclose_bar(c.ref[nm])
    return c


col_case = functools.lru_cache(maxsize=None)(_build_col_case)
COL_SUMS = ('colsum', 'colsum_grouped', 'colsum_weighted', 'colsum_scaled', 'colvar', 'colvar_weighted', 'colvar_scaled', 'bn_bwd_reduce')


def check_col_outputs(c, out, log, emu=None):
    """Every assertion of the column-reduction cases, on the outputs `out` holds (name -> tensor on the CPU)."""
    emu = emu or {}
    for nm in COL_SUMS:
        if nm in out:
            held(nm, out[nm], c.ref[nm], c.bars[nm], log, emu.get(nm))
    if 'bn_bwd_reduce' in out:
        nm = 'bn_bwd_reduce[0]'
        held(nm, out['bn_bwd_reduce'][0], c.ref['bn_bwd_reduce'][0], c.bars[nm], log, emu['bn_bwd_reduce'][0] if 'bn_bwd_reduce' in emu else None)
    for mode in c.bn_modes:
        dH, dHc, cs, sep = (out.get(f'{k}[{mode}]') for k in ('dH', 'dHc', 'cs', 'cs_separate'))
        ref = c.ref[f'dH[{mode}]']
        for nm, t in ((f'dH[{mode}]', dH), (f'dHc[{mode}]', dHc)):
            if t is not None:
                few_beyond(nm, t, ref, log, emu.get(f'dH[{mode}]'))
        if dH is not None and dHc is not None:  # same formula; FMA contraction may differ by an ulp
            assert (dHc - dH).abs().max().item() <= 1e-6 * dH.abs().max().item(), f'dHc[{mode}] and dH[{mode}] disagree'
        if cs is not None:  # the by-product is the column sum of what the pass wrote (the colsum bar, on those values)
            wrote = dHc.double()
            held(f'cs[{mode}]', cs, wrote.sum(0), 4 * EPS * wrote.abs().sum(0).max().item() + 1e-6, log, emu.get(f'cs[{mode}]'))
            if sep is not None:  # ... bit-identical to a separate mode-0 pass: both choose their shape from R alone
                assert torch.equal(cs, sep), f'cs[{mode}] is not the bits of colsum(dH) at R = {c.R}'


def run_col_kernels(K, c):
    cu = lambda t: None if t is None else t.cuda()  # noqa: E731
    X, H, mean, invstd, scale, shift, gamma, red, idx, w = map(cu, (c.X, c.H, c.mean, c.invstd, c.scale, c.shift, c.gamma, c.red, c.idx, c.w))
    out = {'colsum': K.colsum(X), 'colsum_grouped': K.colsum(X, idx, 4), 'colsum_weighted': K.colsum(X, roww=w),
           'colsum_scaled': K.colsum(H, scale=1.0 / c.R), 'colvar': K.colvar_sum(H, mean), 'colvar_weighted': K.colvar_sum(H, mean, roww=w),
           'colvar_scaled': K.colvar_sum(H, mean, scale=1.0 / c.R), 'bn_bwd_reduce': K.bn_bwd_reduce(X, H, mean, invstd, scale, shift)}
    for mode, (inv_rows, roww) in c.bn_modes.items():
        args = (X, H, mean, invstd, scale, shift, gamma, red, inv_rows, cu(roww))
        out[f'dH[{mode}]'] = K.bn_relu_bwd(*args)
        out[f'dHc[{mode}]'], out[f'cs[{mode}]'] = K.bn_relu_bwd_colsum(*args)
        out[f'cs_separate[{mode}]'] = K.colsum(out[f'dHc[{mode}]'])[0]
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


# -- float32 emulation of k_colreduce / k_bn_relu_bwd_colsum + k_colreduce_final in the kernels' own summation order
def _fma32(a, b, acc):
    """fmaf(a, b, acc) on float32 tensors: the product is exact in float64, the sum is rounded to float32 (b None: a + acc)"""
    return (a + acc) if b is None else (a.double() * b.double() + acc.double()).float()


def _emu32_chunks(a, b, R):
    """chunk partials [chunks, C]: every wave adds its rows in order (acc = fmaf(a[r], b[r], acc), or acc + a[r]), a block sums its four
    waves as (w0 + w1) + (w2 + w3); rows past the end add nothing"""
    wr = cr_block(R) // 4
    nch, C = -(-R // (4 * wr)), a.size(1)
    pad = lambda t: torch.cat([t, t.new_zeros(nch * 4 * wr - R, C)]).view(nch, 4, wr, C)  # noqa: E731
    a, b = pad(a), (None if b is None else pad(b))
    acc = torch.zeros(nch, 4, C)
    for r in range(wr):
        acc = _fma32(a[:, :, r], None if b is None else b[:, :, r], acc)
    return (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])


def _emu32_final(part, scale=1.0):
    """k_colreduce_final: partition q adds chunks q, q + 2 Q, ... into s0 and q + Q, q + 3 Q, ... into s1; s0 + s1; the partitions in order"""
    Q, (nch, C) = CONST['CF_Q'], part.shape
    s = torch.zeros(2, Q, C)
    for k in range(-(-nch // Q)):
        blk = part[k * Q:(k + 1) * Q]
        s[k & 1, :blk.size(0)] += blk
    red = s[0] + s[1]
    out = red[0].clone()
    for q in range(1, Q):
        out = out + red[q]
    return out * torch.tensor(scale, dtype=torch.float32)


def col_emulation(c):
    """name -> the float32 answer in the kernels' summation order (the elementwise passes: the emulation's formula in float32)"""
    R, X, H, w = c.R, c.X, c.H, c.w.unsqueeze(1)
    red = lambda a, b=None, scale=1.0: _emu32_final(_emu32_chunks(a, b, R), scale)  # noqa: E731
    d = H - c.mean
    dy = torch.where(H * c.scale + c.shift <= 0, torch.zeros(()), X)
    out = {'colsum': red(X).unsqueeze(0), 'colsum_weighted': red(X * w).unsqueeze(0), 'colsum_scaled': red(H, None, 1.0 / R).unsqueeze(0),
           'colsum_grouped': torch.stack([red(X * (c.idx == k).float().unsqueeze(1)) for k in range(4)]),
           'colvar': red(d, d), 'colvar_weighted': red(d * w, d), 'colvar_scaled': red(d, d, 1.0 / R),
           'bn_bwd_reduce': torch.stack([red(dy), red(dy, d * c.invstd)])}
    for mode, (inv_rows, roww) in c.bn_modes.items():
        dH = EMU.bn_relu_bwd(X, H, c.mean, c.invstd, c.scale, c.shift, c.gamma, c.red, inv_rows, roww)
        out[f'dH[{mode}]'], out[f'cs[{mode}]'] = dH, red(dH)
    return out


# ---- BatchNorm statistics from tile partials ---------------------------------------------------------------------------------------------
STAT_C, STAT_D = 32, 28  # head-padded columns (HP = 8) and the module's dense features (dh = 7: one pad column per head)


def _stat_answer(x, R, gamma, beta, rm0, rv0, pos):
    """float64 statistics of the rows x as qagnn_bn_stats_finalize_f32 lays them out (the variance over R rows), and the running buffers"""
    n = x.size(0)
    mean = x.sum(0) / max(n, 1)
    var = ((x - mean) ** 2).sum(0) / R
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    stats = torch.stack([mean, var, invstd, gamma.double() * invstd, beta.double() - mean * gamma.double() * invstd])
    unb = R / max(R - 1.0, 1.0)
    return stats, rm0.double() + 0.1 * (mean[pos] - rm0.double()), rv0.double() + 0.1 * (var[pos] * unb - rv0.double()), 8


def _build_stat_case(tiles, tail):
    T = CONST['ST_TILE']
    R = T * tiles if tail == 'full' else T * (tiles - 1) + 1
    g = torch.Generator().manual_seed(R)
    mu = torch.randn(STAT_C, generator=g) * 3.0 + 5.0  # a mean far from 0 relative to the spread (test_gemm_column_statistics_and_bn_stats_finalize)
    x = mu + 1.4 * torch.randn(R, STAT_C, generator=g)
    x[-1] = mu + 14.0  # the marker row: mean + 10 std
    gamma, beta = torch.rand(STAT_C, generator=g) + 0.5, torch.randn(STAT_C, generator=g)
    rm0, rv0 = torch.randn(STAT_D, generator=g) * 0.1, torch.rand(STAT_D, generator=g) + 0.5
    from qagnn_amd import ops
    L = ops.HeadLayout(STAT_D, 'cpu')
    assert L.DP == STAT_C
    c = types.SimpleNamespace(tiles=tiles, tail=tail, R=R, x=x, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, pos=L.dense_pos,
                              part=EMU.col_partials(x.double()).float().contiguous(), unb=R / max(R - 1.0, 1.0))
    assert c.part.shape == (tiles, 3, STAT_C)
    c.ref = _stat_answer(x.double(), R, gamma, beta, rm0, rv0, c.pos)
    return c


stat_case = functools.lru_cache(maxsize=None)(_build_stat_case)


def check_stat_outputs(c, got, log, emu=None):
    """got = (stats [5, C], running mean, running var, batch counter); the bars of test_gemm_column_statistics_and_bn_stats_finalize"""
    stats, rm, rv, nbt = got
    (mean64, var64, invstd, scale64, shift64), rm64, rv64, nbt64 = c.ref
    e = emu[0] if emu is not None else [None] * 5
    held('mean', stats[0], mean64, 2e-6 * mean64.abs().max().item(), log, e[0])
    held('var', stats[1], var64, 1e-5 * var64, log, e[1])  # relative, per column: no cancellation against the large mean
    held('invstd', stats[2], invstd, 1e-5 * invstd, log, e[2])
    held('scale', stats[3], scale64, 1e-5 * scale64.abs().max().item(), log, e[3])
    held('shift', stats[4], shift64, 2e-5 * shift64.abs().max().item(), log, e[4])
    held('run_mean', rm, rm64, _allclose_bar(rm64, 1e-5, 1e-6), log, None if emu is None else emu[1])
    held('run_var', rv, rv64, _allclose_bar(rv64, 1e-5, 1e-6), log, None if emu is None else emu[2])
    assert int(nbt) == nbt64 == 8


def stat_emulation(c):
    """k_bn_stats_finalize in float32: partition q merges tiles q, q + P, ... in order (Chan, Golub & LeVeque), the partitions meet in a binary tree"""
    P, T, (nt, _, C) = CONST['BF_PARTS'], CONST['ST_TILE'], c.part.shape
    n_t = torch.tensor([min(T, c.R - t * T) for t in range(nt)], dtype=torch.float32).unsqueeze(1)
    x0, S1, S2 = c.part[:, 0], c.part[:, 1], c.part[:, 2]
    nb, mb, m2b = n_t.expand(nt, C), x0 + S1 / n_t, S2 - S1 * S1 / n_t
    padded = lambda t: torch.cat([t, t.new_zeros(-(-nt // P) * P - nt, C)]).view(-1, P, C)  # noqa: E731  (a tile of 0 rows merges nothing)
    nb, mb, m2b = padded(nb), padded(mb), padded(m2b)

    def merge(a, b):
        (an, am, a2), (bn, bm, b2) = a, b
        n, d = an + bn, bm - am
        live = bn > 0
        safe = torch.where(live, n, torch.ones_like(n))
        return (torch.where(live, n, an), torch.where(live, am + d * (bn / safe), am), torch.where(live, a2 + (b2 + d * d * (an * bn / safe)), a2))

    a = tuple(torch.zeros(P, C) for _ in range(3))
    for k in range(nb.size(0)):
        a = merge(a, (nb[k], mb[k], m2b[k]))
    stride = 1
    while stride < P:
        sel = torch.arange(0, P, 2 * stride)
        m = merge(tuple(t[sel] for t in a), tuple(t[sel + stride] for t in a))
        a = tuple(t.index_copy(0, sel, u) for t, u in zip(a, m))
        stride *= 2
    mean, var = a[1][0], (a[2][0] / torch.tensor(float(c.R))).clamp_min(0)
    rm, rv = c.rm0.clone(), c.rv0.clone()
    invstd, scale, shift = EMU.bn_finalize(mean, var, c.gamma, c.beta, 1e-5, (rm, rv, None, c.pos, 0.1, c.unb))
    return torch.stack([mean, var, invstd, scale, shift]), rm, rv, 8


# ---- elementwise: GELU + dropout, maxima, node preparation --------------------------------------------------------------------------------
GELU_SEED = 0x1234567ABCE00  # (keeps the last element at p = 0.3 for every n of ELEM_N: checked below)
GELU_P = (0.0, 0.3)
ABSMAX_MARK = 77.25


def _build_gelu_case(n, p):
    g = torch.Generator().manual_seed(n)
    X, dY = torch.randn(n, generator=g).clamp(-2, 2), torch.randn(n, generator=g)
    X[-4:], dY[-4:] = 2.5, 64.0  # the marker float4: gelu(2.5) and 64 gelu'(2.5) are the maxima of y and dx where it is kept
    c = types.SimpleNamespace(n=n, p=p, X=X, dY=dY)
    c.y, c.dx = EMU.gelu_dropout_fwd(X.double(), p, GELU_SEED), EMU.gelu_dropout_bwd(X.double(), dY.double(), p, GELU_SEED)
    return c


gelu_case = functools.lru_cache(maxsize=None)(_build_gelu_case)


def check_gelu_outputs(c, y, dx, log, emu=None):
    """the assertions of test_gelu_dropout_forward_backward_and_mask, and that the marker is there: kept, and the maximum of its tensor"""
    ey, edx = emu or (None, None)
    same_mask = torch.equal(y == 0, (c.y == 0) | (c.X == 0))  # (|X| <= 2.5: no underflow of gelu, every element is `live`)
    assert same_mask, 'keep mask differs from the counter-based hash'
    held('y', y, c.y, 2e-6 * (1 + c.y.abs().max().item()), log, ey)
    held('dx', dx, c.dx, 2e-6 * (1 + c.dx.abs().max().item()), log, edx)
    assert y[-1].item() != 0 and y[-1].item() == y.abs().max().item(), 'the last element of y does not carry the maximum'
    assert dx[-1].item() != 0 and dx[-1].item() == dx.abs().max().item(), 'the last element of dx does not carry the maximum'


def _bits(v):
    return torch.as_tensor(v, dtype=torch.float32).view(torch.int32).item()


def absmax_operand(n, where):
    """randn with the maximum in the last (first) float4 and a NaN, which the maximum skips, next to it"""
    x = torch.randn(n, generator=torch.Generator().manual_seed(n + 1))
    if where == 'last':
        x[n - 2], x[n - 1] = -ABSMAX_MARK, float('nan')
    else:
        x[1], x[0] = -ABSMAX_MARK, float('nan')
    return x


def check_absmax_word(word, x):
    want = x[~torch.isnan(x)].abs().max()
    assert want.item() == ABSMAX_MARK and int(word) == _bits(want), f'the word holds {int(word):#x}, max |x| is {_bits(want):#x}'


def _build_node_case(n):
    g = torch.Generator().manual_seed(n)
    B = NODE_B
    raw = -(20.0 + 40.0 * torch.rand(B, n, 1, generator=g)) * (1.0 + 1e-3 * torch.randn(B, n, 1, generator=g))  # arbitrary fp32 scores
    raw[:, 0] = raw.max(dim=1).values + 1.0
    if n > 1:
        raw[:, n - 1] = raw.min(dim=1).values - 100.0  # the marker slot: the largest |score - score[0]| of its row
    al = torch.tensor([1, n // 2 + 1, n])
    nt = torch.randint(0, 3, (B, n), generator=g)
    nt[:, 0] = 3  # subgraph 0 (adj_len = 1, a context node of type 3): every slot masked -> slot 0 is un-masked
    cids = torch.randint(1, 500, (B, n), generator=g)
    c = types.SimpleNamespace(n=n, raw=raw, al=al, nt=nt, cids=cids)
    c.score32, c.mask, c.ridx = EMU.node_prep(raw, al, nt.clone(), cids.clone())  # the reference's fp32 op sequence
    # the kernel's formula: the row sum of |score| in float64, rounded once
    real = (torch.arange(n) < al.unsqueeze(1)).float()
    d = (-raw.view(B, n) - (-raw.view(B, n)[:, 0:1])) * real
    c.want = d / (d.abs().double().sum(1).float() / al.float() + 1e-05).unsqueeze(1)
    return c


node_case = functools.lru_cache(maxsize=None)(_build_node_case)


def check_node_outputs(c, score, mask, ridx, log):
    """the bars of test_node_prep_on_unquantised_scores: the bits of the formula with a float64 row sum, within 4 ulp of the reference's fp32 ops"""
    assert torch.equal(mask, c.mask) and torch.equal(ridx, c.ridx)
    assert mask.dtype == torch.bool and not bool(mask[0, 0]) and bool(mask[0, 1:].all())
    assert torch.equal(score, c.want), f'score differs from the float64-row-sum formula by {(score - c.want).abs().max().item():.3e}'
    ulp = torch.finfo(torch.float32).eps * c.score32.abs().clamp_min(1e-30)
    held('score', score, c.score32.double(), 4 * ulp.double(), log)
    if c.n > 1:
        assert score[2, c.n - 1].item() != 0 and score[2, c.n - 1].abs().item() == score[2].abs().max().item()


# ---- `not gpu` ------------------------------------------------------------------------------------------------------------------------------
def test_the_constants_are_found_and_the_ladders_follow_from_them():
    """`-m "not gpu"`.  A changed constant shows here, not as quietly thinner coverage."""
    missing = [k for k, v in CONST.items() if v is None]
    assert not missing, f'not found in the sources (once, or with one value): {missing}'
    assert (CONST['CR_WR_SMALL'], CONST['CR_WR_BIG'], CONST['CR_SWITCH'], CONST['CR_BATCH'], CONST['CF_Q']) == (8, 32, 32768, 8, 16)
    assert (CONST['ST_TILE'], CONST['BF_PARTS'], CONST['BF_FLIGHT'], CONST['SCAN_ITEMS'] * CONST['SCAN_THREADS']) == (128, 64, 4, 8192)
    assert (CONST['TN_SPLIT_ROWS'], CONST['TN_LONG_ROWS']) == (1024, 4096) and CONST['ST_TILE'] == EMU.STAT_TILE
    assert COL_ROWS == [1, 7, 8, 9, 31, 32, 33, 512, 513, 1025, 32767, 32768, 32769, 32895, 32897]
    assert STAT_TILES == [1, 2, 63, 64, 65, 128, 129, 255, 256, 257]
    assert ELEM_N == [4, 1020, 1024, 1028, 262148, 1048572, 1048576, 1048580]
    # what the counts are there for
    chunks = lambda R: -(-R // cr_block(R))  # noqa: E731
    Q, sw = CONST['CF_Q'], CONST['CR_SWITCH']
    assert {Q, Q + 1, 2 * Q + 1} <= {chunks(R) for R in COL_ROWS} and cr_block(sw - 1) == 32 and cr_block(sw) == 128
    assert [R % cr_block(R) for R in COL_ROWS if R >= sw] == [0, 1, 127, 1] and chunks(sw + 129) == chunks(sw) + 2
    assert sorted({R for R, C in COL_CASES if C == COL_WIDE}) == [R for R in COL_ROWS if R <= 1025] + [sw + 1] and COL_WIDE % 256 == 4
    assert len(COL_CASES) == 26 and len(STAT_CASES) == 20
    assert max(R * C for R, C in COL_CASES) <= 32897 * 260
    assert NODE_N == [1, 63, 64, 65, 255, 256, 257, 1024] and CONST['GELU_THREADS'] == CONST['ABSMAX_THREADS'] == 256
    per_block = [-(-n // (4 * CONST['GELU_THREADS'])) for n in ELEM_N]
    assert per_block == [1, 1, 1, 2, 257, 1024, 1024, 1025]  # (k_absmax sweeps once up to 1024 blocks' worth; the 1025th starts a second sweep)
    # the cases the neighbouring tests run at the other boundaries
    graphs = dict(THK.GRAPH_CASES)
    assert [graphs[f'rand_{N}']()[2].numel() for N in LADDERS.scan_n] == LADDERS.scan_n == [8191, 8192, 8193]
    assert graphs['rand_33k']()[2].numel() == sw + 1 and (sw + 1) % 4 == 1
    tn = next(m for m in THK.test_gemm_tn.pytestmark if m.name == 'parametrize' and m.args[0] == 'R,Ka,No')
    assert {(R, 208, 208) for R in LADDERS.tn_rows} <= set(tn.args[1]) and LADDERS.tn_rows == [1023, 1024, 1025, 4095, 4096, 4097]
    tn2 = next(m for m in THK.test_gemm_tn_two_operands.pytestmark if m.name == 'parametrize')
    assert {(1024, 208, 112, 624), (4097, 208, 112, 624)} <= set(tn2.args[1])
    stat_m = next(m for m in THK.test_gemm_column_statistics_and_bn_stats_finalize.pytestmark if m.name == 'parametrize')
    P, T = CONST['BF_PARTS'], CONST['ST_TILE']
    assert {T * (P - 1) + 1, T * P + 1} <= set(stat_m.args[1])  # 64 and 65 tiles with a one-row last tile, through the GEMM epilogue


def _tail_rows(R):
    return R % cr_block(R)


@pytest.mark.parametrize('R,C', COL_CASES)
def test_column_comparison_accepts_the_right_answer_and_rejects_a_lost_or_doubled_tail(R, C):
    """`-m "not gpu"`, nothing runs on a GPU.  check_col_outputs accepts the float64 answer and the float32 emulation in the kernels' order
    (which stays below half of every bar, and at 0 or 1 elements of the capped exemption); it rejects, output by output, (a) sums without the
    rows of the ragged last block, an elementwise pass that did not write them, and (b) sums with the last row -- the clamped duplicate of a
    short batch -- added once more."""
    c = col_case(R, C)
    check_col_outputs(c, {k: v.float() for k, v in c.ref.items()}, [])
    emu, log = col_emulation(c), []
    check_col_outputs(c, dict(emu, **{f'dHc[{m}]': emu[f'dH[{m}]'] for m in c.bn_modes}), log)
    for nm in COL_SUMS:
        assert _ratio(emu[nm], c.ref[nm], c.bars[nm]) <= 0.5, f'{nm}: the float32 emulation takes {_ratio(emu[nm], c.ref[nm], c.bars[nm]):.2f} of the bar'
    for m in c.bn_modes:  # the cap on exemptions is a condition: the seeds leave the emulation 0 or 1 such elements
        assert _beyond(emu[f'dH[{m}]'], c.ref[f'dH[{m}]']) <= 1, (m, log)
    tail = _tail_rows(R)
    flaws = {'doubled': _col_reference(c, rows=torch.cat([torch.arange(R), torch.tensor([R - 1])]))}
    if tail:
        flaws['lost'] = _col_reference(c, rows=torch.arange(R - tail), dh_rows=torch.arange(R - tail))
    for flaw, wrong in flaws.items():
        wrong = {k: v.float() for k, v in wrong.items()}
        for nm in COL_SUMS:
            with pytest.raises(AssertionError, match=re.escape(nm + ':')):
                check_col_outputs(c, {nm: wrong[nm]}, [])
        with pytest.raises(AssertionError, match=re.escape('bn_bwd_reduce[0]:')):  # sum dy alone, the other output right
            check_col_outputs(c, {'bn_bwd_reduce': torch.stack([wrong['bn_bwd_reduce'][0], c.ref['bn_bwd_reduce'][1].float()])}, [])
        for m in c.bn_modes:
            right = {f'{k}[{m}]': c.ref[f'{k}[{m}]'].float() for k in ('dH', 'dHc', 'cs', 'cs_separate')}
            with pytest.raises(AssertionError, match=re.escape(f'cs[{m}]:')):  # the pass wrote every row, its by-product lost / doubled some
                check_col_outputs(c, dict(right, **{f'cs[{m}]': wrong[f'cs[{m}]'], f'cs_separate[{m}]': wrong[f'cs[{m}]']}), [])
            if flaw == 'lost':
                with pytest.raises(AssertionError, match=re.escape(f'dHc[{m}]:')):
                    check_col_outputs(c, dict(right, **{f'dHc[{m}]': wrong[f'dHc[{m}]']}), [])
                with pytest.raises(AssertionError, match=re.escape(f'dH[{m}]:')):
                    check_col_outputs(c, {f'dH[{m}]': wrong[f'dH[{m}]']}, [])
    with pytest.raises(AssertionError, match='not the bits of colsum'):  # the bit-identity across the form switch is asserted, not reported
        check_col_outputs(c, dict({k: v.float() for k, v in c.ref.items()}, **{'cs_separate[batch]': torch.nextafter(c.ref['cs[batch]'].float(), torch.tensor(float('inf')))}), [])


@pytest.mark.parametrize('tiles,tail', STAT_CASES)
def test_statistics_comparison_accepts_the_right_answer_and_rejects_a_lost_or_doubled_tile(tiles, tail):
    """`-m "not gpu"`.  check_stat_outputs accepts the float64 statistics and the float32 emulation of the merge (partition order, then the
    tree; below half of the mean and variance bars); it rejects the statistics without the last tile and with the last tile -- the clamped
    duplicate of a partition's short batch -- merged twice."""
    c = stat_case(tiles, tail)
    f32 = lambda ans: (ans[0].float(), ans[1].float(), ans[2].float(), ans[3])  # noqa: E731
    check_stat_outputs(c, f32(c.ref), [])
    emu = stat_emulation(c)
    check_stat_outputs(c, emu, [])
    assert _ratio(emu[0][0], c.ref[0][0], 2e-6 * c.ref[0][0].abs().max().item()) <= 0.5
    assert _ratio(emu[0][1], c.ref[0][1], 1e-5 * c.ref[0][1]) <= 0.5
    T = CONST['ST_TILE']
    x = c.x.double()
    last = x[T * (tiles - 1):]
    # (one row merged twice is the same one-row statistics: nothing to reject there)
    for wrong_rows in (x[:T * (tiles - 1)],) + ((torch.cat([x, last]),) if c.R > 1 else ()):
        wrong = f32(_stat_answer(wrong_rows, c.R, c.gamma, c.beta, c.rm0, c.rv0, c.pos))
        with pytest.raises(AssertionError, match='mean:|var:'):
            check_stat_outputs(c, wrong, [])
        if c.R > 1:  # ... and by the variance alone (one tile merged twice keeps its mean)
            with pytest.raises(AssertionError, match='var:'):
                check_stat_outputs(c, (torch.cat([c.ref[0][:1].float(), wrong[0][1:]]),) + wrong[1:], [])


@pytest.mark.parametrize('n', ELEM_N)
def test_elementwise_comparison_accepts_the_right_answer_and_rejects_a_lost_float4(n):
    """`-m "not gpu"`.  The GELU / dropout and maximum checks accept the float64 answer and reject one whose last float4 was never written
    (never read); the dropout seed keeps the last element at every n, so the marker carries the maximum."""
    for p in GELU_P:
        c = gelu_case(n, p)
        assert c.y[-1].item() != 0 and c.dx[-1].item() != 0, f'seed {GELU_SEED:#x} drops the last element at n = {n}, p = {p}'
        y, dx = c.y.float(), c.dx.float()
        check_gelu_outputs(c, y, dx, [], (EMU.gelu_dropout_fwd(c.X, p, GELU_SEED), EMU.gelu_dropout_bwd(c.X, c.dY, p, GELU_SEED)))
        lost = lambda t: torch.cat([t[:-4], torch.zeros(4)])  # noqa: E731
        with pytest.raises(AssertionError):
            check_gelu_outputs(c, lost(y), dx, [])
        with pytest.raises(AssertionError):
            check_gelu_outputs(c, y, lost(dx), [])
    for where in ('last', 'first'):
        x = absmax_operand(n, where)
        check_absmax_word(_bits(ABSMAX_MARK), x)
        if n > 4:
            short = x[:-4] if where == 'last' else x[4:]
            with pytest.raises(AssertionError):
                check_absmax_word(_bits(short[~torch.isnan(short)].abs().max()), x)


@pytest.mark.parametrize('n', NODE_N)
def test_node_comparison_accepts_the_formula_and_rejects_a_lost_slot(n):
    """`-m "not gpu"`.  The float64-row-sum formula is within 4 ulp of the reference's fp32 op sequence at every n (so the two assertions of
    check_node_outputs can hold together); a row sum without the last slot is rejected."""
    c = node_case(n)
    check_node_outputs(c, c.want, c.mask, c.ridx, [])
    if n > 1:
        B = NODE_B
        real = (torch.arange(n) < c.al.unsqueeze(1)).float()
        d = (-c.raw.view(B, n) - (-c.raw.view(B, n)[:, 0:1])) * real
        lost = d / (d[:, :-1].abs().double().sum(1).float() / c.al.float() + 1e-05).unsqueeze(1)
        with pytest.raises(AssertionError, match='score'):
            check_node_outputs(c, lost, c.mask, c.ridx, [])


# ---- `gpu` ----------------------------------------------------------------------------------------------------------------------------------
def _figure(label, log):
    """One line per case for the record of a GPU run (profiles/row_count_gpu_tests.txt; shown by pytest -s, or on failure): per output the
    worst |kernel - float64| as a fraction of its bar (passes at <= 1), and (f32 ...) the same for the float32 emulation."""
    print(f'FIGURE {label} as fractions of the bars: ' + ' | '.join(log))


@pytest.mark.gpu
@pytest.mark.parametrize('R,C', COL_CASES)
def test_column_reductions_at_the_row_count_edges(R, C):
    """qagnn_colreduce_f32 (plain, grouped, row-weighted, scaled sums; plain, row-weighted, scaled squared deviations; the BatchNorm + ReLU
    backward reductions), qagnn_bn_relu_bwd_f32 and qagnn_bn_relu_bwd_colsum_f32 with batch, running and row-weighted statistics, under the
    bars of test_column_reductions_and_bn_backward and test_bn_relu_backward_with_colsum_by_product; at EVERY R the by-product column sums
    are the bits of a separate mode-0 pass."""
    c, log = col_case(R, C), []
    try:
        check_col_outputs(c, run_col_kernels(hip(), c), log, col_emulation(c))
    finally:
        _figure(f'col[{R}x{C}]', log)


@pytest.mark.gpu
@pytest.mark.parametrize('tiles,tail', STAT_CASES)
def test_bn_stats_finalize_at_the_tile_count_edges(tiles, tail):
    """qagnn_bn_stats_finalize_f32 on the partials of an fp32 [R, 32] matrix (mean 5 +- 3 per column, spread 1.4, marker last row) against
    the float64 statistics of that matrix, under the bars of test_gemm_column_statistics_and_bn_stats_finalize."""
    c, log = stat_case(tiles, tail), []
    rm, rv, nbt = c.rm0.clone().cuda(), c.rv0.clone().cuda(), torch.tensor(7, dtype=torch.long, device='cuda')
    try:
        stats = hip().bn_stats_finalize(c.part.cuda(), c.R, c.gamma.cuda(), c.beta.cuda(), 1e-5, running=(rm, rv, nbt, c.pos.cuda(), 0.1, c.unb))
        check_stat_outputs(c, (stats.cpu(), rm.cpu(), rv.cpu(), int(nbt)), log, stat_emulation(c))
    finally:
        _figure(f'stats[{tiles} tiles, {tail} last tile, R = {c.R}]', log)


@pytest.mark.gpu
@pytest.mark.parametrize('p', GELU_P)
@pytest.mark.parametrize('n', ELEM_N)
def test_gelu_dropout_at_the_element_count_edges(n, p):
    """qagnn_gelu_dropout_{fwd,bwd}_f32 against the emulation under the bars of test_gelu_dropout_forward_backward_and_mask; the *_amax_f32
    forms give the same bits and leave the bit pattern of max |out| -- the marker float4 at the very end -- in their word."""
    c, log, K = gelu_case(n, p), [], hip()
    try:
        X, dY = c.X.cuda(), c.dY.cuda()
        y, dx = K.gelu_dropout_fwd(X, p, GELU_SEED).cpu(), K.gelu_dropout_bwd(X, dY, p, GELU_SEED).cpu()
        check_gelu_outputs(c, y, dx, log, (EMU.gelu_dropout_fwd(c.X, p, GELU_SEED), EMU.gelu_dropout_bwd(c.X, c.dY, p, GELU_SEED)))
        (y2, wy), (dx2, wdx) = K.gelu_dropout_fwd(X, p, GELU_SEED, amax=True), K.gelu_dropout_bwd(X, dY, p, GELU_SEED, amax=True)
        assert torch.equal(y2.cpu(), y) and torch.equal(dx2.cpu(), dx), 'the maximum by-product changed the output'
        assert wy[0].item() == _bits(y.abs().max()) and wdx[0].item() == _bits(dx.abs().max())
    finally:
        _figure(f'gelu[n = {n}, p = {p}]', log)


@pytest.mark.gpu
@pytest.mark.parametrize('where', ['last', 'first'])
@pytest.mark.parametrize('n', ELEM_N)
def test_absmax_with_the_maximum_in_the_last_float4(n, where):
    x = absmax_operand(n, where)
    check_absmax_word(hip().absmax(x.cuda())[0].item(), x)


@pytest.mark.gpu
@pytest.mark.parametrize('n', NODE_N)
def test_node_prep_at_the_slot_count_edges(n):
    """qagnn_node_prep_f32 with adj_len = 1, n // 2 + 1 and n (subgraph 0: every slot masked) against EMU.node_prep under the bars of
    test_node_prep_on_unquantised_scores."""
    c, log = node_case(n), []
    try:
        score, mask, ridx = hip().node_prep(c.raw.cuda(), c.al.cuda(), c.nt.cuda(), c.cids.cuda())
        check_node_outputs(c, score.cpu(), mask.cpu(), ridx.cpu(), log)
    finally:
        _figure(f'node_prep[n = {n}]', log)
