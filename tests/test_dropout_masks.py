"""The dropout keep masks as random variables: rate, independence across sites, layers, heads, epochs and ranks, no period, no shared stream.

Every site draws its mask from uniform01(seed, element index) of csrc/common.h with a seed of ops.next_seed(); under graph replay the kernels
add epoch * EPOCH_MULT to the seed.  The other test files compare every mask with the numpy twin bit for bit -- but the twin restates the
kernels' index formula and the oracle is handed the kernels' masks, so a mask that is wrong as a random variable passes them all.  Here:

  * `-m "not gpu"`: known answers of the hash from plain integers (SplitMix64, state 0) for both twins, with the 64-bit wraps; the constants of
    csrc/common.h and ops.py read out of the sources; the PROOF that no two seed streams the library can draw overlap inside a mask
    (test_no_two_seed_streams_overlap states the ranges); the statistical helpers of helpers.py on the twin at exactly the seeds, shapes and
    rates of the GPU tests, and on doctored masks, each of which they must reject.
  * `-m gpu`: the masks read off the kernels' outputs through the C ABI at p = 2^-24, 0.2, 0.5, 1 - 2^-12 for every site (GELU + dropout,
    pooling attention, both masks of the head, the hop's and the stack's built-in GELU + dropout), forward against backward; epochs; the
    seeds the module hands out over two eager steps, on another rank, and under GraphedStep.

Bars: helpers.MASK_Z = 6 standard deviations of a binomial count (see helpers.py); seeds are fixed.  Where the twin itself left a bar at the
first seed tried, a later counter value was taken (RETRY below, found by running the `not gpu` test on the twin alone): at q = 2^-12 a row
of 208 draws with two kept elements is 8.6 standard deviations out, and a mask of 1024 such rows holds 1.3 of them on average.  At the two
extreme rates the normal bar is narrower than one count for a short line (64 draws at q = 2^-12: one kept element is 7.9 standard
deviations out, and 1.6 % of the lines hold one), so the row / column helper pools neighbouring lines until the bar is one count wide
(helpers._pooled_lines_z); at p = 0.2 and 0.5 nothing is pooled.
"""
import itertools
import os
import re
import time

import numpy as np
import pytest
import torch

import emu_kernels
import helpers
from emu_kernels import EmuGraph
from helpers import MASK_LAGS, MASK_Z, check_independent, check_mask, keep_probability, mask_figures, twin_mask
from test_hip_kernels import EMU, edge_inputs, hip, side_width
from test_nonfinite import _prm

M64 = (1 << 64) - 1

# ---- the constants, pinned here and read out of the sources (as tests/test_row_counts.py reads its own) -------------------------------------------
GOLDEN, MIX1, MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB  # SplitMix64: increment, the two finaliser multipliers
EPOCH_MULT = 0xD1B54A32D192ED03
SEED_MULT, COUNTER_MULT, RANK_MULT = 0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D27D4EB4F
SPLITMIX64_STATE0 = (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F)  # the published first outputs for state 0

H = r'(0x[0-9A-Fa-f]+)'
CONSTANT_PATTERNS = {
    'GOLDEN': ('qagnn_amd/csrc/common.h', r'uint64_t z = seed \+ \(idx \+ 1\) \* ' + H + r'ull;', GOLDEN),
    'MIX1': ('qagnn_amd/csrc/common.h', r'z = \(z \^ \(z >> 30\)\) \* ' + H + r'ull;', MIX1),
    'MIX2': ('qagnn_amd/csrc/common.h', r'z = \(z \^ \(z >> 27\)\) \* ' + H + r'ull;', MIX2),
    'SHIFT3': ('qagnn_amd/csrc/common.h', r'z = z \^ \(z >> (\d+)\);\s+return \(float\)\(z >> 40\) \* \(1\.0f / 16777216\.0f\);', 31),
    'EPOCH_MULT': ('qagnn_amd/csrc/common.h', r'return epoch \? seed \+ \(uint64_t\)epoch\[0\] \* ' + H + r'ull : seed;', EPOCH_MULT),
    'SEED_MULT': ('qagnn_amd/ops.py', r'return \(torch\.initial_seed\(\) \* ' + H + r' \+ _seed_counter\[0\] \* 0x', SEED_MULT),
    'COUNTER_MULT': ('qagnn_amd/ops.py', r' \+ _seed_counter\[0\] \* ' + H + r' \+ _rank\(\) \* 0x', COUNTER_MULT),
    'RANK_MULT': ('qagnn_amd/ops.py', r' \+ _rank\(\) \* ' + H + r'\) % \(2 \*\* 63\)', RANK_MULT),
    # the two numpy twins restate the three hash constants: a change of the hash must change them in the same commit
    'twin GOLDEN': ('tests/helpers.py', r'\(idx\.astype\(np\.uint64\) \+ np\.uint64\(1\)\) \* np\.uint64\(' + H + r'\)', GOLDEN),
    'emu GOLDEN': ('tests/emu_kernels.py', r'\(idx\.astype\(np\.uint64\) \+ np\.uint64\(1\)\) \* np\.uint64\(' + H + r'\)', GOLDEN),
}


def _find(name):
    fn, pattern, _ = CONSTANT_PATTERNS[name]
    with open(os.path.join(helpers.ROOT, fn)) as f:
        found = set(re.findall(pattern, f.read()))
    return int(found.pop(), 0) if len(found) == 1 else None


def test_the_seed_and_hash_constants_are_the_ones_in_the_sources():
    """`-m "not gpu"`.  Every multiplier of uniform01 / epoch_seed (csrc/common.h) and of ops.next_seed is found where it is used and has the
    value the proofs and known answers of this file rest on; the reduction mod 2^63 of next_seed is part of the pattern."""
    got = {name: _find(name) for name in CONSTANT_PATTERNS}
    wrong = {name: (None if v is None else hex(v)) for name, v in got.items() if v != CONSTANT_PATTERNS[name][2]}
    assert not wrong, f'constants changed or no longer found (pattern of CONSTANT_PATTERNS): {wrong}'


# ---- known answers ------------------------------------------------------------------------------------------------------------------------------
def splitmix64_outputs(state, count):
    """the first `count` outputs of SplitMix64 from `state`, in plain Python integers"""
    out = []
    for _ in range(count):
        state = (state + GOLDEN) & M64
        z = state
        z = ((z ^ (z >> 30)) * MIX1) & M64
        z = ((z ^ (z >> 27)) * MIX2) & M64
        out.append(z ^ (z >> 31))
    return out


def uniform01_int(seed, idx):
    """uniform01(seed, idx) in plain integers: the top 24 bits of the output SplitMix64 gives idx + 1 steps after state `seed`"""
    z = (seed + (idx + 1) * GOLDEN) & M64
    z = ((z ^ (z >> 30)) * MIX1) & M64
    z = ((z ^ (z >> 27)) * MIX2) & M64
    return ((z ^ (z >> 31)) >> 40) / 16777216.0


TWINS = {'helpers.uniform01': helpers.uniform01, 'emu_kernels._uniform01': emu_kernels._uniform01}


@pytest.mark.parametrize('twin', sorted(TWINS))
def test_hash_known_answers(twin):
    """`-m "not gpu"`.  uniform01(0, i) is the top 24 bits of the i-th SplitMix64 output for state 0: the integer code reproduces the published
    sequence, and both numpy twins equal the integer code -- there, at a seed above 2^63 and at indices above 2^32 (the 64-bit wraps of
    seed + (idx + 1) * GOLDEN and of the two multiplications)."""
    assert tuple(splitmix64_outputs(0, 3)) == SPLITMIX64_STATE0
    f = TWINS[twin]
    idx = np.arange(16, dtype=np.uint64)
    assert f(0, idx).tolist() == [(z >> 40) / 16777216.0 for z in splitmix64_outputs(0, 16)]
    assert f(0, idx).dtype == np.float32
    big_seed, big_idx = (1 << 63) + 0x123456789ABCDEF, np.array([(1 << 32) + 5, (1 << 40) + 3, (1 << 63) + 11, M64 - 1], dtype=np.uint64)
    for seed, ids in ((big_seed, idx), (12345, big_idx), (big_seed, big_idx), (M64, idx)):
        assert f(seed, ids).tolist() == [uniform01_int(seed, int(i)) for i in ids], (hex(seed), ids)


# ---- no two streams overlap --------------------------------------------------------------------------------------------------------------------
def largest_mask_elements():
    """the largest mask the library draws at the sizes bench.py runs: the GELU one, node rows x padded width of its largest configuration"""
    import bench
    from qagnn_amd import ops
    DP = ops.HeadLayout(bench.D, 'cpu').DP
    return max(w['questions'] * w['nc'] * w['n'] for w in bench.WORKLOADS.values()) * DP


def nmax():
    """the next power of two above the largest mask"""
    return 1 << int(largest_mask_elements()).bit_length()


def _bench_like_case():
    import bench
    return dict(shape='tiny', nq=2, nc=3, n=20, n_rel=17, std=1.0, train=True, seed=11,
                cfg=helpers.model_cfg(d=32, k=bench.K_LAYERS, sent_dim=24, n_concept=300, concept_in_dim=16))


def sites_per_step():
    """next_seed() calls of one train-mode forward with every rate > 0, counted on the emulation provider at the bench's layer count"""
    import test_hip_parity as T
    from qagnn_amd import ops
    cd = _bench_like_case()
    old = ops.set_kernels(EMU)
    try:
        with torch.random.fork_rng(devices=[]):
            model = T._package_model(cd, 'cpu', T.RUN_SCRIPT_DROPOUT)
            args, _ = T._case_args(cd)
            with helpers.SeedRecorder() as rec:
                model(*args[:5], (args[5], args[6]))
    finally:
        ops.set_kernels(old)
    return len(rec.seeds)


G_INV = pow(GOLDEN, -1, 1 << 64)


def shift_of(delta):
    """n with delta == n * GOLDEN (mod 2^64), as a distance |n| (uint64 array in, uint64 array out): stream seed + delta is stream seed moved
    by n elements"""
    with np.errstate(over='ignore'):
        n = delta.astype(np.uint64) * np.uint64(G_INV)
        return np.minimum(n, np.uint64(0) - n)


def seed_differences(D):
    """The differences s2 - s1 (mod 2^64) two seeds of next_seed can have when their unreduced values differ by D (uint64 array: the integer
    difference mod 2^64, two's complement for a negative one): each seed is reduced mod 2^63, so s2 - s1 is D mod 2^63, or that minus 2^63
    when the reduction wrapped in between."""
    d = D.astype(np.uint64) & np.uint64((1 << 63) - 1)
    return np.concatenate([d, d | np.uint64(1 << 63)])


def closest_shift(deltas):
    return int(shift_of(deltas).min())


def test_no_two_seed_streams_overlap():
    """`-m "not gpu"`.  THE CLAIM.  Two masks drawn with seeds s1, s2 share elements (one is the other moved by n indices) exactly when
    s2 - s1 == n * GOLDEN (mod 2^64).  With NMAX = the next power of two above the largest mask of bench.py's configurations (2^25 for
    102 400 rows x 208 columns), no seed difference the library can produce has |n| < NMAX, for
      (a) two calls of next_seed() in one process whose call counters differ by 0 < |c| < 2^20 -- about 10^5 eager steps of the module's
          sites (sites per step: counted on the emulation provider, k + 5 = 10 at the bench's five layers);
      (b) two replays of a captured step whose epochs differ by 1 <= e <= 2^16, any two sites of the step (|c| <= sites per step, c = 0
          included: one site against itself);
      (c) two ranks that differ by 1 .. 7 and |c| < 2^20 (c = 0 included).
    In (a) and (c) the seeds are reduced mod 2^63 as next_seed reduces them, so both values of the difference are covered (wrapped in between
    or not); a negative difference is the mirror image (n -> -n) of a covered one."""
    NMAX = nmax()
    assert NMAX == 1 << 25 and largest_mask_elements() == 128 * 4 * 200 * 208
    S = sites_per_step()
    import bench
    assert S == bench.K_LAYERS + 5
    assert (1 << 20) // S >= 10 ** 5
    assert GOLDEN % 2 == 1 and (GOLDEN * G_INV) & M64 == 1
    c = np.arange(1, 1 << 20, dtype=np.int64)
    worst = {}
    # (a) counter differences
    worst['counter'] = closest_shift(seed_differences((c * np.int64(COUNTER_MULT)).astype(np.uint64)))
    # (b) epoch differences x the counter differences inside one captured step; the epoch term is added by the kernels, mod 2^64
    e = np.arange(1, (1 << 16) + 1, dtype=np.uint64)
    with np.errstate(over='ignore'):
        eterm = e * np.uint64(EPOCH_MULT)
        best = closest_shift(eterm)
        for cc in range(-S, S + 1):
            if cc:
                for sd in seed_differences(np.array([cc * COUNTER_MULT], dtype=np.int64).astype(np.uint64)):
                    best = min(best, closest_shift(eterm + sd))
    worst['epoch'] = best
    # (c) rank differences x counter differences (c = 0 and both signs)
    call = (np.concatenate([-c[::-1], np.zeros(1, dtype=np.int64), c]) * np.int64(COUNTER_MULT)).astype(np.uint64)
    best = 1 << 64
    with np.errstate(over='ignore'):
        for r in range(1, 8):
            best = min(best, closest_shift(seed_differences(call + np.uint64((r * RANK_MULT) & M64))))
    worst['rank'] = best
    print('FIGURE closest shift between two streams, in elements (NMAX = 2^25 = %d): ' % NMAX + ', '.join(f'{k} {v} = 2^{np.log2(v):.1f}' for k, v in worst.items()))
    assert all(v >= NMAX for v in worst.values()), worst
    # the search finds an overlap that is there: stream seed + 1000 * GOLDEN is the stream moved by 1000 elements
    assert closest_shift(np.array([(1000 * GOLDEN) & M64, (-77 * GOLDEN) & M64], dtype=np.uint64)) == 77
    assert np.array_equal(helpers.uniform01(5 + 1000 * GOLDEN, np.arange(50, dtype=np.uint64)), helpers.uniform01(5, np.arange(1000, 1050, dtype=np.uint64)))


# ---- the sites: shapes, strides, seeds (shared by the twin test and the GPU tests) --------------------------------------------------------------
P_LADDER = (2.0 ** -24, 0.2, 0.5, 1.0 - 2.0 ** -12)
P_IDS = ('2^-24', '0.2', '0.5', '1-2^-12')
P_VISIBLE = (0.2, 0.5)  # the rates at which a doctored mask must be rejected (at the two extreme rates a mask holds a handful of 0s or 1s)
POOL = dict(B=64, NH=2, n=200, Cc=208)
HEAD = dict(B=64, NH=2, DP=208, dv=100, n=200, Ds=24, d=200)
HEAD_NO, HEAD_L = HEAD['NH'] * HEAD['dv'], HEAD['NH'] * HEAD['dv'] + HEAD['Ds'] + HEAD['d']
# the hop and the stack: rand_small (50 nodes, 300 edges: the smallest graph of tests/test_head_widths.py that has edges to every node) at
# HP = dh = 64 -- no pad column, so every element of y = gelu(out) * keep shows its mask bit
HOP = dict(graph='rand_small', HP=64, dh=64, k=3, N=50)
# site -> (mask shape, (row pitch, per-head / per-sample strides))
SITES = {
    'gelu-1024x208': ((1024, 208), (208,)),
    'gelu-517x52': ((517, 52), (52,)),  # 26 884 elements = 26 blocks of 1024 + 260: a last block that is part float4s, part nothing
    'pool': ((POOL['B'], POOL['NH'], POOL['n']), (POOL['n'], POOL['NH'] * POOL['n'])),
    'head_pool': ((HEAD['B'], HEAD_NO), (HEAD_NO, HEAD['dv'])),
    'head_fc': ((HEAD['B'], HEAD_L), (HEAD_L,)),
    'hop': ((HOP['N'], 4 * HOP['HP']), (4 * HOP['HP'], HOP['HP'])),
    'stack': ((HOP['N'], 4 * HOP['HP']), (4 * HOP['HP'], HOP['HP'])),  # k seeds from consecutive counter values
    'epoch': ((1024, 208), (208,)),
}
BASE_SEED = 20261019
# (site, index of p) -> how many counter values were passed over because the TWIN's mask left a bar there (module docstring)
RETRY = {('gelu-1024x208', 3): 16}


def seed_of(site, pi, layer=0):
    """a seed as next_seed() forms it, from a counter value of the site's own"""
    counter = 1 + 10000 * sorted(SITES).index(site) + 1000 * pi + 10 * RETRY.get((site, pi), 0) + layer
    return (BASE_SEED * SEED_MULT + counter * COUNTER_MULT) % (1 << 63)


EPOCHS = (0, 1, 2, (1 << 32) + 1)
COMMON_SHAPE, COMMON_P = (256, 208), 0.2  # the masks drawn from the module's recorded seeds
MODULE_SEED = 777


def _site_masks_of_the_twin(site, pi):
    shape, strides = SITES[site]
    p = P_LADDER[pi]
    if site == 'stack':
        return [twin_mask(seed_of(site, pi, l), shape, p) for l in range(HOP['k'])]
    if site == 'epoch':
        return [twin_mask(seed_of(site, pi), shape, p, e) for e in EPOCHS]
    return [twin_mask(seed_of(site, pi), shape, p)]


def _twin_site_figures(site, pi, log=None):
    shape, strides = SITES[site]
    p = P_LADDER[pi]
    masks = _site_masks_of_the_twin(site, pi)
    for j, m in enumerate(masks):
        check_mask(m, p, strides, f'twin {site}[{j}] p = {P_IDS[pi]}', log)
    for (i, a), (j, b) in itertools.combinations(enumerate(masks), 2):
        check_independent(a, b, p, strides, f'twin {site}[{i}] x [{j}] p = {P_IDS[pi]}', log)


@pytest.mark.parametrize('site', sorted(SITES))
def test_the_twin_stays_inside_every_bar_at_the_gpu_tests_inputs(site):
    """`-m "not gpu"`.  Every helper on the numpy twin at exactly the seeds, shapes and rates of the GPU tests: the reference alone is inside
    the bars, so a GPU failure is the kernel's.  The k masks of the stack and the masks of the four epochs: pairwise independent too."""
    log = []
    for pi in range(len(P_LADDER)):
        if site == 'epoch' and P_LADDER[pi] not in P_VISIBLE:
            continue
        _twin_site_figures(site, pi, log)
    worst = {}
    for _, fig in log:
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f'FIGURE twin[{site}]: worst z ' + ' | '.join(f'{k} {v:.2f}' for k, v in worst.items()) + f' (bar {MASK_Z})')


def _rate_resolution(n, p):
    """the smallest offset of the keep rate that n draws show at MASK_Z"""
    q = keep_probability(p)
    return MASK_Z * (q * (1 - q) / n) ** 0.5


@pytest.mark.parametrize('p', P_VISIBLE)
def test_the_helpers_reject_doctored_masks(p):
    """`-m "not gpu"`.  The negative controls, at the shapes of the GPU tests: one mask used for two sites; a mask moved by one index; a pooling
    mask that is the same for every head; a mask that repeats with the row pitch; a column that is always dropped; a rate that is off by 0.01.
    The 212 992 draws of the GELU site resolve 0.01 (asserted); a site with fewer draws is held to 1.5 x what its count resolves at MASK_Z
    (pool: 25 600 draws, 0.015 at p = 0.2), and the figure is printed."""
    pi = P_LADDER.index(p)
    for site in ('gelu-1024x208', 'pool', 'head_pool', 'head_fc', 'hop'):
        shape, strides = SITES[site]
        seed, n = seed_of(site, pi), int(np.prod(shape))
        m = twin_mask(seed, shape, p)
        check_mask(m, p, strides, site)  # (the genuine mask passes)
        with pytest.raises(AssertionError, match='joint z'):  # one mask in two sites
            check_independent(m, m.clone(), p, strides, site)
        moved = twin_mask(seed, (n + 1,), p)[1:].view(*shape)  # the same stream read one index on
        assert not torch.equal(moved, m)
        check_mask(moved, p, strides, site)  # (as a mask of its own it is fine ...)
        with pytest.raises(AssertionError, match='joint z'):  # ... next to the first it is not
            check_independent(m, moved, p, strides, site)
        period = m.reshape(-1, shape[-1])[:1].expand(n // shape[-1], shape[-1]).reshape(shape)  # every row is row 0
        assert helpers.mask_lag_z(period, p, MASK_LAGS + strides) > MASK_Z
        with pytest.raises(AssertionError, match='lag z'):
            check_mask(period, p, strides, site)
        dead = m.clone().reshape(-1, shape[-1])
        dead[:, 3] = False
        assert helpers.mask_row_col_z(dead.view(shape), p) > MASK_Z
        res = _rate_resolution(n, p)
        off = max(0.01, 1.5 * res)
        if site == 'gelu-1024x208':
            assert off == 0.01
        print(f'FIGURE rate resolution[{site}, p = {p}]: {res:.4f} of {n} draws; doctored offset {off:.4f}')
        for sign in (1, -1):
            with pytest.raises(AssertionError, match='rate z'):
                check_mask(twin_mask(seed, shape, p + sign * off), p, strides, site)
    shape, strides = SITES['pool']
    m = twin_mask(seed_of('pool', pi), shape, p)
    same_heads = m[:, :1].expand(*shape).contiguous()  # the head index ignored: head 1 draws head 0's mask
    assert helpers.mask_rate_z(same_heads, p) <= MASK_Z  # (its rate alone does not show it)
    with pytest.raises(AssertionError, match='lag z'):
        check_mask(same_heads, p, strides, 'pool')
    assert helpers.mask_lag_z(same_heads, p, MASK_LAGS) <= MASK_Z < helpers.mask_lag_z(same_heads, p, strides[:1])  # (the head stride is what sees it)
    # two layers of the stack with one seed
    shape, strides = SITES['stack']
    layers = [twin_mask(seed_of('stack', pi, l), shape, p) for l in (0, 0, 2)]
    with pytest.raises(AssertionError, match='joint z'):
        for a, b in itertools.combinations(layers, 2):
            check_independent(a, b, p, strides, 'stack')


def test_pooled_lines_at_the_extreme_rates():
    """`-m "not gpu"`.  The row / column helper at the two extreme rates, where it pools short lines: the genuine masks of the head pass, a
    column that is always kept (q = 2^-12) or always dropped (q = 1 - 2^-24) does not; at p = 0.2 the helper pools nothing (a single column
    that is off is seen on its own: the dead column of test_the_helpers_reject_doctored_masks)."""
    shape, _ = SITES['head_pool']
    for pi, stuck in ((3, True), (0, False)):
        p = P_LADDER[pi]
        m = twin_mask(seed_of('head_pool', pi), shape, p)
        assert helpers.mask_row_col_z(m, p) <= MASK_Z
        m[:, 5] = stuck
        assert helpers.mask_row_col_z(m, p) > MASK_Z
    q = keep_probability(0.2)
    assert helpers._pooled_lines_z(np.array([3, 4, 0, 4]), 4, q) == helpers.count_z(0, 4, q)  # (lines of 4 draws: each on its own)


# ---- the hop / stack operands (CPU: the emulation, for the probe's guard; GPU: the library) ----------------------------------------------------
def _hop_case():
    HP, dh, k = HOP['HP'], HOP['dh'], HOP['k']
    (ei, et, nt, R, T), _, _, _, qs = edge_inputs(HOP['graph'], HP, 5, dh)
    gen = torch.Generator().manual_seed(77)
    N, DP, Cn, SP = nt.numel(), 4 * HP, R * T * T + T, side_width(HP)
    assert N == HOP['N']
    rnd = lambda *shape, s=0.3: torch.randn(*shape, generator=gen) * s  # noqa: E731
    prms = []
    for _ in range(k):
        # (W2t small: |out| stays below 4.5 -- the float32 tanh form of GELU is exactly 0 from x = -5.2 down, and a zero must be a dropped element)
        Wx_t, Ws_t, W1t, W2t = rnd(DP, 3 * DP, s=0.1), rnd(SP, 3 * DP, s=0.1), rnd(DP, DP, s=0.1), rnd(DP, DP, s=0.02)
        prms.append([Wx_t, None, Ws_t, None, rnd(T, 3 * DP), rnd(Cn, 2 * DP), W1t, None, rnd(DP), 1 + rnd(DP), rnd(DP), W2t, None, rnd(DP), rnd(DP),
                     0.5 + rnd(DP).abs()])
    return dict(graph=(ei, et, nt, R, T), qs=qs, prms=prms, X=rnd(N, DP, s=1.0), S=rnd(N, SP, s=1.0), dy=rnd(N, DP, s=1.0), HP=HP, k=k)


@pytest.mark.parametrize('pi', range(len(P_LADDER)), ids=P_IDS)
def test_the_hop_probe_shows_every_mask_bit_on_the_emulation(pi):
    """`-m "not gpu"`.  The GPU test reads the hop's and the stack's masks off y = gelu(out) * keep: every gelu(out) must be non-zero (no pad
    column at dh = HP, no underflow).  Checked on the float32 emulation of the same operands, whose masks are the twin's."""
    from qagnn_amd import ops
    c, p = _hop_case(), P_LADDER[pi]
    ei, et, nt, R, T = c['graph']
    e = EmuGraph(ei, et, nt, R, T)
    fl = lambda t: t.float()  # noqa: E731
    prms = [_prm(prm, fl) for prm in c['prms']]
    seed = seed_of('hop', pi)
    y, saved = ops.hop_fwd_composed(EMU, e, c['HP'], c['qs'], c['X'], c['S'], nt, prms[0], True, 1e-5, p, seed, True, None)
    assert saved[4].abs().max().item() < 4.5 and bool((emu_kernels._gelu(saved[4]) != 0).all())
    assert torch.equal(y != 0, twin_mask(seed, SITES['hop'][0], p))
    seeds = [seed_of('stack', pi, l) for l in range(c['k'])]
    y, saved = EMU.stack_fwd(e, c['HP'], c['qs'], c['X'], c['S'], nt, prms, True, 1e-5, p, seeds, [None] * c['k'])
    for l in range(c['k']):
        assert saved[6 * l + 4].abs().max().item() < 4.5 and bool((emu_kernels._gelu(saved[6 * l + 4]) != 0).all()), f'layer {l}'


# ---- the module's own seeds (CPU: on the emulation provider; GPU: on the library) ----------------------------------------------------------------
def _module_steps(device, monkeypatch, rank=0, steps=2):
    """`steps` eager train-mode steps of the smallest model configuration of helpers (small_train: d = 32, k = 2) with the run scripts' dropout
    rates -> (the seeds next_seed handed out, the provider calls that took a seed, [(seeds, calls) counted after every step])"""
    import test_hip_parity as T
    from qagnn_amd import ops
    cd = helpers.GOLDEN_CASES['small_train']
    monkeypatch.setattr(ops, '_rank', lambda: rank)
    old = ops._seed_counter[0]
    with torch.random.fork_rng(devices=[]):
        model = T._package_model(cd, device, T.RUN_SCRIPT_DROPOUT)
        args, _ = T._case_args(cd)
        dargs = [a.to(device) for a in args]
        torch.manual_seed(MODULE_SEED)
        ops._seed_counter[0] = 0
        try:
            with helpers.SeedRecorder() as rec, helpers.SeedSpy() as spy:
                marks = []
                for _ in range(steps):
                    model.zero_grad()
                    logits, _ = model(*dargs[:5], (dargs[5], dargs[6]))
                    logits.sum().backward()
                    marks.append((len(rec.seeds), len(spy.calls)))
        finally:
            ops._seed_counter[0] = old
    return rec.seeds, spy.calls, marks


def _with_p(calls, suffix):
    return sorted((p, s) for name, got in calls if name.endswith(suffix) for p, s in got if p > 0)


def check_module_seeds(device, monkeypatch, draw):
    """The assertions of the module-seed tests; draw(seed) -> a keep mask of COMMON_SHAPE at COMMON_P from the provider under test."""
    k = helpers.GOLDEN_CASES['small_train']['cfg']['k']
    seeds, calls, marks = _module_steps(device, monkeypatch)
    per_step = k + 5  # dropout_e, the k hops, the stack's output dropout, pooling attention, pooling output, dropout_fc
    assert len(seeds) == 2 * per_step and marks[0][0] == per_step, (len(seeds), marks)
    assert len(set(seeds)) == len(seeds), 'two sites of two steps drew one seed'
    assert all(0 < s < 1 << 63 for s in seeds)
    for step in range(2):
        lo, hi = (0, marks[0][1]) if step == 0 else (marks[0][1], marks[1][1])
        fwd, bwd = _with_p(calls[lo:hi], '_fwd'), _with_p(calls[lo:hi], '_bwd')
        mine = seeds[step * per_step:(step + 1) * per_step]
        # every site with p > 0 received a seed of this step's, each seed went to exactly one site, no site ran with p > 0 on seed 0
        given = [s for _, s in fwd]
        assert len(set(given)) == len(given), f'step {step}: two sites (or two layers of the stack) were handed one seed: {sorted(given)}'
        assert sorted(given) == sorted(mine), (step, fwd, mine)
        assert bwd == fwd, f'step {step}: the backward used other (p, seed) pairs than the forward'
        rates = sorted(p for p, _ in fwd)
        assert rates == sorted([0.2] * (k + 3) + [0.1] * 2), rates
    other, _, _ = _module_steps(device, monkeypatch, rank=1)
    assert len(other) == len(seeds) and not set(other) & set(seeds), 'rank 1 shares a seed with rank 0'
    log = []
    masks = [draw(s) for s in seeds[:per_step]]
    for (i, a), (j, b) in itertools.combinations(enumerate(masks), 2):
        check_independent(a, b, COMMON_P, (COMMON_SHAPE[1],), f'module seeds {i} x {j}', log)
    for j, b in enumerate(draw(s) for s in other[:per_step]):  # the same site on the two ranks
        check_independent(masks[j], b, COMMON_P, (COMMON_SHAPE[1],), f'module seed {j}: rank 0 x rank 1', log)
    z = max(fig['joint'] for _, fig in log)
    print(f'FIGURE module seeds[{device}]: {len(log)} pairs of masks {COMMON_SHAPE} at p = {COMMON_P}, worst joint z {z:.2f} (bar {MASK_Z})')
    return seeds


def test_module_seeds_on_the_emulation_provider(monkeypatch):
    """`-m "not gpu"`.  test_the_modules_own_seeds on the emulation provider: the seed plumbing of the Python layer is the same code on both,
    and the masks drawn from the recorded seeds are the twin's -- the proof that the GPU test's inputs stay inside the bar."""
    from qagnn_amd import ops
    old = ops.set_kernels(EMU)
    try:
        check_module_seeds('cpu', monkeypatch, lambda s: twin_mask(s, COMMON_SHAPE, COMMON_P))
    finally:
        ops.set_kernels(old)


# ======================================================== GPU ===================================================================================
@pytest.fixture(autouse=True)
def _wall(request):
    t0 = time.perf_counter()
    yield
    if 'gpu' in request.keywords:
        print(f'WALL {request.node.name}: {time.perf_counter() - t0:.2f} s')


def _inv32(p):
    """1.f / (1.f - p) as the kernels form it (IEEE float32 division)"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def held_like_the_twin(mask, site, pi, label, seed=None, epoch=0, strides=None, stats=True):
    """A mask read off a kernel: every single-mask helper under the bar, the twin's figures next to it, and -- the masks being bit-equal --
    the same figures."""
    shape, st = SITES[site]
    p = P_LADDER[pi]
    strides = st if strides is None else strides
    mask = mask.cpu()
    assert mask.shape == tuple(shape) and mask.dtype == torch.bool
    twin = twin_mask(seed_of(site, pi) if seed is None else seed, shape, p, epoch)
    if not stats:  # (an epoch whose masks the twin test did not hold to the bars: the bits only)
        assert torch.equal(mask, twin), f'{label}: {int((mask != twin).sum())} mask bits differ from the twin at epoch {epoch}'
        return mask
    fk, ft = mask_figures(mask, p, strides), mask_figures(twin, p, strides)
    print(f'FIGURE mask[{label}, p = {P_IDS[pi]}]: kept {int(mask.sum())} of {mask.numel()} | ' +
          ' | '.join(f'{k} z {fk[k]:.2f} (twin {ft[k]:.2f})' for k in fk))
    check_mask(mask, p, strides, label)
    assert torch.equal(mask, twin), f'{label}: {int((mask != twin).sum())} mask bits differ from the twin'
    assert fk == ft
    return mask


@pytest.mark.gpu
@pytest.mark.parametrize('pi', range(len(P_LADDER)), ids=P_IDS)
@pytest.mark.parametrize('site', ['gelu-1024x208', 'gelu-517x52'])
def test_gelu_dropout_mask(site, pi):
    """qagnn_gelu_dropout_{fwd,bwd}_f32 on an all-ones input: a non-zero output is a kept element.  Rate, rows / columns and lags under the
    bars; a kept element is gelu(1) / (1 - p) to the bit (at p = 2^-24 that scale is 1 + 2^-23, one ulp: still applied); the maximum-keeping
    form the training step runs gives the same bits; the backward's zero gradients are the forward's dropped elements."""
    K, p, seed = hip(), P_LADDER[pi], seed_of(site, pi)
    X = torch.ones(*SITES[site][0], device='cuda')
    y, y0 = K.gelu_dropout_fwd(X, p, seed), K.gelu_dropout_fwd(X, 0.0, 0)
    assert bool((y0 != 0).all())
    mask = held_like_the_twin(y != 0, site, pi, site).cuda()
    inv = torch.tensor(_inv32(p))
    assert inv.item() > 1.0 and torch.equal(y, torch.where(mask, y0 * inv.cuda(), torch.zeros_like(y0))), 'a kept element is not gelu(x) / (1 - p)'
    ya, _ = K.gelu_dropout_fwd(X, p, seed, amax=True)
    assert torch.equal(ya, y)
    dx = K.gelu_dropout_bwd(X, torch.ones_like(X), p, seed)
    assert torch.equal(dx != 0, mask), 'backward and forward drop different elements'
    dxa, _ = K.gelu_dropout_bwd(X, torch.ones_like(X), p, seed, amax=True)
    assert torch.equal(dxa, dx)


def _pool_inputs():
    B, NH, n, Cc = (POOL[k] for k in ('B', 'NH', 'n', 'Cc'))
    g = torch.Generator().manual_seed(31)
    u = torch.zeros(B, NH, Cc)
    for h in range(NH):
        u[:, h, h] = 1.0  # head h reads column h of K: the linear probe of the backward (dK[b, l, h] is head h's score gradient)
    cvec, Kx = torch.randn(B, NH, generator=g), torch.randn(B, n, Cc, generator=g) * 0.3
    return u, cvec, Kx, torch.zeros(B, n, dtype=torch.bool)


@pytest.mark.gpu
@pytest.mark.parametrize('pi', range(len(P_LADDER)), ids=P_IDS)
def test_pool_attention_mask(pi):
    """qagnn_pool_attn_{fwd,bwd}_f32 with nothing masked: attn > 0 everywhere, attn_d == 0 is a dropped element.  The head stride (n) and the
    sample stride (NH n) are among the lags.  Kept: attn_d = attn / (1 - p) to the bit.  Backward: with dz = 0, d attn_d = 1 and u = unit
    vectors, dK[b, l, h] = attn (keep / (1 - p) - sum_l attn keep / (1 - p)) / temperature: the softmax backward leaves no zero at a dropped
    element, so its mask bit is recovered as dK / (attn / temperature) + that sum, which is 0 or 1 / (1 - p)."""
    _pool_site(hip(), pi)


def _pool_site(K, pi, epoch=0):
    p, seed, it = P_LADDER[pi], seed_of('pool', pi), 0.5
    u, cvec, Kx, nomask = (t.cuda() for t in _pool_inputs())
    attn, attn_d, z = K.pool_attn_fwd(u, cvec, Kx, nomask, it, p, seed)
    assert bool((attn > 0).all())
    mask = held_like_the_twin(attn_d != 0, 'pool', pi, 'pool', epoch=epoch, stats=epoch == 0).cuda()
    inv = torch.tensor(_inv32(p)).cuda()
    assert torch.equal(attn_d, torch.where(mask, attn * inv, torch.zeros_like(attn))), 'a kept element is not attn / (1 - p)'
    dK, du, dc = K.pool_attn_bwd(u, Kx, it, p, seed, attn, attn_d, torch.zeros_like(z), torch.ones_like(attn))
    ks = 1.0 / (1.0 - float(np.float32(p)))
    a64, m64 = attn.double(), mask.double()
    sdot = (a64 * m64 * ks).sum(2, keepdim=True)
    dat = dK[:, :, :POOL['NH']].double().transpose(1, 2) / (a64 * it) + sdot  # [B, NH, n]: 0 or ks
    assert (dat - m64 * ks).abs().max().item() <= 1e-3 * ks, 'the backward does not regenerate the forward mask'
    assert torch.equal(dat > 0.5 * ks, mask)


def _head_inputs():
    B, NH, DP, dv, n, Ds, d = (HEAD[k] for k in ('B', 'NH', 'DP', 'dv', 'n', 'Ds', 'd'))
    g = torch.Generator().manual_seed(41)
    pos = lambda *shape: 0.5 + torch.rand(*shape, generator=g)  # noqa: E731  (strictly positive: a zero is a dropped element, nothing else)
    NO = NH * dv
    BDv = torch.zeros(NH * DP, NO)
    for h in range(NH):
        BDv[h * DP:(h + 1) * DP, h * dv:(h + 1) * dv] = pos(DP, dv) / DP
    return dict(z=pos(B, NH, DP), attn=pos(B, NH, n) / n, BDv=BDv, bv=pos(NO), sent=pos(B, Ds), K3=pos(B, n, DP), w=pos(HEAD_L), bfc=pos(1))


@pytest.mark.gpu
@pytest.mark.parametrize('pi', range(len(P_LADDER)), ids=P_IDS)
def test_head_post_masks(pi):
    """Both masks of qagnn_head_post_{fwd,bwd}_f32, read off the backward of a linear probe: dlogits = 1 and strictly positive inputs and
    weights, so a zero gradient is a dropped element.  The mask of the pooled vector [B, NH dv] is d out with p_fc = 0, the mask of the
    concatenation [B, L] the addends of d w_fc with p_pool = 0; with both rates on, d out, d sent, dZ and the addends are zero exactly where
    the two masks say.  Kept: d out = w / (1 - p) to the bit.  Forward: the logits are the float64 sum over the elements the backward kept (a
    single other bit moves a logit by a whole term, 50 x the allowance or more: asserted)."""
    _head_site(hip(), pi)


def _head_site(K, pi, epoch=0):
    p = P_LADDER[pi]
    s1, s2 = seed_of('head_pool', pi), seed_of('head_fc', pi)
    t = {k: v.cuda() for k, v in _head_inputs().items()}
    B, n, d, Ds, NO, L = HEAD['B'], HEAD['n'], HEAD['d'], HEAD['Ds'], HEAD_NO, HEAD_L
    pos = EMU._head_pos(d, HEAD['DP'], 'cuda')
    dl = torch.ones(B, device='cuda')

    def run(p1, p2):
        logits, out, asum = K.head_post_fwd(t['z'], t['attn'], t['BDv'], t['bv'], t['sent'], t['K3'], d, t['w'], t['bfc'], p1, p2, s1, s2)
        assert bool((out > 0).all())
        grads = K.head_post_bwd(dl, out, asum, t['BDv'], t['bv'], t['sent'], t['K3'], d, t['w'], p1, p2, s1, s2, n, True)
        return logits, out, dict(zip(('dz', 'dattn', 'dout', 'dsent', 'dZ', 'part'), grads))

    _, _, g1 = run(p, 0.0)
    m1 = held_like_the_twin(g1['dout'] != 0, 'head_pool', pi, 'head_post pooled vector', epoch=epoch, stats=epoch == 0).cuda()
    inv = torch.tensor(_inv32(p)).cuda()
    assert torch.equal(g1['dout'], torch.where(m1, t['w'][:NO] * inv, torch.zeros_like(g1['dout']))), 'a kept element of d out is not w / (1 - p)'
    assert torch.equal(g1['part'][:, :NO] != 0, m1) and bool((g1['part'][:, NO:L] != 0).all()) and bool((g1['dsent'] != 0).all())  # (p_fc = 0 drops nothing)
    _, _, g2 = run(0.0, p)
    m2 = held_like_the_twin(g2['part'][:, :L] != 0, 'head_fc', pi, 'head_post concatenation', epoch=epoch, stats=epoch == 0).cuda()
    assert torch.equal(torch.cat([g2['dout'], g2['dsent'], g2['dZ'][:, pos]], 1) != 0, m2), 'the data gradients and the addends of d w_fc drop different elements'
    if epoch == 0:
        check_independent(m1, m2[:, :NO], p, (NO, HEAD['dv']), 'head_post: pooled vector x concatenation')
    logits, out, g = run(p, p)
    both = m1 & m2[:, :NO]
    assert torch.equal(g['dout'] != 0, both) and torch.equal(g['part'][:, :NO] != 0, both)
    assert torch.equal(torch.cat([g['dsent'], g['dZ'][:, pos]], 1) != 0, m2[:, NO:]) and torch.equal(g['part'][:, NO:L] != 0, m2[:, NO:])
    # forward against the masks the backward showed
    ks = 1.0 / (1.0 - float(np.float32(p)))
    cat = torch.cat([out.double() * m1.double() * ks, t['sent'].double(), t['K3'][:, 0][:, pos].double()], 1)
    terms = cat * m2.double() * ks * t['w'].double()
    # (float32: three roundings per term, two fused adds per thread, eight levels of the block sum -- 13 x 2^-24 of the sum of the terms;
    #  allowed: 4e-6 of it)
    ref, allow = terms.sum(1) + t['bfc'].double(), 4e-6 * terms.abs().sum(1)
    smallest = torch.where(terms > 0, terms, torch.full_like(terms, float('inf'))).min(1).values
    assert bool((smallest > 50 * allow).all())
    assert bool(((logits.double() - ref).abs() <= allow).all()), 'the forward drops other elements than the backward'


def _gpu_hop(K):
    c = _hop_case()
    ei, et, nt, R, T = c['graph']
    cu = lambda t: t.cuda()  # noqa: E731
    g = K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R, T)
    return c, g, nt.cuda(), [_prm(prm, cu) for prm in c['prms']], cu(c['X']), cu(c['S']), cu(c['dy'])


@pytest.mark.gpu
@pytest.mark.parametrize('pi', range(len(P_LADDER)), ids=P_IDS)
def test_hop_and_stack_masks(pi, monkeypatch):
    """The GELU + dropout inside qagnn_hop_fwd_f32 and qagnn_stack_fwd_f32 (k = 3): y is, bit for bit, what qagnn_gelu_dropout_fwd_f32 makes
    of the saved `out` with the same seed, and its zeros are the zeros of that kernel on an all-ones input (every gelu(out) is non-zero:
    asserted).  The masks of the k layers are pairwise independent.  Backward: the hop's gradients are, bit for bit, the composition through
    qagnn_gelu_dropout_bwd_f32 with the same seed (and not with another); the stack's input gradient is that of the chain of hops with the
    same seeds to 1e-4 of its scale, and 100 x farther from a chain that gives layer 1 another seed (p = 0.2 and 0.5)."""
    _hop_site(hip(), pi, monkeypatch)


def _hop_site(K, pi, monkeypatch, epoch=0):
    from qagnn_amd import ops
    p = P_LADDER[pi]
    monkeypatch.setattr(K, 'gemm_split', 1)  # (the exact products, as test_fused_hop_equals_composed_path)
    c, g, nt, prms, X, S, dy = _gpu_hop(K)
    HP, qs, k = c['HP'], c['qs'], c['k']
    ones = torch.ones_like(X)

    def layer_mask(y, out, seed, site, label, l=0):
        assert bool((K.gelu_dropout_fwd(out.contiguous(), 0.0, 0) != 0).all()), 'a zero of gelu(out): the probe cannot see that mask bit'
        assert torch.equal(y, K.gelu_dropout_fwd(out.contiguous(), p, seed)), f'{label}: not the mask of gelu_dropout_fwd with the same seed'
        m = held_like_the_twin(y != 0, site, pi, label, seed=seed, epoch=epoch, stats=epoch == 0)
        assert torch.equal(m.cuda(), K.gelu_dropout_fwd(ones, p, seed) != 0)
        return m

    seed = seed_of('hop', pi)
    args = (g, HP, qs, X, S, nt, prms[0], True, 1e-5, p, seed, True)
    y, saved = K.hop_fwd(*args, None)
    layer_mask(y, saved[4], seed, 'hop', 'hop')
    grads = K.hop_bwd(*args, saved, dy, True, True)
    comp = ops.hop_bwd_composed(K, *args, tuple(saved[:6]), dy, True, True)
    for nm, a, b in zip(('dX', 'dS', 'dWx_t', 'dWs_t', 'dTT', 'dEkEm', 'dW1t', 'db1', 'dgamma', 'dbeta', 'dW2t', 'db2'), grads, comp):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), f'hop backward: {nm} is not the composition with the forward seed'
    if p in P_VISIBLE:
        other = ops.hop_bwd_composed(K, *args[:10], seed + 1, True, tuple(saved[:6]), dy, True, True)
        assert not torch.equal(other[0], grads[0])

    seeds = [seed_of('stack', pi, l) for l in range(k)]
    sargs = (g, HP, qs, X, S, nt, prms, True, 1e-5, p)
    y, ssaved = K.stack_fwd(*sargs, seeds, [None] * k)
    KMQ, aa, rows, stats = ssaved[:4]
    assert torch.equal(y, rows[k - 1, 3])
    masks = [layer_mask(rows[l, 3], rows[l, 2], seeds[l], 'stack', f'stack layer {l}', l) for l in range(k)]
    if epoch:
        return
    log = []
    for (i, a), (j, b) in itertools.combinations(enumerate(masks), 2):
        check_independent(a, b, p, SITES['stack'][1], f'stack layers {i} x {j}', log)
    print(f'FIGURE stack layers, p = {P_IDS[pi]}: worst joint z {max(f["joint"] for _, f in log):.2f} over {len(log)} pairs (bar {MASK_Z})')
    if p in P_VISIBLE:
        dX = K.stack_bwd(*sargs, seeds, ssaved, dy, True, True)[0]

        def chain(sd):
            d = dy
            for l in range(k - 1, -1, -1):
                sv = (KMQ[l], aa[l], rows[l, 0], rows[l, 1], rows[l, 2], stats[l])
                d = K.hop_bwd(g, HP, qs, X if l == 0 else rows[l - 1, 3], S, nt, prms[l], True, 1e-5, p, sd[l], True, sv, d.contiguous(), True, True)[0]
            return d
        scale = dX.abs().max().item()
        same, wrong = ((dX - chain(sd)).abs().max().item() / scale for sd in (seeds, [seeds[0], seeds[1] + 1] + seeds[2:]))
        print(f'FIGURE stack backward, p = {P_IDS[pi]}: {same:.2e} of scale from the chain with the forward seeds, {wrong:.2e} with another seed in layer 1')
        assert same <= 1e-4 < 1e-2 <= wrong


@pytest.mark.gpu
@pytest.mark.parametrize('p', P_VISIBLE)
def test_epochs_draw_independent_masks(p):
    """One seed at the epochs 0, 1, 2 and 2^32 + 1 (qagnn_seed_epoch_set): each mask under the bars and equal to the twin's at
    seed + epoch * EPOCH_MULT, the four pairwise independent; advance(1) twice is set(2), bit for bit."""
    K, pi = hip(), P_LADDER.index(p)
    seed, (shape, strides) = seed_of('epoch', pi), SITES['epoch']
    X = torch.ones(*shape, device='cuda')
    try:
        masks, ys = [], {}
        for e in EPOCHS:
            K.seed_epoch_set(e)
            ys[e] = K.gelu_dropout_fwd(X, p, seed)
            masks.append(held_like_the_twin(ys[e] != 0, 'epoch', pi, f'epoch {e}', epoch=e))
        log = []
        for (i, a), (j, b) in itertools.combinations(enumerate(masks), 2):
            check_independent(a, b, p, strides, f'epochs {EPOCHS[i]} x {EPOCHS[j]}', log)
        print(f'FIGURE epochs, p = {p}: worst joint z {max(f["joint"] for _, f in log):.2f} over {len(log)} pairs (bar {MASK_Z})')
        K.seed_epoch_set(0)
        K.seed_epoch_advance(1)
        assert torch.equal(K.gelu_dropout_fwd(X, p, seed), ys[1])
        K.seed_epoch_advance(1)
        assert torch.equal(K.gelu_dropout_fwd(X, p, seed), ys[2])
        assert torch.equal(K.gelu_dropout_bwd(X, X, p, seed) != 0, masks[2].cuda()), 'the backward reads another epoch than the forward'
    finally:
        K.seed_epoch_set(0)


@pytest.mark.gpu
@pytest.mark.parametrize('p', P_VISIBLE)
def test_every_site_reads_the_epoch(p, monkeypatch):
    """At epoch 2^32 + 1 the pooling attention, both masks of the head, the hop and the stack draw the twin's masks for
    seed + epoch * EPOCH_MULT, and everything else test_pool_attention_mask, test_head_post_masks and test_hop_and_stack_masks assert
    about forward and backward holds there as at epoch 0 (the bars themselves are held at epoch 0, where the twin test proves them)."""
    K, pi, e = hip(), P_LADDER.index(p), EPOCHS[-1]
    try:
        K.seed_epoch_set(e)
        _pool_site(K, pi, epoch=e)
        _head_site(K, pi, epoch=e)
        _hop_site(K, pi, monkeypatch, epoch=e)
    finally:
        K.seed_epoch_set(0)


@pytest.mark.gpu
def test_rate_zero_ignores_the_epoch():
    """p = 0 at every site: the outputs at epoch 5 and 2^32 + 1 are, bit for bit, those at epoch 0 (and nothing is dropped)."""
    K = hip()
    g = torch.Generator().manual_seed(3)
    X = (torch.randn(517, 52, generator=g) * 2).cuda()
    u, cvec, Kx, nomask = (t.cuda() for t in _pool_inputs())
    t = {k: v.cuda() for k, v in _head_inputs().items()}

    def outputs():
        attn, attn_d, z = K.pool_attn_fwd(u, cvec, Kx, nomask, 0.5, 0.0, 99)
        logits, out, asum = K.head_post_fwd(t['z'], t['attn'], t['BDv'], t['bv'], t['sent'], t['K3'], HEAD['d'], t['w'], t['bfc'], 0.0, 0.0, 98, 97)
        back = K.head_post_bwd(torch.ones(HEAD['B'], device='cuda'), out, asum, t['BDv'], t['bv'], t['sent'], t['K3'], HEAD['d'], t['w'], 0.0, 0.0, 98, 97,
                               HEAD['n'], True)
        dK = K.pool_attn_bwd(u, Kx, 0.5, 0.0, 99, attn, attn_d, torch.ones_like(z), torch.ones_like(attn))
        return [K.gelu_dropout_fwd(X, 0.0, 96), K.gelu_dropout_bwd(X, X, 0.0, 96), attn, attn_d, z, logits, out, *back, *dK]
    try:
        base = outputs()
        assert torch.equal(base[2], base[3])  # attn_d is attn
        for e in (5, (1 << 32) + 1):
            K.seed_epoch_set(e)
            for i, (a, b) in enumerate(zip(outputs(), base)):
                assert torch.equal(a, b), f'epoch {e}: output {i} of a p = 0 call changed'
    finally:
        K.seed_epoch_set(0)


@pytest.mark.gpu
def test_the_modules_own_seeds(monkeypatch):
    """Two eager train-mode steps of the smallest model (d = 32, k = 2) on the library, ops.next_seed and the provider calls spied on: every
    site with p > 0 received a seed of its step and no two sites of the two steps the same one; the backward calls took the forward's
    (p, seed) pairs; with ops._rank patched to 1 no seed is shared with rank 0; masks of one common shape drawn by the GELU kernel from the
    recorded seeds of one step -- and from rank 1's seeds of the same sites -- are pairwise independent."""
    K = hip()
    ones = torch.ones(*COMMON_SHAPE, device='cuda')

    def draw(seed):
        m = (K.gelu_dropout_fwd(ones, COMMON_P, seed) != 0).cpu()
        assert torch.equal(m, twin_mask(seed, COMMON_SHAPE, COMMON_P))
        return m
    check_module_seeds('cuda', monkeypatch, draw)


@pytest.mark.gpu
def test_graphed_step_replays_the_seeds_of_its_capture(monkeypatch):
    """GraphedStep (k = 5, every rate > 0): the first call runs its warm-up steps and the capture, each drawing k + 5 seeds; the captured
    launches carry the LAST k + 5, replays draw none, and replay r -- logits, loss, every gradient, bit for bit -- is the eager step on the
    capture's seeds at epoch r."""
    from qagnn_amd import graphed, ops
    from test_graphed import _batch, _eager, _model
    K = hip()
    nc, per_step = 5, 5 + 5
    old = ops._seed_counter[0]
    try:
        with torch.random.fork_rng(devices=[]):
            b, m = _batch(2, nc, 200, 8), _model(0.2)
            torch.manual_seed(MODULE_SEED)
            ops._seed_counter[0] = 0
            step = graphed.GraphedStep(m, nc)

            def replay():
                logits, loss = step(b['sent'], b['cids'], b['nt'], b['ns'], b['al'], b['packed'], b['labels'])
                return logits.clone(), loss.clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
            with helpers.SeedRecorder() as rec, helpers.SeedSpy() as spy:
                replays = [replay()]
            assert len(rec.seeds) == (step.warmup + 1) * per_step and len(set(rec.seeds)) == len(rec.seeds)
            captured = rec.seeds[-per_step:]
            assert spy.seeds('_fwd')[-per_step:] == captured and sorted(spy.seeds('_bwd')[-per_step:]) == sorted(captured)
            with helpers.SeedRecorder() as rec2:
                replays += [replay(), replay()]
            assert not rec2.seeds and step.n_graphs == 1
            for r, (logits, loss, grads) in enumerate(replays):
                K.seed_epoch_set(r)
                feed = iter(captured)
                monkeypatch.setattr(ops, 'next_seed', lambda: next(feed))
                e_logits, e_loss, e_grads, _ = _eager(m, b, nc)
                assert next(feed, None) is None
                assert torch.equal(logits, e_logits) and torch.equal(loss, e_loss), f'replay {r} is not the eager step on the captured seeds at epoch {r}'
                bad = [k for k in grads if not torch.equal(grads[k], e_grads[k])]
                assert set(grads) == set(e_grads) and not bad, f'replay {r}: {len(bad)} gradients differ, e.g. {bad[:3]}'
            assert not torch.equal(replays[0][0], replays[1][0]) and not torch.equal(replays[1][0], replays[2][0])
    finally:
        ops._seed_counter[0] = old
        K.seed_epoch_set(0)
