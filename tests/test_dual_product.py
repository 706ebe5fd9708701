"""The two-output NN product (include/qagnn_hip_dual.h; k_gemm_nn2_dual in csrc/gemm_nn2.hip): a hop's dX = dK|dM|dQ Wx and
dS = dK|dM|dQ Ws from ONE pass over dK|dM|dQ.

What is held:
  * `-m "not gpu"`: the route decision (qagnn_gemm_nn_dual_query, host only): the flagship batch takes the one launch, the 10-subgraph
    batch, the row counts at which the separate products run narrowed column tiles (the 12 800-row MedQA shard among them), other widths,
    a missing maximum and a scratch too small for unregistered images do not.
  * `-m gpu`, bit for bit (fp32 as int32 patterns, NaN positions included): the one launch against the two separate gemm_nn calls at
    DP = 208, SP = 112, K = 624 over the row counts at which the 128-row tile changes (1, 127, 128, 129, 256 + 5, 3 x 128), all four
    combinations of the accumulate flags from pre-filled outputs (NaN where the flag is 0), pitched outputs whose guard columns must come
    back untouched, images from the registry and images packed into the scratch; zero padding columns in B, narrower logical widths
    (No = 200 / 104: the masked last column tile), an all-zero A (maximum word 0), a NaN and an Inf in A.
    The row threshold of the packed forms is lowered to min(M, 128) for the body of each case: M = 1 and 127 lie below 128, where both the
    one launch and the three-MFMA form of the separate calls would otherwise be refused; and the launch runs in mode 2
    (qagnn_nn_dual_enable), which lifts its row-tile condition -- in the default mode so few row tiles keep the two launches.
  * every pair the launch does not take is refused with QAGNN_EUNSUPPORTED, nothing launched, both pre-filled outputs as they were.
  * qagnn_stack_bwd_deferred_f32 with k = 2 at N = 3 x 200 + 37 rows: switch on against switch off, every gradient, dX, the accumulated
    dS and the hops' maximum words bit for bit; the launch counter says the hops took the one launch with the switch on (mode 2, one per
    hop), never with it off, and never in the default mode at these five row tiles.
"""
import contextlib
import ctypes as C
import os
import re
from unittest import mock

import pytest
import torch

import helpers
from qagnn_amd import _lib

DP, SP, K3 = 208, 112, 624
EUNSUPPORTED = 2
M_CASES = [1, 127, 128, 129, 256 + 5, 3 * 128]
GUARD = 2.0 ** 90


# ---- CPU: which pairs take the one launch ---------------------------------------------------------------------------------------------

def _query(lib, M, No1=DP, No2=SP, K=K3, amax=0x3000, A2=None, pack_ws=None, pack_bytes=-1, M2=None):
    """qagnn_gemm_nn_dual_query on made-up, 16-byte aligned addresses (the route looks at presence, equality and alignment only)"""
    a1, a2 = _lib.dual_args(0x10000, K, M, K, amax, 0x20000, No1, No1, 0x30000, No2, No2)
    if A2 is not None:
        a2.A1 = A2
    if M2 is not None:
        a2.M = M2
    return lib.qagnn_gemm_nn_dual_query(C.byref(a1), 0x40000, K, C.byref(a2), 0x50000, K, pack_ws, pack_bytes)


def test_which_shapes_take_the_dual_launch():
    """`-m "not gpu"`.  The route of a pair (A [M, 624]; B1 -> No1, B2 -> No2 columns) as the library decides it, without a device; the default
    row threshold of the packed forms (8192)."""
    from qagnn_amd.build import build
    build(verbose=False)
    lib = _lib.load_library()
    assert lib.qagnn_dual_version() == 1
    with open(os.path.join(helpers.ROOT, 'include', 'qagnn_hip_dual.h')) as f:
        declared = re.findall(r'\b(qagnn_[a-z0-9_]+)\s*\(', f.read())
    assert sorted(declared) == sorted(_lib.EXPORTS_DUAL) and not set(declared) & set(_lib.EXPORTS), declared
    assert lib.qagnn_packed_min_rows(-1) == 8192
    assert _query(lib, 64000) == 1, 'the flagship batch: 320 subgraphs, N = 64 000'
    assert _query(lib, 2000) == 0, 'the 10-subgraph batch lies below the row threshold of the packed forms'
    # between the row threshold and 1.5 row tiles per CU (256 CUs without a device: 384 tiles = 49 152 rows) the separate products run
    # narrowed column tiles and the pair keeps its two launches: the 64-subgraph MedQA shard (12 800 rows) among them
    assert [_query(lib, M) for M in (8191, 8192, 12800, 32768, 49024, 49025, 49152)] == [0, 0, 0, 0, 0, 1, 1]
    assert lib.qagnn_nn_dual_enable(-1) == 1
    try:  # mode 2 lifts that condition, not the row threshold
        lib.qagnn_nn_dual_enable(2)
        assert [_query(lib, M) for M in (8191, 8192, 12800)] == [0, 1, 1]
    finally:
        lib.qagnn_nn_dual_enable(1)
    assert _query(lib, 64000, No1=200, No2=104) == 1, '13 and 7 column tiles with a masked last tile'
    for No1, No2 in [(208, 208), (112, 112), (112, 208), (192, 112), (208, 96), (224, 112), (208, 128)]:
        assert _query(lib, 64000, No1=No1, No2=No2) == 0, (No1, No2)
    assert _query(lib, 64000, K=608) == 1 and _query(lib, 64000, K=620) == 0, 'K a multiple of 8'
    assert _query(lib, 64000, amax=None) == 0, 'a missing maximum'
    assert _query(lib, 64000, A2=0x60000) == 0 and _query(lib, 64000, M2=63999) == 0
    # unregistered images: both must fit the scratch, the second behind the first.  A hop's pack scratch (sized for the projection) does
    need = [((20 * nj + 13) * 2048 + ((nj + 13) * 4 + 15) // 16 * 16 + 15) // 16 * 16 for nj in (13, 7)]
    assert _query(lib, 64000, pack_ws=None, pack_bytes=0) == 0
    assert _query(lib, 64000, pack_ws=0x70000, pack_bytes=sum(need)) == 1
    assert _query(lib, 64000, pack_ws=0x70000, pack_bytes=sum(need) - 16) == 0
    assert _query(lib, 64000, pack_ws=0x70008, pack_bytes=sum(need) + 16) == 0, 'a misaligned scratch counts as none'
    assert lib.qagnn_gemm_nn_pack_bytes(3 * DP, DP, DP) >= sum(need), "a hop's pack scratch holds both images"


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

def _hip():
    from test_hip_kernels import hip
    return hip()


@contextlib.contextmanager
def _small_rows(Kh, rows, mode=2):
    """the row threshold of the packed forms lowered to `rows`, and the two-output launch in `mode` (2: its row-tile condition lifted, so
    that a few row tiles take it -- by default they keep the two launches with narrowed column tiles); both process-wide values put back"""
    was = Kh.nn_dual_enable(mode)
    try:
        with helpers.form_everywhere(rows):
            yield
    finally:
        Kh.nn_dual_enable(was)


def _operands(M, seed, No1=DP, No2=SP, a_kind='randn', zero_pad=None):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K3, generator=g)
    if a_kind == 'zero':
        A.zero_()
    elif a_kind == 'nonfinite':  # one NaN and one Inf, in different rows and k-tiles
        A[M // 3, 5] = float('nan')
        A[(2 * M) // 3, K3 - 9] = float('inf')
    B1n, B2n = torch.randn(No1, K3, generator=g) * 0.1, torch.randn(No2, K3, generator=g) * 0.1
    if zero_pad:
        B1n[zero_pad[0]:] = 0
        B2n[zero_pad[1]:] = 0
    return A.cuda(), B1n.cuda(), B2n.cuda()


def _prefilled(M, No, pad, accumulate, seed):
    """[M, No + pad] buffer: the view's columns random where the product accumulates, NaN where prior contents must be ignored; guards 2^90"""
    buf = torch.full((M, No + pad), GUARD)
    g = torch.Generator().manual_seed(seed)
    buf[:, :No] = torch.randn(M, No, generator=g) if accumulate else float('nan')
    return buf.cuda()


def _both_ways(Kh, A, B1n, B2n, acc1, acc2, pack=True):
    """-> (status, dual buffers, reference buffers): the one launch and the two separate gemm_nn calls from equal pre-filled pitched outputs"""
    M, No1, No2 = A.size(0), B1n.size(0), B2n.size(0)
    am = Kh.absmax(A.contiguous().view(-1))
    fill = [_prefilled(M, No1, 8, acc1, 1), _prefilled(M, No2, 4, acc2, 2)]
    got, want = [f.clone() for f in fill], [f.clone() for f in fill]
    ws = torch.empty(int(Kh.lib.qagnn_gemm_nn_pack_bytes(3 * DP, DP, DP)), dtype=torch.uint8, device='cuda') if pack else None  # a hop's pack scratch
    rc = Kh.gemm_nn_dual(A, B1n, B2n, am, got[0][:, :No1], got[1][:, :No2], accumulate1=acc1, accumulate2=acc2, ws=ws)
    Kh.gemm_nn(A, B1n.t().contiguous(), B1n=B1n, a_amax1=am, out=want[0][:, :No1], accumulate=acc1)
    Kh.gemm_nn(A, B2n.t().contiguous(), B1n=B2n, a_amax1=am, out=want[1][:, :No2], accumulate=acc2)
    torch.cuda.synchronize()
    return rc, got, want, fill


def _assert_same(got, want, what):
    for i in range(2):
        a, b = helpers._bits(got[i]), helpers._bits(want[i])
        assert torch.equal(a, b), f'{what}: output {i + 1}: {int((a != b).sum())} of {a.numel()} elements differ (guard columns included)'


@pytest.mark.gpu
@pytest.mark.parametrize('images', ['registry', 'scratch'])
@pytest.mark.parametrize('M', M_CASES)
def test_dual_equals_the_two_separate_products(M, images):
    """All four accumulate combinations at one row count, from pre-filled pitched outputs (ldc = 208 + 8 and 112 + 4; one-row operands have
    no pitch): every bit of both buffers, guard columns included, equals the two separate launches'; the guards still hold 2^90 and the
    products hold no NaN of the pre-fill's."""
    Kh = _hip()
    A, B1n, B2n = _operands(M, 100 + M)
    tag = 0x44554131
    with _small_rows(Kh, min(M, 128)):
        keep = Kh.prepack([(B1n, None, 2), (B2n, None, 2)], tag) if images == 'registry' else None
        try:
            before = Kh.dual_launches()
            for acc1 in (False, True):
                for acc2 in (False, True):
                    rc, got, want, _ = _both_ways(Kh, A, B1n, B2n, acc1, acc2)
                    assert rc == 0, Kh.lib.qagnn_last_error()
                    _assert_same(got, want, f'M={M} accumulate=({acc1}, {acc2}) {images}')
                    assert bool((got[0][:, DP:] == GUARD).all()) and bool((got[1][:, SP:] == GUARD).all())
                    assert bool(torch.isfinite(got[0][:, :DP]).all()) and bool(torch.isfinite(got[1][:, :SP]).all())
            assert Kh.dual_launches() == before + 4
        finally:
            if keep is not None:
                Kh.prepack_clear(tag)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['zero_pad_columns', 'narrow_widths', 'zero_A', 'nonfinite_A'])
def test_dual_edge_operands(case):
    """M = 256 + 5 (two whole row tiles and a tail).  zero_pad_columns: logical widths 200 and 104 inside No = 208 / 112 with zero rows of B
    behind them -- the pad columns of C are exactly 0.  narrow_widths: No = 200 / 104 themselves (13 and 7 column tiles whose last is masked).
    zero_A: the maximum word is 0.  nonfinite_A: one NaN and one Inf reach the same output positions as in the separate launches."""
    Kh = _hip()
    M = 261
    No1, No2 = (200, 104) if case == 'narrow_widths' else (DP, SP)
    A, B1n, B2n = _operands(M, 7, No1, No2, a_kind={'zero_A': 'zero', 'nonfinite_A': 'nonfinite'}.get(case, 'randn'),
                            zero_pad=(200, 104) if case == 'zero_pad_columns' else None)
    with _small_rows(Kh, 128):
        for acc in ((False, False), (True, True)):
            rc, got, want, _ = _both_ways(Kh, A, B1n, B2n, *acc)
            assert rc == 0, Kh.lib.qagnn_last_error()
            _assert_same(got, want, f'{case} accumulate={acc}')
            assert bool((got[0][:, No1:] == GUARD).all()) and bool((got[1][:, No2:] == GUARD).all())
            if case == 'zero_pad_columns' and not acc[0]:
                assert bool((got[0][:, 200:DP] == 0).all()) and bool((got[1][:, 104:SP] == 0).all())
            if case == 'zero_A' and not acc[0]:
                assert bool((got[0][:, :DP] == 0).all()) and bool((got[1][:, :SP] == 0).all())
            if case == 'nonfinite_A' and not acc[0]:
                bad = ~torch.isfinite(got[0][:, :DP])
                assert bool(bad[M // 3].all()) and bool(bad[(2 * M) // 3].all()) and int(bad.any(1).sum()) == 2


@pytest.mark.gpu
@pytest.mark.parametrize('why', ['other_A', 'other_M', 'second_segment', 'bias', 'widths_13_13', 'widths_7_7', 'below_threshold', 'no_maximum',
                                 'few_row_tiles'])
def test_unsupported_pairs_are_refused_before_anything_runs(why):
    """QAGNN_EUNSUPPORTED, no launch counted, both NaN / random pre-filled outputs bit for bit as they were.  The row-tile condition is lifted
    (mode 2) so that each case is refused for its own reason -- but for few_row_tiles, the same valid pair of 256 rows in the default mode:
    two row tiles are far below 1.5 per CU."""
    Kh = _hip()
    M = 127 if why == 'below_threshold' else 256
    No1 = SP if why == 'widths_7_7' else DP
    No2 = DP if why == 'widths_13_13' else SP
    A, B1n, B2n = _operands(M, 9, No1, No2)
    other = torch.randn(M, K3, device='cuda')
    bias = torch.zeros(No1, device='cuda')
    am = Kh.absmax(A.view(-1))
    fill = [_prefilled(M, No1, 8, True, 1), _prefilled(M, No2, 4, False, 2)]
    got = [f.clone() for f in fill]
    a1, a2 = _lib.dual_args(A.data_ptr(), K3, M, K3, None if why == 'no_maximum' else am.data_ptr(), got[0].data_ptr(), No1 + 8, No1,
                          got[1].data_ptr(), No2 + 4, No2, True, False)
    if why == 'other_A':
        a2.A1 = other.data_ptr()
    elif why == 'other_M':
        a2.M = M - 1
    elif why == 'second_segment':
        a1.A2, a1.lda2, a1.K2 = other.data_ptr(), K3, 8
    elif why == 'bias':
        a1.bias = bias.data_ptr()
    ws = torch.empty(int(Kh.lib.qagnn_gemm_nn_pack_bytes(3 * DP, DP, DP)), dtype=torch.uint8, device='cuda')
    with _small_rows(Kh, 128, mode=1 if why == 'few_row_tiles' else 2):
        before = Kh.dual_launches()
        rc = Kh.lib.qagnn_gemm_nn_dual_f32(C.byref(a1), B1n.data_ptr(), K3, C.byref(a2), B2n.data_ptr(), K3, ws.data_ptr(), ws.numel(), Kh._stream())
        torch.cuda.synchronize()
        assert rc == EUNSUPPORTED, (rc, Kh.lib.qagnn_last_error().decode())
        assert Kh.dual_launches() == before
    for i in range(2):
        assert torch.equal(helpers._bits(got[i]), helpers._bits(fill[i])), f'{why}: a refused call wrote to output {i + 1}'


@pytest.mark.gpu
def test_stack_backward_takes_the_dual_launch_and_keeps_every_bit():
    """qagnn_stack_bwd_deferred_f32, k = 2, N = 637 rows at DP = 208 / SP = 112 with the row threshold lowered to 128: the switch on against the
    switch off from NaN-filled buffers -- parameter gradients, the gradients handed from hop to hop, dX, the dS both hops add to, the maximum
    words: all bits equal.  On (mode 2: the row-tile condition lifted): one two-output launch per hop; off: none; the default mode: none
    either at five row tiles.  The runtime places two blocks of the kernel on a CU."""
    import test_deferred_reductions as TD
    Kh = _hip()
    case = {'dual_637': (lambda: TD._graph(21, 3 * 200 + 37, 2400, 3, 2), 52, (2,), True)}
    with _small_rows(Kh, 128), mock.patch.dict(TD.DEFER_CASES, case):
        st = TD._Stack('dual_637', 2)
        assert (st.DP, st.SP, st.g.N) == (DP, SP, 637)
        n0 = Kh.dual_launches()
        on = st.backward('deferred')
        n1 = Kh.dual_launches()
        Kh.nn_dual_enable(0)
        off = st.backward('deferred')
        n2 = Kh.dual_launches()
        Kh.nn_dual_enable(1)  # the default mode: five row tiles keep the two launches
        default = st.backward('deferred')
        n3 = Kh.dual_launches()
    assert n3 == n2 and Kh.lib.qagnn_dual_blocks_per_cu() == 2
    TD._same(default, off, 'the stack backward in the default mode against the two launches')
    assert (n1 - n0, n2 - n1) == (2, 0), (n0, n1, n2)
    n = TD._same(on, off, 'the stack backward with the two-output launch against the two launches')
    words = on['amax'][:, _lib.HOP_AM_DKMQ].tolist()
    assert all(0 < w < 0x7F000000 for w in words), f'the backward maxima {words}: the three-MFMA form did not run'
    assert bool(torch.isfinite(on['dX']).all()) and bool(torch.isfinite(on['dS']).all())
    print(f'FIGURE dual stack: {n} elements equal with the switch on and off; launches on / off = {n1 - n0} / {n2 - n1}; '
          f'blocks per CU as the runtime reports them: {Kh.lib.qagnn_dual_blocks_per_cu()}')
