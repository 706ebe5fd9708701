"""Every row pitch of the C ABI (include/qagnn_hip.h) with a pitch that differs from the width, padded inputs and guarded outputs.

The header gives almost every fp32 entry point a row pitch separate from the row width; the module only ever passes the width.  With
pitch == width three kinds of error are invisible: a width used where the pitch belongs (the same number), a store past a row's width
(it lands in the next row and is overwritten by that row's owner) or past the last row (allocator slack), and a k tail that is not
predicated (the kernels size their buffer descriptors as rows * pitch, so the hardware range check is no check on the columns).

Here every operand of a call is a view into a larger buffer (`pitched`): its rows start `off` floats into rows of `ld` floats, with one
extra row below.  Around an INPUT the buffer holds 2^100 -- finite, so outside the non-finite contract, and the ruin of any sum it
leaks into.  Around an OUTPUT it holds a canary bit pattern.  Every case asserts (`check_three`):
  (a) the result inside the view meets the float64 emulation (tests/emu_kernels.py on the logical operands) under the bound of the
      kernel's own test in test_hip_kernels.py;
  (b) it is bit-identical to the same call on contiguous copies -- a pitch changes addresses, never arithmetic;
  (c) every element of an output's buffer outside the view still holds the canary, bit for bit (`check_guard`).
`-m "not gpu"`: the same checking code rejects three torch stand-ins for a wrong pitched product, each of which it accepts in its
contiguous form.
"""
import contextlib

import pytest
import torch

import helpers
from test_hip_kernels import (EDGE_OUTPUTS, EMU, EPS, _bound, _h2_bound, check_edge_outputs, edge_case, hip, print_figures, run_edge_kernels)

BIG = 2.0 ** 100      # around every input
CANARY = 0x7FC5A5A5   # around every output: a quiet NaN whose payload no kernel produces; compared as int32


def pitched(t, ld, off, fill, device=None):
    """-> (buf, view): `t` [rows, width] copied into columns [off, off + width) of a [rows + 1, ld] buffer; the margins and the extra row
    below hold `fill` (a float, or an int32 bit pattern).  off is a multiple of 4: the view's base is 16-byte aligned, not pitch aligned."""
    rows, width = t.shape
    assert ld % 4 == 0 and off % 4 == 0 and 0 <= off and off + width <= ld, (ld, off, width)
    if isinstance(fill, int):
        buf = torch.full((rows + 1, ld), fill, dtype=torch.int32).view(torch.float32)
    else:
        buf = torch.full((rows + 1, ld), float(fill), dtype=torch.float32)
    buf[:rows, off:off + width] = t
    buf = buf.to(device if device is not None else t.device)
    return buf, buf[:rows, off:off + width]


def check_guard(buf, view, what='output'):
    """Every element of `buf` outside `view` (the rows of a 2-D or 3-D view of it, all with the pitch of buf) still holds the canary."""
    ld, width = buf.size(1), view.size(-1)
    r0, c0 = divmod(view.storage_offset() - buf.storage_offset(), ld)
    rows = view.numel() // width
    bits = buf.detach().cpu().view(torch.int32).clone()
    assert r0 + rows <= bits.size(0) and c0 + width <= ld
    bits[r0:r0 + rows, c0:c0 + width] = CANARY
    bad = (bits != CANARY).nonzero()
    if bad.numel():
        r, c = bad[0].tolist()
        where = 'below the last row' if r >= r0 + rows else 'in the margin right of the view' if c >= c0 + width else 'in the margin left of the view'
        raise AssertionError(f'(c) {what}: {bad.size(0)} elements outside the view (rows {r0}..{r0 + rows - 1}, columns {c0}..{c0 + width - 1} of a '
                             f'[{bits.size(0)}, {ld}] buffer) were written; the first at row {r}, column {c}, {where}')


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


class Place:
    """Hands a test's logical operands (CPU tensors) to a call: contiguous copies (on=False), or pitched views with 2^100 around the
    inputs and the canary around the outputs (on=True).  slack: floats behind a contiguous output, as a caching allocator leaves them."""

    def __init__(self, on, device='cuda', slack=0):
        self.on, self.device, self.slack, self.guards = on, device, slack, []

    def inp(self, t, extra=8, off=4):
        if t is None:
            return None
        if not self.on:
            return t.contiguous().to(self.device)
        return pitched(t, t.size(1) + extra, off, BIG, self.device)[1]

    def inp3(self, t, extra=8, off=4):
        """[B, n, Cc] node rows: B * n rows with one pitch"""
        return self.inp(t.flatten(0, 1), extra, off).unflatten(0, t.shape[:2])

    def out(self, name, rows, width, extra=8, off=4, init=None):
        if init is None:
            init = torch.zeros(rows, width)
        if not self.on:
            flat = torch.zeros(rows * width + self.slack, device=self.device)
            view = flat[:rows * width].view(rows, width)
            view.copy_(init)
            return view
        buf, view = pitched(init, width + extra, off, CANARY, self.device)
        self.guards.append((name, buf, view))
        return view

    def out3(self, name, B, n, width, extra=8, off=4, init=None):
        return self.out(name, B * n, width, extra, off, None if init is None else init.flatten(0, 1)).unflatten(0, (B, n))

    def check(self):
        for name, buf, view in self.guards:
            check_guard(buf, view, name)


def both(call, device='cuda', slack=0):
    """call(place) -> a tensor or a tuple of tensors, once on contiguous copies and once on pitched views -> (pitched results, contiguous
    results, the pitched Place)"""
    pc, pp = Place(False, device, slack), Place(True, device, slack)
    want, got = call(pc), call(pp)
    if device == 'cuda':
        torch.cuda.synchronize()
    return got, want, pp


def check_three(label, got, want, ref, bound, place=None, log=None):
    """(a), (b), (c) of the module docstring for one output.  `bound`: a tensor like ref or a number, elementwise on |got - ref|.
    place=None leaves (c) to the caller (several outputs, one Place).  All three are evaluated before anything is raised."""
    g = got.detach().cpu()
    err = (g.double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err)  # (a NaN is the worst error, not one max() may skip)
    ratio = (err / bound).max().item() if err.numel() else 0.0
    if log is not None:
        log.append(f'{label} {ratio:.3f}')
    fails = []
    if not ratio <= 1.0:
        fails.append(f'(a) {label}: max err {err.max().item():.3e}, worst error / bound {ratio:.3g}')
    if want is not None and not same_bits(g, want):
        w = want.detach().cpu()
        n = int((g.contiguous().view(torch.int32) != w.contiguous().view(torch.int32)).sum()) if g.shape == w.shape else -1
        fails.append(f'(b) {label}: {n} elements differ in their bits from the same call on contiguous operands')
    if place is not None:
        try:
            place.check()
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, '; '.join(fails)


def figure(label, log):
    """one line per case for the record of a GPU run (profiles/pitched_operands_gpu_tests.txt): per output the worst error / bound"""
    print(f'FIGURE {label}: worst error / bound: ' + ' | '.join(log))


# ---- `-m "not gpu"`: the checks above against wrong kernels ------------------------------------------------------------------------------------

def _standin_product(flaw):
    """A torch stand-in for a product kernel C = A B that is handed what the binding hands the library -- base addresses and pitches -- and
    addresses memory from them.  flaw None: right.  'width_as_pitch': rows of A are taken K floats apart.  'tile_past_No': every row is
    stored in whole 16-column tiles (zeros past No), in row order.  'row_M': a row M of zeros is stored."""
    def run(A, B, C):
        (M, K), No = A.shape, B.size(1)
        lda, ldc = A.stride(0), C.stride(0)
        prod = (A.as_strided((M, K), (K if flaw == 'width_as_pitch' else lda, 1)).double() @ B.double()).float()
        if flaw == 'tile_past_No':
            Nt = -(-No // 16) * 16
            Cw = C.as_strided((M, Nt), (ldc, 1))
            for m in range(M):  # (in row order: in a contiguous C a row's overrun is overwritten by the next row's owner)
                Cw[m] = torch.cat([prod[m], torch.zeros(Nt - No)])
        elif flaw == 'row_M':
            Cw = C.as_strided((M + 1, No), (ldc, 1))
            Cw[:M], Cw[M] = prod, 0.0
        else:
            C.copy_(prod)
        return C
    return run


@pytest.mark.parametrize('flaw,letters', [(None, ''), ('width_as_pitch', 'ab'), ('tile_past_No', 'c'), ('row_M', 'c')])
def test_the_pitched_checks_reject_a_wrong_kernel_the_contiguous_ones_accept(flaw, letters):
    """`-m "not gpu"`.  check_three -- the code every GPU case below runs -- on three wrong product kernels (torch stand-ins on the CPU):
    each passes on contiguous operands, where pitch == width, a column overrun is overwritten by the next row's owner and a row overrun
    lands in allocator slack -- the blindness of a suite that never passes a pitch -- and fails (a), (b) or (c) on pitched, guarded
    operands.  The right product passes all three in both forms."""
    g = torch.Generator().manual_seed(3)
    M, K, No = 37, 24, 40  # (No is no multiple of 16)
    A, B = torch.randn(M, K, generator=g), torch.randn(K, No, generator=g)
    ref = A.double() @ B.double()
    bound = _bound(A.abs().double(), B.abs().double()) + 4 * EPS * ref.abs()
    run = _standin_product(flaw)

    def call(P):
        return run(P.inp(A, 8, 4), P.inp(B, 12, 4), P.out('C', M, No, 16, 4))
    pc = Place(False, 'cpu', slack=64)
    got_c = call(pc)
    check_three('C, contiguous', got_c, got_c, ref, bound, pc)  # pitch == width: every stand-in passes
    got, want, pp = both(call, 'cpu', slack=64)
    if not letters:
        check_three('C', got, want, ref, bound, pp)
        return
    with pytest.raises(AssertionError) as exc:
        check_three('C', got, want, ref, bound, pp)
    for letter in 'abc':
        assert (f'({letter}) ' in str(exc.value)) == (letter in letters), str(exc.value)


def test_pitched_places_what_it_says():
    """`-m "not gpu"`.  The helpers themselves: base aligned to 16 bytes but not to the pitch, fills where they belong, and check_guard
    sees one changed bit left of, right of and below a view -- and nothing inside it."""
    t = torch.arange(15.0).view(3, 5)[:, :4].contiguous()
    buf, view = pitched(t, 12, 4, BIG)
    assert view.shape == (3, 4) and view.stride() == (12, 1) and view.data_ptr() % 16 == 0 and (view.data_ptr() - buf.data_ptr()) % 48 == 16
    assert torch.equal(view, t) and (buf[3] == BIG).all() and (buf[:, :4] == BIG).all() and (buf[:, 8:] == BIG).all()
    P = Place(True, 'cpu')
    o = P.out('o', 3, 4, 8, 4)
    assert o.stride() == (12, 1)
    o.fill_(float('nan'))  # (any value inside the view, a NaN included)
    P.check()
    buf = P.guards[0][1]
    for r, c, where in ((1, 3, 'left of'), (0, 8, 'right of'), (3, 5, 'below')):
        keep = buf[r, c].clone()
        buf.view(torch.int32)[r, c] ^= 1
        with pytest.raises(AssertionError, match=where):
            P.check()
        buf[r, c] = keep
    P.check()
    o3 = P.out3('o3', 2, 3, 4, 8, 4)
    assert o3.shape == (2, 3, 4) and o3.stride() == (36, 12, 1)
    P.check()


# ---- NN products ---------------------------------------------------------------------------------------------------------------------------------

def _nn_operands(M, K1, K2, No, variant, V=0):
    """as test_gemm_nn builds them; V > 0: A1 is a table of V rows gathered through a_rowidx (some rows -1)"""
    g = torch.Generator().manual_seed(M + K1 + No)
    o = dict(A1=torch.randn(V or M, K1, generator=g), B1=torch.randn(K1, No, generator=g), A2=None, B2=None, vec={}, rowtab=None, out0=None, idx=None)
    if K2:
        o['A2'], o['B2'] = torch.randn(M, K2, generator=g), torch.randn(K2, No, generator=g)
    if variant in ('bias_tab', 'stats'):
        o['vec']['bias'] = torch.randn(No, generator=g)
    if variant == 'bias_tab':
        o['rowtab'], o['vec']['rowidx'] = torch.randn(4, No, generator=g), torch.randint(0, 4, (M,), generator=g)
    if variant == 'affine':
        o['vec'].update(a_scale=torch.randn(K1, generator=g), a_shift=torch.randn(K1, generator=g))
    if variant == 'accumulate':
        o['out0'] = torch.randn(M, No, generator=g)
    if V:
        o['idx'] = torch.randint(0, V, (M,), generator=g)
        o['idx'][1::17] = -1
    return o


def _nn_reference(o, three_mfma=False):
    """-> (float64 reference, bound): test_gemm_nn's bound; three_mfma: test_gemm_nn_three_mfma_form's (_h2_bound)"""
    d = lambda t: None if t is None else (t.double() if t.is_floating_point() else t)  # noqa: E731
    kw = {k: d(v) for k, v in o['vec'].items()}
    ref = EMU.gemm_nn(d(o['A1']), d(o['B1']), d(o['A2']), d(o['B2']), rowtab=d(o['rowtab']), a_rowidx=o['idx'], **kw)
    if o['out0'] is not None:
        ref = ref + o['out0'].double()
    A1 = EMU._gather_rows(o['A1'], o['idx'])
    A1e = torch.relu(A1 * o['vec']['a_scale'] + o['vec']['a_shift']) if 'a_scale' in o['vec'] else A1
    if three_mfma:
        return ref, _h2_bound(A1e, o['B1'], o['A2'], o['B2'], ref), A1e
    bound = _bound(A1e.abs().double(), o['B1'].abs().double()) + 4 * EPS * ref.abs()
    if o['A2'] is not None:
        bound = bound + 8 * EPS * (o['A2'].abs().double() @ o['B2'].abs().double())
    return ref, bound, A1e


class _Spy:
    """records the names of the library calls the binding makes"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def _nn_case(K, o, M, No, split, ldc_extra=16, c_off=8, amax=None, register=0, colstats=False):
    """call(place) for K.gemm_nn on the operands `o`: lda1 = K1 + 8, lda2 = K2 + 16, ldb = No + 12, ldn1 = K1 + 8, ldn2 = K2 + 12,
    ldt = No + 8, ldc = No + ldc_extra; register = pieces: B's images are registered first, under the views' own pointers and pitches."""
    cu = lambda t: None if t is None else t.cuda()  # noqa: E731

    def call(P):
        kw = {k: cu(v) for k, v in o['vec'].items()}
        if o['rowtab'] is not None:
            kw['rowtab'] = P.inp(o['rowtab'], 8, 4)
        if split:
            kw['B1n'] = P.inp(o['B1'].t().contiguous(), 8, 4)
            kw['B2n'] = P.inp(o['B2'].t().contiguous(), 12, 8) if o['B2'] is not None else None
        if amax is not None:
            kw['a_amax1'], kw['a_amax2'] = amax
        out = P.out('C', M, No, ldc_extra, c_off, o['out0'])
        if register:
            keep = K.prepack([(kw['B1n'], kw['B2n'], register)], tag=0x917C)
        try:
            res = K.gemm_nn(P.inp(o['A1'], 8, 4), P.inp(o['B1'], 12, 4), P.inp(o['A2'], 16, 8), P.inp(o['B2'], 12, 8), out=out,
                            accumulate=o['out0'] is not None, a_rowidx=cu(o['idx']), colstats=colstats, **kw)
            torch.cuda.synchronize()
        finally:
            if register:
                K.prepack_clear(0x917C)
                del keep
        return res if colstats else (res,)
    return call


NN_VARIANTS = ['plain', 'bias_tab', 'affine', 'accumulate']


@pytest.mark.gpu
@pytest.mark.parametrize('variant', NN_VARIANTS)
@pytest.mark.parametrize('M,K1,K2,No', [(513, 32, 32, 96), (130, 112, 0, 112)])
def test_pitched_nn_fp32_mfma_kernel(M, K1, K2, No, variant):
    """qagnn_gemm_nn_f32 (k_gemm_nn, csrc/gemm.hip): lda1 != lda2, ldb > No, ldc > No, ldt > No"""
    o = _nn_operands(M, K1, K2, No, variant)
    ref, bound, _ = _nn_reference(o)
    call = _nn_case(hip(), o, M, No, split=False)
    (got,), (want,), P = both(call)
    log = []
    try:
        check_three('C', got, want, ref, bound, P, log)
    finally:
        figure(f'nn_fp32[{M}-{K1}-{K2}-{No}-{variant}]', log)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', NN_VARIANTS + ['flat'])
def test_pitched_nn_first_generation_split_kernel(variant):
    """k_gemm_nn_split (csrc/gemm_split.hip) on a shape nn2_ok declines (K2 = 8 < 32 - 200 % 32: the straddling k-tile would leave
    segment 2), B in its [No, K] layout with ldn > K.  flat: its FLAT form -- A1 gathered from a pitched table through a_rowidx next to a
    second segment (a gathered product with K2 > 0 is the first-generation kernel's alone: nn2_ok)."""
    M, K1, K2, No = 300, 200, 8, 320
    o = _nn_operands(M, K1, K2, No, 'plain' if variant == 'flat' else variant, V=150 if variant == 'flat' else 0)
    ref, bound, _ = _nn_reference(o)
    call = _nn_case(hip(), o, M, No, split=True)
    (got,), (want,), P = both(call)
    log = []
    try:
        check_three('C', got, want, ref, bound, P, log)
    finally:
        figure(f'nn_split1[{M}-{K1}-{K2}-{No}-{variant}]', log)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', NN_VARIANTS)
@pytest.mark.parametrize('M,K1,K2,No', [(257, 208, 112, 624), (129, 8, 24, 16), (260, 224, 0, 320)])
def test_pitched_nn_second_generation_kernel_b_in_kernel(M, K1, K2, No, variant):
    """k_gemm_nn2 splitting B itself (csrc/gemm_nn2.hip; below the packed-image row threshold): [208 | 112] has the straddling k-tile,
    whose A1 tail is predicated next to a live margin; a k-tile tail; a straddling tile with a short first segment."""
    o = _nn_operands(M, K1, K2, No, variant)
    ref, bound, _ = _nn_reference(o)
    K = hip()
    call = _nn_case(K, o, M, No, split=True)
    assert M < K.PACK_MIN_M
    (got,), (want,), P = both(call)
    log = []
    try:
        check_three('C', got, want, ref, bound, P, log)
    finally:
        figure(f'nn2_in_kernel[{M}-{K1}-{K2}-{No}-{variant}]', log)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', NN_VARIANTS)
@pytest.mark.parametrize('b', ['scratch', 'registered'])
@pytest.mark.parametrize('M,K1,K2,No', [(2000, 624, 0, 208), (257, 32, 16, 96)])
def test_pitched_nn_second_generation_kernel_packed_b(M, K1, K2, No, b, variant, monkeypatch):
    """k_pack_b + the DMA-fed k_gemm_nn2 at hundreds of rows (helpers.form_everywhere), B [No, K] with ldn > K.  scratch: packed per call
    (qagnn_gemm_nn_split_ws_f32); registered: qagnn_gemm_nn_prepack_f32 with ldn > K in the qagnn_pack_desc, and the product finds the
    image by pointer AND pitch -- the binding is seen to ask for no scratch.  (affine at K1 = 624 leaves the second generation --
    nn2_ok: the scale / shift vectors live in LDS -- and runs, equally pitched, on the first-generation kernel.)"""
    o = _nn_operands(M, K1, K2, No, variant)
    ref, bound, _ = _nn_reference(o)
    K = hip()
    call = _nn_case(K, o, M, No, split=True, register=3 if b == 'registered' else 0)
    spy = _Spy(K.lib)
    monkeypatch.setattr(K, 'lib', spy)
    with helpers.form_everywhere():
        (got,), (want,), P = both(call)
    log = []
    try:
        check_three('C', got, want, ref, bound, P, log)
        if not (variant == 'affine' and K1 > 256):
            used_scratch = 'qagnn_gemm_nn_split_ws_f32' in spy.calls
            assert used_scratch == (b == 'scratch') and (used_scratch or spy.calls.count('qagnn_gemm_nn_split_f32') == 2), spy.calls
    finally:
        figure(f'nn2_packed[{M}-{K1}-{K2}-{No}-{b}-{variant}]', log)


@pytest.mark.gpu
@pytest.mark.parametrize('M,K1,K2,No,b,variant', [(2000, 624, 0, 208, 'scratch', v) for v in ('plain', 'bias_tab', 'accumulate', 'stats')] +
                         [(257, 32, 16, 96, 'scratch', v) for v in NN_VARIANTS] + [(2000, 624, 0, 208, 'registered', 'plain'), (257, 32, 16, 96, 'registered', 'plain')])
def test_pitched_nn_three_mfma_form(M, K1, K2, No, b, variant, monkeypatch):
    """The three-MFMA form (the operand maxima from absmax of the logical operands) on the packed two-piece image, per call and
    registered; held to the form's own bound (test_gemm_nn_three_mfma_form).  stats: colstat_part does not depend on ldc -- bit-identical
    to the contiguous call's, and describing the values stored.  (No affine at K1 = 624: nn2_ok declines it.)  The registered image runs
    the plain variant only, on purpose: it differs from the per-call image in where B's packed pieces come from, not in the epilogue;
    test_pitched_nn_second_generation_kernel_packed_b runs a registered image across the variants, and the plain cases here show that
    the lookup matches on pitch for the two-piece image too."""
    o = _nn_operands(M, K1, K2, No, variant)
    ref, bound, A1e = _nn_reference(o, three_mfma=True)
    K = hip()
    assert K.gemm_split == 2
    amax = (K.absmax(A1e.contiguous().cuda()), K.absmax(o['A2'].cuda()) if K2 else None)
    call = _nn_case(K, o, M, No, split=True, amax=amax, register=2 if b == 'registered' else 0, colstats=variant == 'stats')
    (six_c,) = _nn_case(K, o, M, No, split=True)(Place(False))  # (no maxima: six MFMAs per product, whichever way B travels)
    spy = _Spy(K.lib)
    monkeypatch.setattr(K, 'lib', spy)
    with helpers.form_everywhere():
        got, want, P = both(call)
    log = []
    try:
        check_three('C', got[0], want[0], ref, bound, P, log)
        assert ('qagnn_gemm_nn_split_ws_f32' in spy.calls) == (b == 'scratch'), spy.calls
        if variant == 'plain':
            assert not same_bits(six_c, want[0]), 'the three-MFMA form did not run: the six-MFMA route answered'
        if variant == 'stats':
            part, c64 = got[1], got[0].cpu().double()
            assert same_bits(part, want[1]), 'colstat_part depends on ldc'
            assert torch.equal(part[:, 0].cpu().double(), c64[::128])  # x0 = the tile's first row, as stored
            stat = EMU.col_partials(c64)
            assert (part.cpu().double() - stat).abs().max().item() <= 2e-5 * stat.abs().max().item()  # (test_gemm_column_statistics_and_bn_stats_finalize)
    finally:
        figure(f'nn2_three_mfma[{M}-{K1}-{K2}-{No}-{b}-{variant}]', log)


@pytest.mark.gpu
@pytest.mark.parametrize('route', ['fp32', 'six', 'three'])
def test_pitched_nn_gathered_product(route, monkeypatch):
    """A1 gathered from a table whose pitch exceeds its width (a_rowidx, rows of -1): the fp32-MFMA kernel, the second-generation kernel
    in its default form, and -- at the same 257 rows, helpers.form_everywhere -- the three-MFMA form with the table's maximum as the
    operand word.  Bounds of test_gemm_with_fused_row_gather{,_in_the_three_mfma_form_at_small_m}."""
    M, V, Kd, No = 257, 500, 32, 208
    o = _nn_operands(M, Kd, 0, No, 'stats', V=V)  # (bias only)
    ref, bound, _ = _nn_reference(o)
    K = hip()
    amax = None
    if route == 'three':
        Ag, B = EMU._gather_rows(o['A1'].double(), o['idx']), o['B1']
        bound = 12 * EPS * (Ag.abs() @ B.abs().double()) + 2.0 ** -38 * Kd * o['A1'].abs().max().item() * B.abs().max(0).values.double() + 4 * EPS * ref.abs()
        amax = (K.absmax(o['A1'].cuda().view(-1)), None)
    call = _nn_case(K, o, M, No, split=route != 'fp32', amax=amax)
    with (helpers.form_everywhere() if route == 'three' else contextlib.nullcontext()):
        (got,), (want,), P = both(call)
    log = []
    try:
        check_three('C', got, want, ref, bound, P, log)
        assert (got.cpu()[o['idx'] < 0] == o['vec']['bias']).all()
    finally:
        figure(f'nn_gather[{M}-{V}-{Kd}-{No}-{route}]', log)


@pytest.mark.gpu
def test_pitched_nn_staggered_eight_wave_block():
    """The one large case: k_gemm_nn2's staggered 8-wave form (>= 10 k-tiles, a 256-row tile per CU) stores straight from registers
    through a buffer descriptor sized by ldc; No = 200 in rows of ldc = 208, 4 floats of canary on either side."""
    M, K1, K2, No = 61003, 320, 0, 200
    o = _nn_operands(M, K1, K2, No, 'plain')
    ref, bound, _ = _nn_reference(o)
    K = hip()
    call = _nn_case(K, o, M, No, split=True, ldc_extra=8, c_off=4)
    assert M >= K.PACK_MIN_M
    (got,), (want,), P = both(call)
    log = []
    try:
        check_three('C', got, want, ref, bound, P, log)
    finally:
        figure(f'nn2_staggered[{M}-{K1}-{K2}-{No}-plain]', log)


# ---- TN products (weight gradients) ----------------------------------------------------------------------------------------------------------------
# (named test_pitched_tn_*: test_hip_kernels.py::test_gemm_kernel_families runs them once more with QAGNN_GEMM_SPLIT=0, which pins the
# fp32-MFMA kernels k_gemm_tn_strip / k_gemm_tn for every shape)

def _tn_bound(Ae, B):
    """test_gemm_tn's bound (the accumulate variant too: the one rounding of C + product is far inside it)"""
    return 16 * EPS * (Ae.abs().double().t() @ B.abs().double()) + 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['plain', 'affine', 'gather', 'colsum1', 'colsum4', 'accumulate'])
@pytest.mark.parametrize('R,Ka,No', [(7, 32, 96), (1030, 624, 208), (2049, 208, 624), (1500, 64, 104), (2080, 612, 208)])
def test_pitched_tn_product(R, Ka, No, variant):
    """qagnn_gemm_tn_colsum_f32 with lda > Ka, ldb > No, ldc > No: the split kernel where it takes the shape, the strip / runtime-shape
    fp32 kernels otherwise (and always with the column sums), k_sum_chunks4 into the guarded C."""
    g = torch.Generator().manual_seed(R + Ka)
    V = R // 2 + 3 if variant == 'gather' else R
    A, B = torch.randn(V, Ka, generator=g), torch.randn(R, No, generator=g)
    vec, idx, out0, groups, ridx = {}, None, None, 0, None
    if variant == 'affine':
        vec = dict(a_scale=torch.randn(Ka, generator=g), a_shift=torch.randn(Ka, generator=g))
    if variant == 'gather':
        idx = torch.randint(0, V, (R,), generator=g)
        idx[::17] = -1
    if variant == 'accumulate':
        out0 = torch.randn(Ka, No, generator=g)
    if variant.startswith('colsum'):
        groups = int(variant[-1])
        ridx = torch.randint(0, 4, (R,), generator=g) if groups == 4 else None
    Ae = EMU._gather_rows(A, idx)
    Ae = torch.relu(Ae * vec['a_scale'] + vec['a_shift']) if vec else Ae
    ref = Ae.double().t() @ B.double() + (out0.double() if out0 is not None else 0.0)
    bound = _tn_bound(Ae, B)
    K = hip()
    cu = lambda t: None if t is None else t.cuda()  # noqa: E731

    def call(P):
        res = K.gemm_tn(P.inp(A, 8, 4), P.inp(B, 16, 8), out=P.out('C', Ka, No, 12, 4, out0), accumulate=out0 is not None, a_rowidx=cu(idx),
                        colsum_groups=groups, b_rowidx=cu(ridx), **{k: cu(v) for k, v in vec.items()})
        return res if groups else (res,)
    got, want, P = both(call)
    log = []
    try:
        check_three('C', got[0], want[0], ref, bound, P, log)
        if groups:
            check_three('bsum', got[1], want[1], EMU.colsum(B.double(), ridx, groups), 8 * EPS * B.abs().sum(0).max().item() + 1e-6, None, log)
    finally:
        figure(f'tn[{R}-{Ka}-{No}-{variant}]', log)


@pytest.mark.gpu
@pytest.mark.parametrize('R,Ka1,Ka2,No', [(700, 32, 16, 96), (2000, 208, 112, 624), (1500, 100, 112, 208), (51200, 208, 112, 624)])
def test_pitched_tn_two_operands(R, Ka1, Ka2, No):
    """qagnn_gemm_tn2_f32 with lda1 != lda2: two fp32 products, the merged split launch, and (Ka1 = 100: one half declined) two again.
    51 200 rows: k_gemm_tn_ws runs from chunks of 28 k-tiles on, i.e. from about 50 000 rows of this product (tn_route) -- the second
    large case of this file, here because no smaller shape reaches that kernel."""
    g = torch.Generator().manual_seed(R + Ka1 + Ka2)
    A1, A2, B = torch.randn(R, Ka1, generator=g), torch.randn(R, Ka2, generator=g), torch.randn(R, No, generator=g)
    A = torch.cat([A1, A2], 1)
    ref = A.double().t() @ B.double()
    K = hip()

    def call(P):
        return (K.gemm_tn2(P.inp(A1, 8, 4), P.inp(A2, 16, 8), P.inp(B, 12, 4), out=P.out('C', Ka1 + Ka2, No, 16, 8)),)
    (got,), (want,), P = both(call)
    log = []
    try:
        check_three('C', got, want, ref, _tn_bound(A, B), P, log)
    finally:
        figure(f'tn2[{R}-{Ka1}-{Ka2}-{No}]', log)


@pytest.mark.gpu
@pytest.mark.parametrize('R,Ka1,Ka2,No', [(2000, 208, 112, 624), (5000, 112, 0, 624)])
def test_pitched_tn_three_mfma_form(R, Ka1, Ka2, No):
    """qagnn_gemm_tn_h2_f32 (operand maxima from the logical operands) under test_gemm_tn_three_mfma_form's bound"""
    g = torch.Generator().manual_seed(R + Ka1 + Ka2 + No)
    A1, B = torch.randn(R, Ka1, generator=g), torch.randn(R, No, generator=g)
    A2 = torch.randn(R, Ka2, generator=g) if Ka2 else None
    A = A1 if not Ka2 else torch.cat([A1, A2], 1)
    ref = A.double().t() @ B.double()
    arow = torch.cat([torch.full((Ka1,), A1.abs().max().item()), torch.full((Ka2,), A2.abs().max().item() if Ka2 else 0.0)]).double()
    bound = 16 * EPS * (A.abs().double().t() @ B.abs().double()) + 2.0 ** -38 * R * arow[:, None] * B.abs().max().item() + 1e-30
    K = hip()
    w1, wb, w2 = K.absmax(A1.cuda()), K.absmax(B.cuda()), (K.absmax(A2.cuda()) if Ka2 else None)

    def call(P):
        return (K.gemm_tn_h2(P.inp(A1, 8, 4), P.inp(B, 12, 4), w1, wb, A2=P.inp(A2, 16, 8), amax_a2=w2, out=P.out('C', Ka1 + Ka2, No, 16, 8)),)
    (got,), (want,), P = both(call)
    log = []
    try:
        check_three('C', got, want, ref, bound, P, log)
    finally:
        figure(f'tn_h2[{R}-{Ka1}-{Ka2}-{No}]', log)


# ---- column reductions and BatchNorm backward ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('R,C', [(257, 624), (5, 32), (1000, 208)])
def test_pitched_column_reductions_and_bn_backward(R, C):
    """qagnn_colreduce_f32 modes 0, 1, 2 (ldx != ldx2), grouped and row-weighted, and qagnn_bn_relu_bwd{,_colsum}_f32 with one shared
    ld > Cc and a guarded dH; tolerances of test_column_reductions_and_bn_backward; every column sum bit-identical to the contiguous call's."""
    g = torch.Generator().manual_seed(R * 7 + C)
    X, H = torch.randn(R, C, generator=g), torch.randn(R, C, generator=g) * 2 + 0.3
    idx = torch.randint(0, 4, (R,), generator=g)
    w = torch.rand(R, generator=g) + 0.1
    w = w / w.sum()
    mean = H.mean(0)
    var = EMU.colvar_sum(H.double(), mean.double()).float() / R
    invstd = torch.rsqrt(var + 1e-5)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    scale, shift = gamma * invstd, beta - mean * gamma * invstd
    K = hip()
    log = []
    try:
        for label, rowidx, groups, roww in (('colsum', None, 1, None), ('colsum4', idx, 4, None), ('colsum_w', None, 1, w)):
            call = lambda P: (K.colsum(P.inp(X, 8, 4), None if rowidx is None else rowidx.cuda(), groups, roww=None if roww is None else roww.cuda()),)  # noqa: E731
            (got,), (want,), _ = both(call)
            ref = EMU.colsum(X.double(), rowidx, groups, roww=None if roww is None else roww.double())
            check_three(label, got, want, ref, 4 * EPS * X.abs().sum(0).max().item() + 1e-6, None, log)
        for label, roww in (('colvar', None), ('colvar_w', w)):
            call = lambda P: (K.colvar_sum(P.inp(H, 16, 8), mean.cuda(), roww=None if roww is None else roww.cuda()),)  # noqa: E731
            (got,), (want,), _ = both(call)
            ref = EMU.colvar_sum(H.double(), mean.double(), roww=None if roww is None else roww.double())
            check_three(label, got, want, ref, 8 * EPS * ref + 1e-6, None, log)
        stats = [t.cuda() for t in (mean, invstd, scale, shift)]
        (got,), (want,), _ = both(lambda P: (K.bn_bwd_reduce(P.inp(X, 8, 4), P.inp(H, 16, 8), *stats),))
        ref = EMU.bn_bwd_reduce(*[t.double() for t in (X, H, mean, invstd, scale, shift)])
        # (mask flips at |y| ~ 1e-7 are legal: the bound has the size of a few elements)
        check_three('bn_bwd_reduce', got, want, ref, 8 * EPS * (X.abs() * (1 + ((H - mean) * invstd).abs())).sum(0).max().item() + 3 * X.abs().max().item() * 4, None, log)
        red = ref.float().contiguous()
        for label, inv_rows, roww in (('bn_relu_bwd', 1.0 / R, None), ('bn_relu_bwd_eval', 0.0, None), ('bn_relu_bwd_w', 0.0, w)):
            for colsum in (False, True):
                def call(P):
                    fn = K.bn_relu_bwd_colsum if colsum else K.bn_relu_bwd
                    res = fn(P.inp(X, 12, 4), P.inp(H, 12, 8), *stats, gamma.cuda(), red.cuda(), inv_rows, None if roww is None else roww.cuda(),
                             dH=P.out('dH', R, C, 12, 0))
                    return res if colsum else (res,)
                got, want, P = both(call)
                ref2 = EMU.bn_relu_bwd(*[t.double() for t in (X, H, mean, invstd, scale, shift, gamma, red)], inv_rows, roww=None if roww is None else roww.double())
                err = (got[0].cpu().double() - ref2).abs()
                flips = (err > 1e-4 * (1 + ref2.abs())).sum().item()
                log.append(f'{label}{"+colsum" if colsum else ""} {flips} elements beyond fp32 rounding (<= 2)')
                assert flips <= 2 and torch.isfinite(got[0]).all()
                assert same_bits(got[0], want[0]), f'(b) {label}: dH differs in its bits from the contiguous call'
                P.check()
                if colsum:  # (test_bn_relu_backward_with_colsum_by_product: the sums ARE a mode-0 reduction of the output)
                    assert same_bits(got[1], want[1]) and same_bits(got[1], K.colsum(got[0])[0]), f'(b) {label}: column sums'
    finally:
        figure(f'colreduce_bn[{R}-{C}]', log)


# ---- edge attention ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('name,HP', [('rand_small', 28), ('class_ladder', 16), ('degree_ladder', 52), ('degree_ladder', 8)])
def test_pitched_edge_attention(name, HP):
    """qagnn_edge_attn_{fwd,bwd}_f32 with ldk = 3 DP + 16, lde = 2 DP + 8, lda = DP + 4, ldg = DP + 12; aggr, dKMQ (pitch ldk) and dEkEm
    (pitch lde) guarded.  check_edge_outputs on the views (bars of the contiguous test, head pads exactly zero), bit identity with the
    contiguous run of test_edge_attention_forward_backward."""
    case = edge_case(name, HP)
    (ei, et, nt, R, T), DP = case.graph, 4 * HP
    K = hip()
    g = K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R, T)
    P = Place(True)
    KMQ, EkEm = P.inp(case.KMQ, 16, 8), P.inp(case.EkEm, 8, 4)
    assert (KMQ.stride(0), EkEm.stride(0)) == (3 * DP + 16, 2 * DP + 8)
    aggr, a, alpha = K.edge_attn_fwd(g, KMQ, EkEm, HP, case.qs, aggr=P.out('aggr', g.N, DP, 4, 0))
    dKMQ, dEkEm = K.edge_attn_bwd(g, KMQ, EkEm, HP, case.qs, a, alpha, P.inp(case.G, 12, 4), dKMQ=P.out('dKMQ', g.N, 3 * DP, 16, 4),
                                  dEkEm=P.out('dEkEm', g.C, 2 * DP, 8, 4))
    torch.cuda.synchronize()
    got = (aggr, a, alpha, dKMQ, dEkEm)
    log = []
    try:
        check_edge_outputs(case, got, log)
        for nm, x, y in zip(EDGE_OUTPUTS, got, run_edge_kernels(case)):
            assert same_bits(x, y), f'(b) {nm} differs in its bits from the contiguous run'
        P.check()
    finally:
        print_figures(f'edge_pitched[{name}-{HP}]', log)


# ---- pooling and head --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('B,n,NH,Cc,p', [(3, 37, 4, 32, 0.0), (5, 200, 2, 208, 0.3)])
def test_pitched_pool_attention(B, n, NH, Cc, p):
    """qagnn_pool_attn_{fwd,bwd}_f32 with ldk = Cc + 8 and lddk = Cc + 16, dK guarded; tolerances of test_pool_attention_forward_backward"""
    g = torch.Generator().manual_seed(B * 100 + n)
    u, c = torch.randn(B, NH, Cc, generator=g) * 0.3, torch.randn(B, NH, generator=g)
    Kx = torch.randn(B, n, Cc, generator=g)
    lens = torch.randint(1, n + 1, (B,), generator=g)
    mask = torch.arange(n).unsqueeze(0) >= lens.unsqueeze(1)
    dz, da = torch.randn(B, NH, Cc, generator=g), torch.randn(B, NH, n, generator=g)
    K, seed, it = hip(), 12345, 0.2
    r_attn, r_attn_d, r_z = EMU.pool_attn_fwd(u.double(), c.double(), Kx.double(), mask, it, p, seed)
    r_bwd = EMU.pool_attn_bwd(u.double(), Kx.double(), it, p, seed, r_attn, r_attn_d, dz.double(), da.double())

    def call(P):
        Kp = P.inp3(Kx, 8, 4)
        attn, attn_d, z = K.pool_attn_fwd(u.cuda(), c.cuda(), Kp, mask.cuda(), it, p, seed)
        dK, du, dc = K.pool_attn_bwd(u.cuda(), Kp, it, p, seed, attn, attn_d, dz.cuda(), da.cuda(), dK=P.out3('dK', B, n, Cc, 16, 8))
        return attn, attn_d, z, dK, du, dc
    got, want, P = both(call)
    assert not P.on or got[3].stride(1) == Cc + 16
    log = []
    try:
        for nm, x, y, ref, rtol, atol in zip(('attn', 'attn_d', 'z'), got, want, (r_attn, r_attn_d, r_z), (1e-4, 1e-4, 1e-4), (1e-6, 1e-6, 1e-5)):
            check_three(nm, x, y, ref, atol + rtol * ref.abs(), None, log)
        assert ((got[1].cpu() == 0) == (r_attn_d == 0)).all(), 'dropout masks differ'
        for nm, x, y, ref in zip(('dK', 'du', 'dc'), got[3:], want[3:], r_bwd):
            check_three(nm, x, y, ref, 2e-5 * max(1.0, ref.abs().max().item()) + 2e-4 * ref.abs(), None, log)
        P.check()
    finally:
        figure(f'pool_pitched[{B}-{n}-{NH}-{Cc}-{p}]', log)


@pytest.mark.gpu
def test_pitched_head():
    """qagnn_head_post_{fwd,bwd}_f32 reading row 0 of every subgraph of a pitched K3 (ldh = n * pitch); part with ldp = the minimum + 64:
    the extra columns exactly zero, the row behind the last intact; qagnn_add_row0_f32 on a pitched dK (ld_sub = n * pitch): rows 1
    onward and every margin untouched.  Tolerances of test_head_post_forward_backward."""
    B, n, NH, DP, dv, Ds, d, p1, p2 = 3, 37, 4, 32, 8, 20, 32, 0.3, 0.0
    g = torch.Generator().manual_seed(B * 100 + n + NH)
    NO, L = NH * dv, NH * dv + Ds + d
    z, attn = torch.randn(B, NH, DP, generator=g), torch.rand(B, NH, n, generator=g) / n
    BDv, bv = torch.randn(NH * DP, NO, generator=g) * 0.1, torch.randn(NO, generator=g)
    for h in range(NH):
        BDv[h * DP:(h + 1) * DP, :h * dv] = 0
        BDv[h * DP:(h + 1) * DP, (h + 1) * dv:] = 0
    sent, K3 = torch.randn(B, Ds, generator=g), torch.randn(B, n, DP, generator=g)
    w, bfc, dl = torch.randn(L, generator=g) * 0.1, torch.randn(1, generator=g), torch.randn(B, generator=g)
    dK0 = torch.randn(B, n, DP, generator=g)
    K, s1, s2 = hip(), 4711, 815
    cu, dd = (lambda t: t.cuda()), (lambda t: t.double())  # noqa: E731
    ldp = (L + NO + 1 + 3) // 4 * 4 + 64
    r_fwd = EMU.head_post_fwd(dd(z), dd(attn), dd(BDv), dd(bv), dd(sent), dd(K3), d, dd(w), dd(bfc), p1, p2, s1, s2)
    r_bwd = EMU.head_post_bwd(dd(dl), r_fwd[1], r_fwd[2], dd(BDv), dd(bv), dd(sent), dd(K3), d, dd(w), p1, p2, s1, s2, n, True)

    def call(P):
        K3p = P.inp3(K3, 8, 4)
        logits, out, asum = K.head_post_fwd(cu(z), cu(attn), cu(BDv), cu(bv), cu(sent), K3p, d, cu(w), cu(bfc), p1, p2, s1, s2)
        part = P.out('part', B, ldp, 0, 0)  # (every column is the kernel's: the guard is the row behind the last)
        bwd = K.head_post_bwd(cu(dl), out, asum, cu(BDv), cu(bv), cu(sent), K3p, d, cu(w), p1, p2, s1, s2, n, True, part=part)
        dK = K.add_row0(P.out3('dK', B, n, DP, 16, 8, init=dK0), bwd[4])
        return (logits, out, asum) + tuple(bwd) + (dK,)
    got, want, P = both(call)
    assert got[8] is not None and got[8].shape == (B, ldp) and (not P.on or got[9].stride(1) == DP + 16)
    log = []
    try:
        for nm, x, y, ref, atol in zip(('logits', 'out', 'asum'), got, want, r_fwd, (2e-4, 2e-5, 2e-5)):
            check_three(nm, x, y, ref, atol + 2e-4 * ref.abs(), None, log)
        for nm, x, y, ref in zip(('dz', 'dattn', 'dout', 'dsent', 'dZ'), got[3:8], want[3:8], r_bwd):
            check_three(nm, x, y, ref, 2e-5 * max(1.0, ref.abs().max().item()) + 2e-4 * ref.abs(), None, log)
        rp = torch.zeros(B, ldp, dtype=torch.float64)
        rp[:, :r_bwd[5].size(1)] = r_bwd[5]
        check_three('part', got[8], want[8], rp, 2e-5 * max(1.0, rp.abs().max().item()) + 2e-4 * rp.abs(), None, log)
        assert (got[8].cpu()[:, L + NO + 1:] == 0).all(), 'the columns of part past L + NH dv + 1 are not exactly zero'
        wantK = dK0.clone()
        wantK[:, 0] += r_bwd[4].float()
        dK = got[9].cpu()
        assert torch.allclose(dK, wantK, rtol=1e-5, atol=1e-6) and same_bits(dK[:, 1:], dK0[:, 1:]) and same_bits(dK, want[9])
        P.check()
    finally:
        figure('head_pitched[3-37-4-32-8-20-32-0.3-0.0]', log)


# ---- rejections (host side: QAGNN_EINVAL before any launch) ---------------------------------------------------------------------------------------

def _reject_cases():
    """name -> (operands by name, the names whose pitch the library is told 4 floats short, the call).  Every operand is allocated
    contiguous at its full size: were a check missing, the kernels would read and write inside the allocations all the same."""
    r = lambda *s: torch.randn(*s).cuda()  # noqa: E731
    M, K1, K2, No = 64, 32, 16, 48
    nn = dict(A1=r(M, K1), B1=r(K1, No), A2=r(M, K2), B2=r(K2, No), C=r(M, No), tab=r(4, No), B1n=r(No, K1), B2n=r(No, K2))
    ridx = torch.randint(0, 4, (M,)).cuda()
    fp32 = lambda K, o: K.gemm_nn(o['A1'], o['B1'], o['A2'], o['B2'], rowtab=o['tab'], rowidx=ridx, out=o['C'])  # noqa: E731
    split = lambda K, o: K.gemm_nn(o['A1'], o['B1'], o['A2'], o['B2'], rowtab=o['tab'], rowidx=ridx, out=o['C'], B1n=o['B1n'], B2n=o['B2n'])  # noqa: E731
    cases = {f'nn_fp32-{k}': (nn, [k], fp32) for k in ('A1', 'A2', 'B1', 'B2', 'C', 'tab')}
    cases.update({f'nn_split-{k}': (nn, [k], split) for k in ('A1', 'A2', 'C', 'tab', 'B1n', 'B2n')})
    R, Ka, Ka2 = 96, 32, 16
    tn = dict(A=r(R, Ka), A2=r(R, Ka2), B=r(R, No), C=r(Ka, No), C2=r(Ka + Ka2, No))
    cases.update({f'tn-{k}': (tn, [k], lambda K, o: K.gemm_tn(o['A'], o['B'], out=o['C'])) for k in ('A', 'B', 'C')})
    cases.update({f'tn2-{k}': (tn, [k], lambda K, o: K.gemm_tn2(o['A'], o['A2'], o['B'], out=o['C2'])) for k in ('A', 'A2', 'B', 'C2')})
    Cc = 32
    cr = dict(X=r(R, Cc), H=r(R, Cc), dH=r(R, Cc), v=r(Cc), red=r(2, Cc))
    cases['colreduce-X'] = (cr, ['X'], lambda K, o: K.colsum(o['X']))
    cases['colreduce-X-mode1'] = (cr, ['X'], lambda K, o: K.colvar_sum(o['X'], o['v']))
    cases['colreduce-X2'] = (cr, ['H'], lambda K, o: K.bn_bwd_reduce(o['X'], o['H'], o['v'], o['v'], o['v'], o['v']))
    bn = lambda fn: (lambda K, o: getattr(K, fn)(o['X'], o['H'], o['v'], o['v'], o['v'], o['v'], o['v'], o['red'], 0.1, dH=o['dH']))  # noqa: E731
    cases['bn_relu_bwd-ld'] = (cr, ['X', 'H', 'dH'], bn('bn_relu_bwd'))
    cases['bn_relu_bwd_colsum-ld'] = (cr, ['X', 'H', 'dH'], bn('bn_relu_bwd_colsum'))
    B, NH, DP, dv, Ds, d = 3, 4, 32, 8, 20, 32  # (n = 1: the distance between the subgraphs' rows 0 is the row pitch itself)
    NO = NH * dv
    hd = dict(z=r(B, NH, DP), attn=r(B, NH, 1), BDv=r(NH * DP, NO), bv=r(NO), sent=r(B, Ds), K3=r(B, 1, DP), w=r(NO + Ds + d), bfc=r(1), dl=r(B),
              out=r(B, NO), asum=r(B, NH), dK=r(B, 1, DP), dZ=r(B, DP))
    cases['head_fwd-ldh'] = (hd, ['K3'], lambda K, o: K.head_post_fwd(o['z'], o['attn'], o['BDv'], o['bv'], o['sent'], o['K3'], d, o['w'], o['bfc'],
                                                                       0.3, 0.0, 4711, 815))
    cases['head_bwd-ldh'] = (hd, ['K3'], lambda K, o: K.head_post_bwd(o['dl'], o['out'], o['asum'], o['BDv'], o['bv'], o['sent'], o['K3'], d, o['w'],
                                                                       0.3, 0.0, 4711, 815, 1, True))
    cases['add_row0-ld_sub'] = (hd, ['dK'], lambda K, o: K.add_row0(o['dK'], o['dZ']))
    return cases


REJECTS = ['nn_fp32-A1', 'nn_fp32-A2', 'nn_fp32-B1', 'nn_fp32-B2', 'nn_fp32-C', 'nn_fp32-tab', 'nn_split-A1', 'nn_split-A2', 'nn_split-C',
           'nn_split-tab', 'nn_split-B1n', 'nn_split-B2n', 'tn-A', 'tn-B', 'tn-C', 'tn2-A', 'tn2-A2', 'tn2-B', 'tn2-C2', 'colreduce-X',
           'colreduce-X-mode1', 'colreduce-X2', 'bn_relu_bwd-ld', 'bn_relu_bwd_colsum-ld', 'head_fwd-ldh', 'head_bwd-ldh', 'add_row0-ld_sub']


@pytest.mark.gpu
@pytest.mark.parametrize('name', REJECTS)
def test_pitched_rejections(name, monkeypatch):
    """Every lower bound a pitch has (>= the width it strides) is checked on the host: with ONE pitch handed over 4 floats short -- through
    the binding, on operands allocated at full size -- the call returns QAGNN_EINVAL before anything is launched, and the same call with
    the true pitches goes through."""
    from qagnn_amd import _lib
    torch.manual_seed(1)
    cases = _reject_cases()
    assert sorted(cases) == sorted(REJECTS)
    operands, short, call = cases[name]
    K = hip()
    call(K, operands)  # the true pitches: accepted
    torch.cuda.synchronize()
    before = {k: v.clone() for k, v in operands.items()}
    for fn in ('_ld', '_ld3'):  # (_ld3: the row pitch of the [B, n, Cc] operands of the head)
        monkeypatch.setattr(_lib, fn, lambda t, true_ld=getattr(_lib, fn): true_ld(t) - (4 if any(t is operands[k] for k in short) else 0))
    with pytest.raises(RuntimeError, match=r'\(code 1\)'):
        call(K, operands)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert all(same_bits(before[k], v) for k, v in operands.items()), 'a rejected call wrote to an operand'
