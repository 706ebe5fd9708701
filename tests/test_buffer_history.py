"""Every entry point on fresh buffers whose prior contents it must ignore (the contract the headers state in words).

The binding (qagnn_amd/_lib.py) allocates its outputs, saved buffers and workspaces with torch.empty; include/qagnn_hip.h calls a
workspace's contents "undefined before and after", defines an output without `accumulate` by the call alone, lets the hop zero its own
maximum words, and names the few words the caller zeroes (the absmax slot, the *_amax by-products, the err flags).  On a zeroed buffer
a product that adds into its output, a skipped tile or padding row, a partial slot that is summed but not written, a counter that is
not reset or a maximum word that only grows all give the right answer, and on the finite leftovers of the caching allocator a nearly
right one.  Here every call runs on buffers that arrive filled -- helpers.fresh_buffers: 0x00, 0xFF (NaN) and 0x7B (1.3e36) bytes --
and helpers.check_history_free holds what it returns to the same BITS under all three.

  1. `-m "not gpu"`  the fill policy fills every dtype the package allocates and restores torch; the inventory of allocation forms
     (an ast walk over qagnn_amd/*.py) and of allocating binding methods (against the case table below) is closed; the comparison
     accepts the operator layer on the emulation and rejects three stand-ins that are right on zeros.
  2. `-m gpu`  the case table: one entry per route of every HipKernels method that allocates, at the smallest shape that reaches it.
  3. `-m gpu`  the words the caller owns: the documented merge of the maximum slots, and the four hop / stack entry points through the
     raw struct over NaN canaries with 0x7F000000 in the maximum words.
  4. `-m gpu`  the module end to end: one eager training step, one eval forward on the inference path, one explain.trace.

An exemption (helpers.Exempt) is a region the header declares unwritten: it must still hold the fill, bit for bit, under every fill;
the header's sentence stands next to it; the call that consumes the tensor runs on the poisoned tensor in the same case.
QAGNN_HISTORY_TEST_LOG names a file that collects the FIGURE lines (profiles/buffer_history_gpu_tests.txt).
"""
import ast
import contextlib
import ctypes as C
import functools
import inspect
import os
import re
import time
from unittest import mock

import pytest
import torch

import helpers
from helpers import Exempt, check_history_free, fresh_buffers
from qagnn_amd import _lib, ops

LOG_FILE = os.environ.get('QAGNN_HISTORY_TEST_LOG')
PKG = os.path.join(helpers.ROOT, 'qagnn_amd')


def note(line):
    print(line)
    if LOG_FILE:
        with open(LOG_FILE, 'a') as f:
            f.write(line + '\n')


class _Log(list):
    def append(self, line):
        super().append(line)
        if LOG_FILE:
            with open(LOG_FILE, 'a') as f:
                f.write(line + '\n')


LOG = _Log()


def hip():
    ops.set_kernels(None)
    return ops.kernels()


def reset_seeds():
    """what a run's dropout masks depend on: torch's generators, the package's call counter, the library's seed epoch (ops.manual_seed)"""
    ops.manual_seed(5)


# =================================================================================================================================
# 1. Without a GPU: the fill policy
# =================================================================================================================================
PACKAGE_DTYPES = {torch.float32, torch.int32, torch.int64, torch.uint8, torch.bool}
FORBIDDEN = ('empty_strided', 'new_empty_strided', 'empty_permuted', 'empty_quantized', 'resize_', 'resize_as_', 'set_')
LEGACY_CTORS = ('Tensor', 'FloatTensor', 'DoubleTensor', 'HalfTensor', 'BFloat16Tensor', 'LongTensor', 'IntTensor', 'ShortTensor', 'ByteTensor',
                'CharTensor', 'BoolTensor')
HOST_ARRAY_MODULES = ('np', 'numpy')  # np.empty: host index scratch of data_utils, filled by the host code that follows it -- no device buffer


def _package_sources():
    for f in sorted(os.listdir(PKG)):
        if f.endswith('.py'):
            with open(os.path.join(PKG, f)) as fh:
                yield f, ast.parse(fh.read(), f)


def allocation_inventory(sources=None):
    """-> (allowed, refused, dtypes): every uninitialised allocation of the package as (file, line, form); `refused` the ones the fill policy
    would miss; the constant dtypes named at the allowed ones"""
    allowed, refused, dtypes = [], [], set()
    alias = {'float': torch.float32, 'long': torch.int64, 'int': torch.int32, 'double': torch.float64, 'half': torch.float16}
    for fname, tree in (sources or _package_sources()):
        calls = {id(n.func): n for n in ast.walk(tree) if isinstance(n, ast.Call)}
        for n in ast.walk(tree):
            if isinstance(n, ast.ImportFrom) and n.module and n.module.split('.')[0] == 'torch':
                for a in n.names:
                    if a.name in helpers.UNINITIALISED + FORBIDDEN + LEGACY_CTORS or a.name == '*':
                        refused.append((fname, n.lineno, f'from {n.module} import {a.name}'))
            if not isinstance(n, ast.Attribute):
                continue
            recv = n.value.id if isinstance(n.value, ast.Name) else None
            where = (fname, n.lineno, f'{recv or "<expr>"}.{n.attr}')
            if n.attr in FORBIDDEN or (n.attr in LEGACY_CTORS and recv == 'torch' and id(n) in calls):
                refused.append(where)
            elif n.attr in ('empty', 'empty_like'):
                if recv in HOST_ARRAY_MODULES:
                    continue
                (allowed if recv == 'torch' and id(n) in calls else refused).append(where)  # (an alias `e = torch.empty` escapes the scope)
            elif n.attr == 'new_empty':
                (allowed if id(n) in calls else refused).append(where)
            else:
                continue
            call = calls.get(id(n))
            for kw in (call.keywords if call is not None else ()):
                v = kw.value
                if kw.arg == 'dtype' and isinstance(v, ast.Attribute) and isinstance(v.value, ast.Name) and v.value.id == 'torch':
                    dtypes.add(alias.get(v.attr, getattr(torch, v.attr)))
    return allowed, refused, dtypes


def test_the_allocation_inventory_is_closed():
    """`-m "not gpu"`.  Every uninitialised allocation of qagnn_amd/*.py is torch.empty, torch.empty_like (through the module's `torch`
    global) or Tensor.new_empty -- the three forms fresh_buffers fills.  empty_strided, resize_, torch.Tensor(...), an alias of torch.empty
    or `from torch import empty` would escape the policy: each is refused here and named.  The dtypes named at the allocations are the
    five the fill test covers."""
    allowed, refused, dtypes = allocation_inventory()
    assert not refused, 'allocations the fill policy of tests/helpers.py would miss: ' + ', '.join(f'{f}:{ln} {form}' for f, ln, form in refused)
    per_file = {}
    for f, _, _ in allowed:
        per_file[f] = per_file.get(f, 0) + 1
    note(f'FIGURE history inventory: {len(allowed)} uninitialised allocations in {len(per_file)} files ({per_file}), dtypes {sorted(map(str, dtypes))}')
    assert per_file.get('_lib.py', 0) >= 80 and len(per_file) >= 7
    assert dtypes == PACKAGE_DTYPES, f'the package allocates {sorted(map(str, dtypes))}: extend the fill test to them'
    # every module that allocates reaches torch through a module global named `torch`, the name fresh_buffers replaces
    mods = helpers.package_modules()
    for f in per_file:
        assert mods[f[:-3]].__dict__.get('torch') is torch, f'{f}: no module global `torch`'


@pytest.mark.parametrize('bad', ['x = torch.empty_strided((2, 2), (2, 1))', 'x.resize_(4)', 'x = torch.Tensor(3)', 'from torch import empty',
                                 'e = torch.empty', 'import torch as th\nx = th.empty(3)', 'y = x.new_empty_strided((2,), (1,))'])
def test_the_inventory_names_an_allocation_the_policy_would_miss(bad):
    """`-m "not gpu"`: the walk refuses each form on a one-line module"""
    _, refused, _ = allocation_inventory([('later.py', ast.parse('import torch\n' + bad))])
    assert len(refused) == 1 and refused[0][0] == 'later.py', refused


def _package_allocations(dev='cpu'):
    """one allocation of every dtype and form, made by PACKAGE code: functions compiled with the globals of qagnn_amd._lib"""
    src = ('def _alloc(dtype, dev):\n    return torch.empty((3, 5), dtype=dtype, device=dev)\n'
           'def _like(t):\n    return torch.empty_like(t)\n'
           'def _new(t, shape):\n    return t.new_empty(shape)\n')
    ns = {}
    exec(compile(src, os.path.join(PKG, '_lib.py'), 'exec'), _lib.__dict__, ns)
    return ns


def test_fresh_buffers_fills_every_dtype_and_restores_on_exit_and_on_an_exception():
    """`-m "not gpu"`.  Byte patterns for float and uint8 buffers (0x00 | 0xFF, a NaN | 0x7B, 1.3e36 in fp32 and 61 280 in fp16), 0 | 1 | 1 for
    integer and bool buffers; all three forms; torch's own allocations and a test's are untouched; everything is back on exit."""
    fn = _package_allocations()
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty, 'new_empty' in torch.Tensor.__dict__)
    want32 = {'zero': 0, 'nan': -1, 'big': 0x7B7B7B7B}
    assert [helpers.fill_word(f) for f in helpers.FILLS] == list(want32.values())
    for fill in helpers.FILLS:
        with fresh_buffers(fill):
            assert _lib.torch is not torch and ops.torch is not torch
            for dt in sorted(PACKAGE_DTYPES | {torch.float16, torch.bfloat16, torch.float64}, key=str):
                for t in (fn['_alloc'](dt, 'cpu'), fn['_like'](torch.zeros(4, 2, dtype=dt)), fn['_new'](torch.zeros(1, dtype=dt), (2, 3))):
                    if dt.is_floating_point or dt == torch.uint8:
                        assert bool((t.contiguous().view(torch.uint8) == helpers.FILL_BYTES[fill]).all()), (fill, dt)
                    else:
                        assert bool((t == (fill != 'zero')).all()) and t.dtype == dt, (fill, dt)
            f32, f16 = fn['_alloc'](torch.float32, 'cpu'), fn['_alloc'](torch.float16, 'cpu')
            assert bool((f32.view(torch.int32) == want32[fill]).all())
            if fill == 'nan':
                assert bool(torch.isnan(f32).all()) and bool(torch.isnan(f16).all()) and bool(torch.isnan(fn['_alloc'](torch.bfloat16, 'cpu')).all())
            if fill == 'big':
                assert 1.2e36 < f32[0, 0].item() < 1.4e36 and f16[0, 0].item() == 61280.0
            leaf = _lib.torch.empty(3, requires_grad=True)  # (graphed.py allocates one leaf that requires grad)
            assert leaf.requires_grad and leaf.is_leaf and bool((leaf.detach().view(torch.int32) == want32[fill]).all())
            # not the package's: torch's own entry points, a tensor method called from a test module, autograd's buffers
            g = torch.Generator().manual_seed(1)
            assert torch.equal(torch.randn(5, generator=g), torch.randn(5, generator=torch.Generator().manual_seed(1)))
            assert torch.empty is before[0] and torch.empty_like is before[1]
            x = torch.ones(3, requires_grad=True)
            (x * x).sum().backward()
            assert torch.equal(x.grad, torch.full((3,), 2.0))
            mine = torch.zeros(2).new_empty(64)  # (called from this module: whatever the allocator hands back, not the fill)
            assert mine.shape == (64,)
        assert (torch.empty, torch.empty_like, torch.Tensor.new_empty, 'new_empty' in torch.Tensor.__dict__) == before
        assert all(m.__dict__.get('torch', torch) is torch for m in helpers.package_modules().values())
    with pytest.raises(ZeroDivisionError):
        with fresh_buffers('nan'):
            1 / 0
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty, 'new_empty' in torch.Tensor.__dict__) == before
    assert all(m.__dict__.get('torch', torch) is torch for m in helpers.package_modules().values())
    with pytest.raises(AssertionError):
        with fresh_buffers('ones'):
            pass


# ---- the comparison, on the emulation ---------------------------------------------------------------------------------------------------
def _emu_hops():
    """two chained hops of the operator layer (ops.hop_fwd_composed / hop_bwd_composed) on the emulation, train mode with dropout, fp32 on
    the CPU -> every forward buffer and every gradient"""
    import test_nonfinite as TN
    case = TN.hop_case('small_train', k=2)
    ei, et, nt, R, T = case['graph']
    conv = lambda t: t.clone()  # noqa: E731
    prms = [TN._prm(p, conv) for p in case['prms']]
    dy = torch.randn(case['N'], case['DP'], generator=torch.Generator().manual_seed(3))

    def call():
        g = TN.EMU.graph_prep(ei, et, nt, R, T)
        x, outs, saved = case['X'], [], []
        for l in range(2):
            args = (g, case['HP'], case['qs'], x, case['S'], nt, prms[l], True, 1e-5, 0.2, 4321 + l)
            y, sv = ops.hop_fwd_composed(TN.EMU, *args, True, None)
            saved.append((args, sv))
            outs += [y, *sv]
            x = y
        d = dy
        for args, sv in reversed(saved):
            r = ops.hop_bwd_composed(TN.EMU, *args, True, sv, d, True, True)
            outs += [t for t in r if t is not None]
            d = r[0]
        return outs
    return call


def _adds_into_its_output(orig):
    """a product that ADDS into the output it allocated: right on zeros"""
    def gemm_nn(self, A1, B1, *a, out=None, accumulate=False, colstats=False, **kw):
        if out is not None or colstats:
            return orig(self, A1, B1, *a, out=out, accumulate=accumulate, colstats=colstats, **kw)
        Cm = orig(self, A1, B1, *a, **kw)
        fresh = ops.torch.empty(Cm.shape, dtype=Cm.dtype)
        fresh += Cm
        return fresh
    return gemm_nn


def _sums_an_unwritten_partial(orig):
    """a reduction over row chunks whose workspace has one slot more than it writes, and that sums every slot: right on zeros"""
    def colsum(self, X, rowidx=None, groups=1, scale=1.0, roww=None, out=None):
        if rowidx is not None or roww is not None or out is not None:
            return orig(self, X, rowidx, groups, scale, roww, out)
        chunks = X.split(32)
        ws = ops.torch.empty((len(chunks) + 1, X.size(1)), dtype=X.dtype)
        for i, c in enumerate(chunks):
            ws[i] = c.sum(0)
        return ws.sum(0, keepdim=True) * scale
    return colsum


def _skips_the_last_row(orig):
    """an elementwise pass that leaves the last row of its output unwritten: deterministic on zeros"""
    def gelu_dropout_fwd(self, X, p, seed):
        Y = ops.torch.empty_like(X)
        Y[:-1] = orig(self, X, p, seed)[:-1]
        return Y
    return gelu_dropout_fwd


STAND_INS = {'adds': ('gemm_nn', _adds_into_its_output), 'unwritten_partial': ('colsum', _sums_an_unwritten_partial),
             'last_row': ('gelu_dropout_fwd', _skips_the_last_row)}


def test_the_comparison_accepts_the_operator_layer_on_the_emulation():
    """`-m "not gpu"`: two hops forward and backward through ops.hop_*_composed on tests/emu_kernels.py, as they are"""
    n, ex = check_history_free(_emu_hops(), reset=reset_seeds, what='emulation, operator layer')
    assert n > 10000 and ex == 0


def test_the_comparison_accepts_the_module_on_the_emulation(monkeypatch):
    """`-m "not gpu"`: a train-mode forward and backward of the module with the run scripts' dropout on the emulation, whose deferred weight
    gradients are allocated ahead of their launches (ops._wgrad: Tensor.new_empty) -- logits and every gradient; the allocations of that
    path are counted, so that the acceptance is one of filled buffers."""
    import test_hip_parity as T
    import test_nonfinite as TN
    from emu_kernels import EmuKernels
    case = dict(TN.TINY, train=True)
    args, _ = T._case_args(case)
    made = []
    plain = helpers.policy_fill_
    monkeypatch.setattr(helpers, 'policy_fill_', lambda t, fill: made.append(t.numel()) or plain(t, fill))

    def call():
        model = T._package_model(case, 'cpu', T.RUN_SCRIPT_DROPOUT)
        ops.manual_seed(5)
        logits, _ = model(*args[:5], (args[5], args[6]))
        (logits * torch.linspace(0.5, 1.5, logits.numel()).view_as(logits)).sum().backward()
        return [logits.detach()] + [p.grad for _, p in sorted(model.named_parameters()) if p.grad is not None]
    old = ops.set_kernels(EmuKernels())
    try:
        n, _ = check_history_free(call, reset=reset_seeds, what='emulation, module')
    finally:
        ops.set_kernels(old)
    assert n > 10000 and len(made) >= 4 * 6, f'{len(made)} filled allocations in four runs: the deferred weight gradients did not come through the policy'


@pytest.mark.parametrize('name', list(STAND_INS))
def test_the_comparison_rejects_a_stand_in_that_is_right_on_zeros(name, monkeypatch):
    """`-m "not gpu"`.  Each stand-in, patched into the emulation, is accepted under 'zero' alone -- the point of the three fills -- and
    rejected under each of the other two."""
    from emu_kernels import EmuKernels
    method, make = STAND_INS[name]
    monkeypatch.setattr(EmuKernels, method, make(getattr(EmuKernels, method)))
    call = _emu_hops()
    check_history_free(call, reset=reset_seeds, fills=('zero',), what=f'stand-in {name}, zeros only')
    for fill in ('nan', 'big'):
        with pytest.raises(AssertionError, match='depend on what a fresh buffer held'):
            check_history_free(call, reset=reset_seeds, fills=('zero', fill), what=f'stand-in {name}')


def test_the_comparison_reports_a_run_that_is_not_deterministic_as_such_and_holds_exemptions_to_the_fill():
    """`-m "not gpu"`.  Two runs from zeros that differ are "not deterministic", whatever the fills would show; an exempt region must hold
    the fill (a region that is written is no exemption) and may not cover a whole tensor."""
    count = [0]

    def drifting():
        count[0] += 1
        return torch.full((4,), float(count[0]))
    with pytest.raises(AssertionError, match='not deterministic'):
        check_history_free(drifting, what='drift')

    def half_written():
        t = ops.torch.empty((4, 3))
        t[2:] = 1.0
        return t
    with pytest.raises(AssertionError, match='depend on what a fresh buffer held'):
        check_history_free(half_written, what='half')
    quote = 'rows 0 and 1 are not written'
    assert check_history_free(half_written, [Exempt(0, lambda t: t[:2], quote, 'nobody')], what='half, exempt') == (6, 6)
    with pytest.raises(AssertionError, match='not an exemption'):
        check_history_free(half_written, [Exempt(0, lambda t: t[1:3], quote, 'nobody')], what='half, wrong rows')
    with pytest.raises(AssertionError, match='cover the whole'):
        check_history_free(half_written, [Exempt(0, lambda t: t[:], quote, 'nobody')], what='half, all exempt')


# =================================================================================================================================
# 2. The case table: every binding method that allocates, per route
# =================================================================================================================================
class Case:
    def __init__(self, methods, build, form=False):
        self.methods, self.build, self.form = tuple(methods), build, form  # form: under helpers.form_everywhere (row threshold 1)


CASES = {}


def case(name, methods, form=False):
    def deco(build):
        assert name not in CASES, name
        CASES[name] = Case(methods, build, form)
        return build
    return deco


def cu(*ts):
    return [None if t is None else t.cuda() for t in ts]


STATS_QUOTE = ('[5, DP]: mean, var, invstd, scale, shift; with batch_stats == 0 rows 0 and 1 (mean, var) are not written and not read: the '
               'hop reads run_mean_p / run_var_p')  # qagnn_hop_args.stats, include/qagnn_hip.h
AMAX_QUOTE = 'a call that does not run the form neither writes nor reads them'  # qagnn_hop_args.amax, include/qagnn_hip.h
EXPORT_QUOTE ='each such row of a layer of out is written exactly once, no row behind it is touched'  # include/qagnn_hip_explain.h


# ---- NN products ------------------------------------------------------------------------------------------------------------------------
NN_SHAPES = [(208, 112, 624), (32, 16, 96), (624, 0, 208)]  # the straddling k-tile (208 % 32 = 16), one tile, one operand with column statistics
NN_ROWS = (1, 257, 2000)
NN_ROUTES = ('fp32', 'six', 'three', 'reduced', 'gathered', 'prepacked', 'colstats')


def _nn_build(route, M, K1, K2, No):
    def build(K):
        import test_hip_kernels as THK
        g = torch.Generator().manual_seed(1000 * M + K1 + No)
        rows = M + 13 if route == 'gathered' else M
        A1 = THK._ranged(g, rows, K1, 'spread').cuda()
        B1 = (torch.randn(K1, No, generator=g) * 0.1).cuda()
        B1n, A2, B2, B2n = B1.t().contiguous(), None, None, None
        if K2:
            A2, B2 = torch.randn(M, K2, generator=g).cuda(), (torch.randn(K2, No, generator=g) * 0.1).cuda()
            B2n = B2.t().contiguous()
        bias, gamma, beta = cu(torch.randn(No, generator=g), 1 + 0.1 * torch.randn(No, generator=g), torch.randn(No, generator=g))
        ridx = torch.randint(0, rows, (M,), generator=g)
        ridx[::5] = -1  # (a negative index reads a zero row)
        ridx = ridx.cuda()

        def words():
            return K.absmax(A1.view(-1)), (K.absmax(A2.view(-1)) if K2 else None)

        def with_split(mode, fn):
            old, K.gemm_split = K.gemm_split, mode
            try:
                return fn()
            finally:
                K.gemm_split = old

        def call():
            nn = functools.partial(K.gemm_nn, A1, B1, A2, B2, bias=bias)
            if route == 'fp32':
                return nn()
            if route == 'six':
                return nn(B1n=B1n, B2n=B2n)
            if route in ('three', 'reduced'):
                w1, w2 = words()
                out = with_split(3 if route == 'reduced' else 2, lambda: nn(B1n=B1n, B2n=B2n, a_amax1=w1, a_amax2=w2))
                return [out, w1] + ([w2] if K2 else [])
            if route == 'gathered':
                w1, w2 = words()
                return [nn(B1n=B1n, B2n=B2n, a_rowidx=ridx), nn(a_rowidx=ridx), nn(B1n=B1n, B2n=B2n, a_rowidx=ridx, a_amax1=w1, a_amax2=w2)]
            if route == 'colstats':
                Cm, part = K.gemm_nn(A1, B1, bias=bias, B1n=B1n, colstats=True)
                return Cm, part, K.bn_stats_finalize(part, M, gamma, beta, 1e-5)
            outs = []  # prepacked: the images of B registered ahead of the product, in both piece counts
            for pieces in (3, 2):
                keep = K.prepack([(B1n, B2n, pieces)], 7701)
                try:
                    w1, w2 = words() if pieces == 2 else (None, None)
                    outs.append(nn(B1n=B1n, B2n=B2n, a_amax1=w1, a_amax2=w2))
                finally:
                    K.prepack_clear(7701)
                    del keep
            return outs
        return call, ()
    return build


for _route in NN_ROUTES:
    for _K1, _K2, _No in NN_SHAPES:
        if _route == 'colstats' and not (_K2 == 0 and 192 < _No <= 208):
            continue
        for _M in NN_ROWS:
            _meth = {'colstats': ('gemm_nn', 'bn_stats_finalize'), 'prepacked': ('gemm_nn', 'prepack', 'absmax')}.get(_route, ('gemm_nn', 'absmax'))
            case(f'nn-{_route}-{_M}-{_K1}x{_K2}x{_No}', _meth, form=True)(_nn_build(_route, _M, _K1, _K2, _No))
for _route in ('six', 'three'):  # the default threshold: the large-product kernel with its phase groups, once
    case(f'nn-{_route}-8193-default', ('gemm_nn', 'absmax'))(_nn_build(_route, 8193, 208, 112, 624))


# ---- TN products ------------------------------------------------------------------------------------------------------------------------
TN_SHAPES = [(208, 112, 624), (208, 0, 208), (32, 16, 96), (32, 0, 32)]
TN_ROWS = (1, 60, 257, 2049)  # fallbacks below the first chunk; the split routes with a ragged last chunk


def tn_families(query):
    """(R, Ka1, Ka2, No) -> family, for the table's shapes: qagnn_gemm_tn_route_query, host-only"""
    return {(R,) + s: query(R, *s)[0] for R in TN_ROWS for s in TN_SHAPES}


def _tn_build(R, Ka1, Ka2, No):
    def build(K):
        g = torch.Generator().manual_seed(R * 31 + Ka1 + No)
        A1, B = cu(torch.randn(R + 5, Ka1, generator=g), torch.randn(R, No, generator=g))
        A2 = torch.randn(R, Ka2, generator=g).cuda() if Ka2 else None
        A = torch.cat([A1[:R], A2], 1).contiguous() if Ka2 else A1[:R]
        Ka = Ka1 + Ka2
        sc, sh = cu(1 + 0.1 * torch.randn(Ka, generator=g), 0.1 * torch.randn(Ka, generator=g))
        grp = torch.randint(0, 4, (R,), generator=g).cuda()
        ridx = torch.randint(0, R + 5, (R,), generator=g)
        ridx[::7] = -1
        ridx = ridx.cuda()

        def call():
            outs = [K.gemm_tn(A, B), K.gemm_tn(A, B, a_scale=sc, a_shift=sh), K.gemm_tn(A1, B, a_rowidx=ridx)]
            outs += list(K.gemm_tn(A, B, colsum_groups=4, b_rowidx=grp)) + list(K.gemm_tn(A, B, colsum_groups=1))
            wa1, wb = K.absmax(A1[:R].reshape(-1)), K.absmax(B.view(-1))
            wa2 = K.absmax(A2.view(-1)) if Ka2 else None
            outs += [K.gemm_tn_h2(A1[:R], B, wa1, wb, A2, wa2), wa1, wb]
            old, K.gemm_split = K.gemm_split, 3
            try:
                outs.append(K.gemm_tn_h2(A1[:R], B, wa1, wb, A2, wa2))  # (qagnn_gemm_tn_h1_f32)
            finally:
                K.gemm_split = old
            if Ka2:
                outs += [K.gemm_tn2(A1[:R], A2, B), K.gemm_tn_graph(A1[:R], A2, B), K.gemm_tn_graph(A1[:R], A2, B, pieces=2, amax=(wa1, wa2, wb)),
                         K.gemm_tn_graph(A1[:R], A2, B, pieces=1, amax=(wa1, wa2, wb))]
            return outs
        return call, ()
    return build


for _s in TN_SHAPES:
    for _R in TN_ROWS:
        case(f'tn-{_R}-{_s[0]}x{_s[1]}x{_s[2]}', ('gemm_tn', 'gemm_tn2', 'gemm_tn_h2', 'gemm_tn_graph', 'absmax'))(_tn_build(_R, *_s))


def _tn_live_build(pattern):
    def build(K):
        import test_tn_live_tiles as TLT
        R = TLT.first_ws_rows(K) + 17  # the smallest two-operand shape of tests/test_tn_live_tiles.py on the live-tile route, ragged
        fam, chunk_rows, nchunks, live_route = K.tn_route_query(R, TLT.KA1, TLT.KA2, TLT.NO)
        assert fam == TLT.WS and live_route == 1
        T = (R + 31) // 32
        lone = TLT.one_live_mask(R, T - 1) if pattern == 'one_tail' else TLT.bench_like_mask(R)
        A1, A2, B, _ = TLT.operands(R)
        ei = TLT.ring_edges(lone).cuda()
        et, nt = torch.zeros(ei.size(1), dtype=torch.long, device='cuda'), torch.zeros(R, dtype=torch.long, device='cuda')

        def call():
            g = K.graph_prep(ei, et, nt, 2, 2)  # (its tile lists, partly empty, come out of poisoned storage too)
            live = g.live_tiles()
            Bm = TLT.masked_b(B, live[0].cpu().numpy())
            outs = [TLT.run_product(K, np_, A1, A2, Bm, g) for np_ in (3, 2)]
            old = K.tn_live_tiles(0)
            try:
                outs.append(TLT.run_product(K, 3, A1, A2, Bm, g))
            finally:
                K.tn_live_tiles(old)
            return outs + [K.tn_work_table(g, 3 * nchunks, chunk_rows // 32)] + list(live)
        return call, ()
    return build


for _p in ('one_tail', 'bench_like'):
    case(f'tn-live-{_p}', ('gemm_tn_graph', 'tn_work_table', 'graph_prep', 'absmax'))(_tn_live_build(_p))


# ---- reductions and elementwise -----------------------------------------------------------------------------------------------------------
def _col_rows():
    import test_row_counts as TRC
    c = TRC.CONST
    sb, sw, bb = 4 * c['CR_WR_SMALL'], c['CR_SWITCH'], 4 * c['CR_WR_BIG']
    return [(sb + 1, TRC.COL_WIDE), (sw - 1, 32), (sw + bb + 1, 32), (sw + 1, TRC.COL_WIDE)]  # one ragged block; either side of the switch, ragged tails


def _col_build(i):
    def build(K):
        import test_row_counts as TRC
        c = TRC.col_case(*_col_rows()[i])
        return (lambda: list(TRC.run_col_kernels(K, c).values())), ()
    return build


for _i, _nm in enumerate(('ragged_block', 'below_switch', 'above_switch_ragged', 'switch_wide')):
    case(f'col-{_nm}', ('colsum', 'colvar_sum', 'bn_bwd_reduce', 'bn_relu_bwd', 'bn_relu_bwd_colsum'))(_col_build(_i))


@case('bn_finalize', ('bn_finalize',))
def _bn_finalize(K):
    L = ops.HeadLayout(200, 'cuda')
    g = torch.Generator().manual_seed(8)
    mean, var, gamma, beta = cu(torch.randn(L.DP, generator=g), torch.rand(L.DP, generator=g) + 0.1, 1 + 0.1 * torch.randn(L.DP, generator=g),
                                torch.randn(L.DP, generator=g))
    rm0, rv0 = cu(torch.randn(200, generator=g), torch.rand(200, generator=g) + 0.5)

    def call():
        outs = []
        for ones_col in (-1, 51):
            run = (rm0.clone(), rv0.clone(), torch.tensor(7, device='cuda'), L.dense_pos, 0.1, 1.01)
            outs += list(K.bn_finalize(mean, var, gamma, beta, 1e-5, run, ones_col)) + list(run[:3])
        return outs + list(K.bn_finalize(mean, var, gamma, beta, 1e-5))
    return call, ()


def _stat_build(tail):
    def build(K):
        import test_row_counts as TRC
        c = TRC.stat_case(TRC.CONST['BF_PARTS'] + 1, tail)
        part, gamma, beta, pos = cu(c.part, c.gamma, c.beta, c.pos)

        def call():
            rm, rv, nbt = c.rm0.clone().cuda(), c.rv0.clone().cuda(), torch.tensor(7, dtype=torch.long, device='cuda')
            return K.bn_stats_finalize(part, c.R, gamma, beta, 1e-5, running=(rm, rv, nbt, pos, 0.1, c.unb)), rm, rv, nbt
        return call, ()
    return build


for _tail in ('full', 'one_row'):
    case(f'bn_stats_finalize-{_tail}', ('bn_stats_finalize',))(_stat_build(_tail))


def _gelu_build(which):
    def build(K):
        import test_row_counts as TRC
        eb = 4 * TRC.CONST['GELU_THREADS']
        c = TRC.gelu_case({'block_plus_one': eb + 4, 'many_blocks': 256 * eb + 4}[which], 0.3)
        X, dY = cu(c.X, c.dY)

        def call():
            y2, wy = K.gelu_dropout_fwd(X, 0.3, TRC.GELU_SEED, amax=True)
            dx2, wdx = K.gelu_dropout_bwd(X, dY, 0.3, TRC.GELU_SEED, amax=True)
            return K.gelu_dropout_fwd(X, 0.3, TRC.GELU_SEED), K.gelu_dropout_bwd(X, dY, 0.3, TRC.GELU_SEED), y2, wy, dx2, wdx, K.absmax(X)
        return call, ()
    return build


for _w in ('block_plus_one', 'many_blocks'):
    case(f'gelu_dropout-{_w}', ('gelu_dropout_fwd', 'gelu_dropout_bwd', 'absmax'))(_gelu_build(_w))


@case('bn_relu_absmax-sin_basis', ('bn_relu_absmax', 'sin_basis'))
def _absmax_sin(K):
    g = torch.Generator().manual_seed(4)
    H, sc, sh = cu(torch.randn(1025, 260, generator=g), torch.randn(260, generator=g), torch.randn(260, generator=g))
    score, js = cu(torch.randn(257, generator=g) * 3, torch.pow(1.1, torch.arange(100).float()))
    return (lambda: (K.bn_relu_absmax(H, sc, sh), K.bn_relu_absmax(H[:1], sc, sh), K.sin_basis(score, js, 112))), ()


# ---- graph and node preparation -------------------------------------------------------------------------------------------------------------
def graph_outputs(g, E):
    """every array of the graph that a kernel reads, over its defined range (E: the batch's true edge count), the chunk tables, the flag
    words with the XCD partition, the live-tile words"""
    import test_hip_kernels as THK
    torch.cuda.synchronize()
    sizes = {'N+1': g.N + 1, 'Ep': E + g.N, 'C': g.C, 'pairs+1': g.c.n_groups * g.C + 1}
    nch = int(g.array('n_chunks', 1).item())
    assert 0 <= nch <= g.max_chunks
    return ([g.array(a, sizes[s]) for a, s in THK.GRAPH_ARRAYS] + [g.array(a, nch) for a in ('chunk_cls', 'chunk_beg', 'chunk_len')] +
            [g.array('n_chunks', 1), g.array('err', 13)] + list(g.live_tiles()))


def _graph_build(way):
    def build(K):
        import test_class_counts as TCC
        import test_hip_kernels as THK
        ei, et, nt, R, T = dict(THK.GRAPH_CASES)['rand_small']()
        E, cap = ei.size(1), ei.size(1) + 37  # a capacity bucket that is not full
        eic, etc, ntc = cu(ei, et, nt)

        def call():
            if way == 'blocked':
                return graph_outputs(K.graph_prep(eic, etc, ntc, R, T, block_n=25), E)
            if way == 'cap':
                return graph_outputs(K.graph_prep_cap(TCC._edge_buffers(ei, et, cap), ntc, R, T), E)
            packed = TCC._blob_batch(ei, et, nt, R, T)
            packed.e_cap = cap
            return graph_outputs(K.graph_from_blobs(packed, ntc), E)
        return call, ()
    return build


for _way, _m in (('blocked', 'graph_prep'), ('cap', 'graph_prep_cap'), ('blobs', 'graph_from_blobs')):
    case(f'graph-{_way}', (_m,))(_graph_build(_way))


@case('graph-store', ('store_gather', 'graph_from_store'))
def _graph_store(K):
    import test_device_store as TDS
    h, ids = TDS._special(), TDS.BATCHES['unsorted']
    d = h.device('cuda')
    E = int(h.store.edge_count[ids].sum())

    def call():
        sb = d.batch(ids, 1)
        sb.e_cap = E + 37
        gathered = sb.gathered()
        return list(gathered) + graph_outputs(K.graph_from_store(sb, sb.fields()[1].reshape(-1)), E)
    return call, ()


@case('node_prep', ('node_prep',))
def _node_prep(K):
    import test_row_counts as TRC
    c = TRC.node_case(65)
    raw, al, nt, cids = cu(c.raw, c.al, c.nt, c.cids)
    return (lambda: list(K.node_prep(raw, al, nt, cids)) + list(K.node_prep(raw, al, nt, cids, table_rows=500))), ()


# ---- attention, pooling and head --------------------------------------------------------------------------------------------------------------
def _edge_build(name, HP):
    def build(K):
        import test_hip_kernels as THK
        c = THK.edge_case(name, HP)
        return (lambda: THK.run_edge_kernels(c)), ()
    return build


for _name, _HP in (('rand_small', 8), ('degree_ladder', 52)):
    case(f'edge_attn-{_name}-{_HP}', ('graph_prep', 'edge_attn_fwd', 'edge_attn_bwd'))(_edge_build(_name, _HP))


@case('pool_attn', ('pool_attn_fwd', 'pool_attn_bwd'))
def _pool(K):
    B, n, NH, Cc, p = 3, 37, 4, 32, 0.3  # the smallest case of test_pool_attention_forward_backward, with dropout
    g = torch.Generator().manual_seed(B * 100 + n)
    u, c, Kx = cu(torch.randn(B, NH, Cc, generator=g) * 0.3, torch.randn(B, NH, generator=g), torch.randn(B, n, Cc, generator=g))
    lens = torch.randint(1, n + 1, (B,), generator=g)
    mask = (torch.arange(n).unsqueeze(0) >= lens.unsqueeze(1)).cuda()
    dz, da = cu(torch.randn(B, NH, Cc, generator=g), torch.randn(B, NH, n, generator=g))

    def call():
        attn, attn_d, z = K.pool_attn_fwd(u, c, Kx, mask, 0.2, p, 12345)
        return [attn, attn_d, z, *K.pool_attn_bwd(u, Kx, 0.2, p, 12345, attn, attn_d, dz, da), *K.pool_attn_bwd(u, Kx, 0.2, p, 12345, attn, attn_d, dz, None)]
    return call, ()


@case('head_post', ('head_post_fwd', 'head_post_bwd'))
def _head(K):
    B, n, NH, DP, dv, Ds, d, p1, p2 = 3, 37, 4, 32, 8, 20, 32, 0.3, 0.2  # the smallest case of test_head_post_forward_backward
    g = torch.Generator().manual_seed(B * 100 + n + NH)
    NO, L = NH * dv, NH * dv + Ds + d
    z, attn = torch.randn(B, NH, DP, generator=g), torch.rand(B, NH, n, generator=g) / n
    BDv, bv = torch.randn(NH * DP, NO, generator=g) * 0.1, torch.randn(NO, generator=g)
    for h in range(NH):
        BDv[h * DP:(h + 1) * DP, :h * dv] = 0
        BDv[h * DP:(h + 1) * DP, (h + 1) * dv:] = 0
    sent, K3 = torch.randn(B, Ds, generator=g), torch.randn(B, n, DP, generator=g)
    w, bfc, dl, dK0 = torch.randn(L, generator=g) * 0.1, torch.randn(1, generator=g), torch.randn(B, generator=g), torch.randn(B, n, DP, generator=g)
    z, attn, BDv, bv, sent, K3, w, bfc, dl, dK0 = cu(z, attn, BDv, bv, sent, K3, w, bfc, dl, dK0)

    def call():
        logits, out, asum = K.head_post_fwd(z, attn, BDv, bv, sent, K3, d, w, bfc, p1, p2, 4711, 815)
        outs = [logits, out, asum]
        for need_dsent in (True, False):
            got = K.head_post_bwd(dl, out, asum, BDv, bv, sent, K3, d, w, p1, p2, 4711, 815, n, need_dsent)
            outs += [t for t in got if t is not None]
        return outs + [K.add_row0(dK0.clone(), got[4])]
    return call, ()


@case('gather_multi', ('gather_multi', 'gather_multi_sum'))
def _gather(K):
    g = torch.Generator().manual_seed(6)
    srcs = [torch.randn(n, generator=g).cuda() for n in (5, 300, 1, 4097)]
    S = 1000
    tid = torch.randint(-1, 4, (3, S), generator=g)
    off = torch.stack([torch.stack([torch.randint(0, srcs[max(int(t), 0)].numel(), ()) for t in row]) for row in tid])
    tid, off = tid.int().cuda(), off.int().cuda()
    return (lambda: (K.gather_multi(srcs, tid[0].contiguous(), off[0].contiguous()), K.gather_multi_sum(srcs[:3] + [None], tid, off))), ()


# ---- hops and stacks ------------------------------------------------------------------------------------------------------------------------------
HOP_WIDTH = {'small_train': (8, 32), 'csqa_b10': (52, 200)}  # head pitch, d (120 rows, 2 000 rows)


@functools.lru_cache(maxsize=None)
def _hop_case(name, k):
    import test_nonfinite as TN
    with mock.patch.dict(TN.HOP_GRAPHS, {name: HOP_WIDTH[name][0]}):
        return TN.hop_case(name, k=k)


def _hop_operands(name, k):
    import test_nonfinite as TN
    c = _hop_case(name, k)
    ei, et, nt, R, T = c['graph']
    return c, cu(ei, et, nt) + [R, T], c['X'].cuda(), c['S'].cuda(), [TN._prm(p, lambda t: t.cuda()) for p in c['prms']]


def _split(K, mode):
    @contextlib.contextmanager
    def scope():
        old, K.gemm_split = K.gemm_split, mode
        try:
            yield
        finally:
            K.gemm_split = old
    return scope()


def _runnings(L, k):
    """the module's dense running statistics of k hops, fresh: (run_mean, run_var, batches tracked, dense_pos, momentum, unbias) each"""
    return [(torch.zeros(L.d, device='cuda'), torch.ones(L.d, device='cuda'), torch.tensor(0, device='cuda'), L.dense_pos, 0.1, 1.0) for _ in range(k)]


def _hop_build(name, split, batch_stats):
    def build(K):
        c, (ei, et, nt, R, T), X, S, prms = _hop_operands(name, 1)
        HP, qs, L = c['HP'], c['qs'], ops.HeadLayout(HOP_WIDTH[name][1], 'cuda')
        assert L.DP == c['DP']
        dy = torch.randn(c['N'], c['DP'], generator=torch.Generator().manual_seed(2)).cuda()
        p, seed = (0.2, 4321) if batch_stats else (0.0, 0)
        form_on = split == 2 and batch_stats  # (hop_h2: the maximum words are live, zeroed and written by the hop)
        fixed = (HP, qs, X, S, nt, prms[0], batch_stats, 1e-5, p, seed, True)

        def call():
            with _split(K, split):
                g = K.graph_prep(ei, et, nt, R, T)
                run = _runnings(L, 1)[0] if batch_stats else None
                y, saved = K.hop_fwd(g, *fixed, run)
                grads = K.hop_bwd(g, *fixed, saved, dy, True, True)  # (on the forward's poisoned saved state, maximum words included)
            # (with the form off the maximum words are not touched and not read: see the header's sentence at qagnn_hop_args.amax)
            return [y, *saved[:6]] + ([saved[6]] if form_on else []) + [t for t in grads if t is not None] + (list(run[:3]) if run else [])
        exempt = () if batch_stats else [Exempt(6, lambda t: t[0:2], STATS_QUOTE, 'hop_bwd, same case')]
        return call, exempt
    return build


def _stack_build(name, split, batch_stats):
    def build(K):
        k = 2
        c, (ei, et, nt, R, T), X, S, prms = _hop_operands(name, k)
        HP, qs, L = c['HP'], c['qs'], ops.HeadLayout(HOP_WIDTH[name][1], 'cuda')
        dy = torch.randn(c['N'], c['DP'], generator=torch.Generator().manual_seed(2)).cuda()
        p, seeds = (0.2, [4321, 4322]) if batch_stats else (0.0, [0, 0])
        form_on = split == 2 and batch_stats
        fixed = (HP, qs, X, S, nt, prms, batch_stats, 1e-5, p, seeds)

        def call():
            with _split(K, split):
                g = K.graph_prep(ei, et, nt, R, T)
                runs = _runnings(L, k) if batch_stats else [None] * k
                y, saved = K.stack_fwd(g, *fixed, runs)
                dX, dS, grads = K.stack_bwd(g, *fixed, saved, dy, True, True)
            outs = [y, *saved[:4]] + ([saved[4]] if form_on else []) + [dX, dS] + [t for gr in grads for t in gr if t is not None]
            return outs + [t for r in runs if r is not None for t in r[:3]]
        exempt = () if batch_stats else [Exempt(4, lambda t: t[:, 0:2], STATS_QUOTE, 'stack_bwd, same case')]
        return call, exempt
    return build


def _infer_build(name, split):
    def build(K):
        k = 2
        c, (ei, et, nt, R, T), X, S, prms = _hop_operands(name, k)
        form_on = split == 2  # (the forward-only stack runs the form on running statistics)

        def call():
            with _split(K, split):
                g = K.graph_prep(ei, et, nt, R, T)
                args = (g, c['HP'], c['qs'], X, S, nt, prms, 1e-5)
                y, amax = K.stack_infer(*args)
                yk, amax_k, (KMQ, aa, rows, stats) = K.stack_infer(*args, keep=True)
                ya, amax_a, a_all = K.stack_infer(*args, attn=True)
            return [y, yk, ya, a_all, KMQ, aa, rows, stats] + ([amax, amax_k, amax_a] if form_on else [])
        return call, [Exempt(7, lambda t: t[:, 0:2], STATS_QUOTE, 'the hops of the same stack (they read run_mean_p / run_var_p)')]
    return build


for _name in HOP_WIDTH:
    for _split_mode in (1, 2):
        for _bs in (True, False):
            _tag = f'{_name}-split{_split_mode}-{"batch" if _bs else "running"}'
            case(f'hop-{_tag}', ('graph_prep', 'hop_fwd', 'hop_bwd'), form=_split_mode == 2)(_hop_build(_name, _split_mode, _bs))
            case(f'stack-{_tag}', ('graph_prep', 'stack_fwd', 'stack_bwd'), form=_split_mode == 2)(_stack_build(_name, _split_mode, _bs))
        case(f'stack_infer-{_name}-split{_split_mode}', ('graph_prep', 'stack_infer'), form=_split_mode == 2)(_infer_build(_name, _split_mode))


# ---- loss, evaluation, explain, optimiser ----------------------------------------------------------------------------------------------------------
@case('choice_loss', ('choice_loss', 'choice_loss_bwd'))
def _loss(K):
    g = torch.Generator().manual_seed(12)
    logits, labels = cu(torch.randn(7, 5, generator=g), torch.randint(0, 5, (7,), generator=g))
    word, three = cu(torch.tensor([0.37]), torch.tensor([3.0]))

    def call():
        outs = []
        for kind in ('cross_entropy', 'margin_rank'):
            stats = torch.zeros(2, dtype=torch.float64, device='cuda')
            loss, gr = K.choice_loss(logits, labels, kind, 0.1, word, stats)
            outs += [loss, gr, K.choice_loss_bwd(gr, three), stats.float()]
        counts = torch.zeros(2, dtype=torch.long, device='cuda')
        pred = _lib.torch.empty(7, dtype=torch.long, device='cuda')  # (as inference.evaluate_detail allocates it)
        K.choice_eval(logits, labels, counts, pred)
        return outs + [counts, pred]
    return call, ()


def _explain_build(cap):
    def build(K):
        import test_explain as TE
        B, n, k = 3, 65, 5  # the smallest case of test_attn_export with real edges
        ei, et, nt = TE.make_graph(B, n, 11 + n, e_rand=100, star=False, pad=0)
        E = ei.size(1)
        cnt = E + B * n

        def call():
            G = TE.dev_graph(K, ei, et, nt, n, e_cap=E + 37 if cap else None)
            a = torch.rand((k, G.Ep, 4), generator=torch.Generator().manual_seed(1)).cuda()
            return [K.attn_export(G, a), *K.attn_trace(G, a, B, n), *K.attn_trace(G, a, B, n, 0, 2)]
        exempt = [Exempt(0, lambda t: t[:, cnt:], EXPORT_QUOTE, 'explain.trace(edges=True) cuts alpha to the live rows: the module cases below')] if cap else ()
        return call, exempt
    return build


for _cap in (False, True):
    case(f'explain-{"capacity" if _cap else "exact"}', ('graph_prep_cap' if _cap else 'graph_prep', 'attn_export', 'attn_trace'))(_explain_build(_cap))


@case('optimiser', ('grad_norm',))
def _optimiser(K):
    import test_grad_clip as TGC
    g = torch.Generator().manual_seed(2)
    total = sum(TGC.SIZES)
    flat, p0, m0, v0 = cu(torch.randn(total, generator=g), torch.randn(total, generator=g), 0.1 * torch.randn(total, generator=g),
                          (0.01 * torch.randn(total, generator=g)) ** 2)

    def call():
        grads, params, ms, vs = (TGC.views(t.clone()) for t in (flat, p0, m0, v0))
        out = K.grad_norm(grads, 1.0)
        K.radam_step(params, grads, ms, vs, 0.9, 0.999, 1e-8, 1e-3, 0.01, 1e-3, 1, grad_scale=out[1:2])  # (scaled as read: the gradients stay)
        K.scale_multi(grads, out[1:2])
        cat = lambda ts: torch.cat([t.reshape(-1) for t in ts])  # noqa: E731
        return out, cat(grads), cat(params), cat(ms), cat(vs)
    return call, ()


# ---- the inventory of binding methods ---------------------------------------------------------------------------------------------------------------
# public methods whose source allocates nothing that a kernel writes: none today.  (A method that only sizes or reads goes here, with why.)
ALLOCATES_NOTHING_A_KERNEL_WRITES = {}
_ALLOC = re.compile(r'torch\.empty(_like)?\(|\.new_empty\(')


def allocating_methods(cls=_lib.HipKernels):
    """the public methods of the binding whose source allocates uninitialised memory, directly or through a method of the class that does"""
    src = {}
    for nm, fn in vars(cls).items():
        fn = fn.__func__ if isinstance(fn, (staticmethod, classmethod)) else fn
        if callable(fn):
            src[nm] = inspect.getsource(inspect.unwrap(fn))
    alloc = {nm for nm, s in src.items() if _ALLOC.search(s)}
    grew = True
    while grew:
        grew = False
        for nm, s in src.items():
            if nm not in alloc and any(re.search(r'self\.%s\(' % re.escape(a), s) for a in alloc):
                alloc.add(nm)
                grew = True
    return sorted(nm for nm in alloc if not nm.startswith('_'))


def test_every_binding_method_that_allocates_is_in_the_case_table():
    """`-m "not gpu"`.  inspect.getsource over HipKernels: a public method whose source allocates (itself, or through a helper of the class)
    appears in the table above or in the short list of methods that allocate nothing a kernel writes."""
    methods = allocating_methods()
    covered = {m for c in CASES.values() for m in c.methods}
    missing = [m for m in methods if m not in covered and m not in ALLOCATES_NOTHING_A_KERNEL_WRITES]
    note(f'FIGURE history methods: {len(methods)} allocating binding methods, {len(CASES)} cases')
    assert len(methods) >= 40, methods
    assert not missing, f'binding methods that allocate and have no case in tests/test_buffer_history.py: {missing}'
    unknown = sorted((covered | set(ALLOCATES_NOTHING_A_KERNEL_WRITES)) - set(dir(_lib.HipKernels)))
    assert not unknown, f'the table names methods the binding does not have: {unknown}'


def test_every_exemption_quotes_a_sentence_of_the_headers():
    """`-m "not gpu"`.  The sentence that declares an exempt region unwritten stands in a public header, word for word (comment layout aside);
    so does the one that lets a call that does not run the three-MFMA form leave the hop's maximum words alone -- why the hop cases return
    those words only where the form runs."""
    flat = lambda s: re.sub(r'[\s*/]+', ' ', s)  # noqa: E731
    hdr = {f: flat(open(os.path.join(helpers.ROOT, 'include', f)).read()) for f in ('qagnn_hip.h', 'qagnn_hip_explain.h')}
    assert flat(STATS_QUOTE) in hdr['qagnn_hip.h']
    assert flat(EXPORT_QUOTE) in hdr['qagnn_hip_explain.h']
    assert flat(AMAX_QUOTE) in hdr['qagnn_hip.h']


def test_the_tn_shapes_reach_every_family_of_the_dispatch():
    """`-m "not gpu"` (the route query is host code): the table's weight-gradient shapes reach every family qagnn_gemm_tn_route_query names
    below the live-tile route, fallbacks and split routes with a ragged last chunk among them; the live-tile route has its own two cases."""
    from qagnn_amd.build import build
    build(verbose=False)
    lib = _lib.load_library()
    out = (C.c_int32 * 4)()

    def query(R, Ka1, Ka2, No):
        assert lib.qagnn_gemm_tn_route_query(R, Ka1, Ka2, No, C.cast(out, C.c_void_p)) == 0
        return tuple(out)
    fam = tn_families(query)
    assert set(fam.values()) == {0, 1, 2, 4}, sorted(set(fam.values()))  # (3: the live-tile route, first at first_ws_rows)
    ragged = [(key, query(*key)) for key in fam if query(*key)[2] > 1 and key[0] % max(query(*key)[1], 1)]
    assert len(ragged) >= 4, ragged


# ---- the GPU run ----------------------------------------------------------------------------------------------------------------------------------
_T0 = [None]


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(CASES))
def test_binding_call_ignores_what_its_fresh_buffers_held(name):
    """One route of one binding method (the table above): run from 0x00 bytes twice, then from 0xFF and 0x7B bytes; the same bits."""
    K = hip()
    _T0[0] = _T0[0] or time.time()
    _lib.ERR_WATCH.poll(block=True)
    spec = CASES[name]
    with (helpers.form_everywhere() if spec.form else contextlib.nullcontext()):
        call, exempt = spec.build(K)
        check_history_free(call, exempt, reset=reset_seeds, what=name, log=LOG)
    torch.cuda.synchronize()
    _lib.ERR_WATCH.poll(block=True)  # (a flag word that kept a fill's 1 would be reported here)
    note(f'FIGURE history wall: {time.time() - _T0[0]:.1f} s after {name}')


# =================================================================================================================================
# 3. The words the caller does own
# =================================================================================================================================
def _f2i(x):
    return torch.tensor([x], dtype=torch.float32).view(torch.int32).item()


def _presets(true_bits):
    """0, a bit pattern below the true maximum, one above it"""
    return [0, true_bits - 0x00800000, true_bits + 0x00800000]


@pytest.mark.gpu
def test_maximum_slots_merge_with_what_the_caller_left_in_them():
    """qagnn_absmax_f32, qagnn_gelu_dropout_{fwd,bwd}_amax_f32 and qagnn_bn_relu_absmax_f32 through the raw entry points with the slot pre-set
    to 0, to a pattern below the true maximum and to one above it: exactly max(pre-set, true) as bit patterns (the documented merge); the
    binding, which zeroes the word itself, gives the true maximum -- from buffers filled with 0xFF and 0x7B bytes too."""
    import test_row_counts as TRC
    K = hip()
    c = TRC.gelu_case(4 * TRC.CONST['GELU_THREADS'] + 4, 0.3)
    X, dY = cu(c.X, c.dY)
    n, s = X.numel(), K._stream()
    g = torch.Generator().manual_seed(4)
    H, sc, sh = cu(torch.randn(257, 260, generator=g), torch.randn(260, generator=g), torch.randn(260, generator=g))
    scratch = torch.full((int(K.lib.qagnn_gelu_dropout_amax_scratch_elems(n)),), float('nan'), device='cuda')
    bra = torch.full((max(int(K.lib.qagnn_bn_relu_absmax_scratch_elems(257, 260)), 1),), float('nan'), device='cuda')
    Y = torch.empty_like(X)
    raw = {
        'absmax': lambda w: K.lib.qagnn_absmax_f32(X.data_ptr(), n, w.data_ptr(), s),
        'gelu_dropout_fwd_amax': lambda w: K.lib.qagnn_gelu_dropout_fwd_amax_f32(X.data_ptr(), Y.data_ptr(), n, 0.3, TRC.GELU_SEED, w.data_ptr(),
                                                                                 scratch.data_ptr(), s),
        'gelu_dropout_bwd_amax': lambda w: K.lib.qagnn_gelu_dropout_bwd_amax_f32(X.data_ptr(), dY.data_ptr(), Y.data_ptr(), n, 0.3, TRC.GELU_SEED,
                                                                                 w.data_ptr(), scratch.data_ptr(), s),
        'bn_relu_absmax': lambda w: K.lib.qagnn_bn_relu_absmax_f32(H.data_ptr(), 260, 257, 260, sc.data_ptr(), sh.data_ptr(), w.data_ptr(), bra.data_ptr(), s),
    }
    binding = {'absmax': lambda: K.absmax(X), 'gelu_dropout_fwd_amax': lambda: K.gelu_dropout_fwd(X, 0.3, TRC.GELU_SEED, amax=True)[1],
               'gelu_dropout_bwd_amax': lambda: K.gelu_dropout_bwd(X, dY, 0.3, TRC.GELU_SEED, amax=True)[1],
               'bn_relu_absmax': lambda: K.bn_relu_absmax(H, sc, sh)}
    for nm, fn in raw.items():
        true = int(binding[nm]()[0])
        assert 0x30000000 < true < 0x50000000, f'{nm}: {true:#x}'
        for fill in helpers.FILLS:
            with fresh_buffers(fill):
                assert int(binding[nm]()[0]) == true, f'{nm}: the binding under {fill}'
        for pre in _presets(true):
            w = torch.tensor([pre, 5, 6, 7], dtype=torch.int32, device='cuda')
            assert fn(w) == 0, K.lib.qagnn_last_error()
            assert w.tolist() == [max(pre, true), 5, 6, 7], f'{nm}: slot pre-set to {pre:#x}, true maximum {true:#x}, left {int(w[0]):#x}'
        w = torch.tensor([true + 0x00800000], dtype=torch.int32, device='cuda')  # bn_relu_absmax through the binding's own `out`: the merge
        if nm == 'bn_relu_absmax':
            assert int(K.bn_relu_absmax(H, sc, sh, out=w)[0]) == true + 0x00800000
        note(f'FIGURE history merge {nm}: true maximum {true:#x}, pre-sets {[hex(p) for p in _presets(true)]} merged exactly')


AMAX_CANARY = 0x7F000000  # a float bit pattern (1.7e38), never an index: the one hostile pattern an int32 buffer gets


def _nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


def _same_bits(a, b, what):
    a, b = helpers._bits(a), helpers._bits(b)
    assert a.shape == b.shape and torch.equal(a, b), f'{what}: {int((a != b).sum())} of {a.numel()} elements differ'
    return a.numel()


@pytest.mark.gpu
@pytest.mark.parametrize('entry', ['hop', 'stack'])
def test_hop_and_stack_entry_points_on_canaried_buffers_equal_the_binding_from_zeros(entry):
    """qagnn_{hop,stack}_{fwd,bwd}_f32 through the raw struct at HP = 16 under form_everywhere (the maximum words are live), on a call that
    SUCCEEDS: every float buffer and the workspaces hold NaN, the maximum words 0x7F000000.  Outputs, saved buffers and maximum words
    after the calls are the bits of the binding's run from zeroed buffers."""
    import test_head_widths as THW
    import test_hip_kernels as THK
    K = hip()
    ei, et, nt, R, T = THK.edge_case('rand_small', 28).graph
    g, nt = K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R, T), nt.cuda()
    HP, k = 16, (1 if entry == 'hop' else 2)
    DP, W = 4 * HP, _lib.HOP_AMAX_WORDS
    with helpers.form_everywhere():
        assert K.gemm_split == 2
        parts = [THW._canaried_hop(K, g, nt, HP, True, canary=float('nan'), amax_word=AMAX_CANARY) for _ in range(k)]
        prms, (X, S, dy) = [p[2][0] for p in parts], parts[0][2][1:4]
        SP = S.size(1)
        n = 0
        if entry == 'hop':
            h, guarded, keep = parts[0]
            amax = keep[4]
            fwd_ws = _nan(int(K.lib.qagnn_hop_fwd_workspace_elems(g.N, g.Ep, DP)))
            bwd_ws = (h.ws, h.ws_elems)
            h.ws, h.ws_elems = fwd_ws.data_ptr(), fwd_ws.numel()
            assert K.lib.qagnn_hop_fwd_f32(C.byref(h), K._stream()) == 0, K.lib.qagnn_last_error()
            h.ws, h.ws_elems = bwd_ws
            h.side_stream = None
            assert K.lib.qagnn_hop_bwd_f32(C.byref(h), K._stream()) == 0, K.lib.qagnn_last_error()
            torch.cuda.synchronize()
            KMQ, aa, rows, stats, flat, dX, dS = guarded[:7]
            sizes, offs = K._grad_sizes(DP, SP, 4, g.C)
            raw_grads = K._carve_grads(_lib.qagnn_hop_args(DP=DP, SP=SP, T=4, ones_col=-1, tab_col=-1), flat, sizes, offs, g.C)
            with fresh_buffers('zero'):
                y, saved = K.hop_fwd(g, HP, 0.25, X, S, nt, prms[0], True, 1e-5, 0.0, 0, True, None)
                got = K.hop_bwd(g, HP, 0.25, X, S, nt, prms[0], True, 1e-5, 0.0, 0, True, saved, dy, True, True)
            torch.cuda.synchronize()
            pairs = [('y', rows[3], y), ('KMQ', KMQ, saved[0]), ('aa', aa, saved[1]), ('aggr', rows[0], saved[2]), ('h1', rows[1], saved[3]),
                     ('out', rows[2], saved[4]), ('stats', stats, saved[5]), ('amax', amax, saved[6]), ('dX', dX, got[0]), ('dS', dS, got[1])]
            pairs += [(f'grad {i}', a, b) for i, (a, b) in enumerate(zip(raw_grads, got[2:])) if b is not None]
        else:
            N, Ep = g.N, g.Ep
            KMQ, aa, rows, stats = _nan(k, N, 3 * DP), _nan(k, 2, Ep, 4), _nan(k, 4, N, DP), _nan(k, 5, DP)
            amax = torch.full((k, W), AMAX_CANARY, dtype=torch.int32, device='cuda')
            ys = rows[:, 3].unbind(0)
            ws = _nan(int(K.lib.qagnn_hop_fwd_workspace_elems(N, Ep, DP)))
            hops = K._hop_chain(g, HP, 0.25, X, S, nt, prms, ys, (KMQ, aa, rows, stats), amax.data_ptr(), None, None, ws, True, 1e-5, 0.0, [0, 0], -1)
            assert K.lib.qagnn_stack_fwd_f32(hops, k, K._stream()) == 0, K.lib.qagnn_last_error()
            sizes, offs = K._grad_sizes(DP, SP, 4, g.C)
            per = offs[-1]
            flat, dxs, dS, dX = _nan(k * per), _nan(max(k - 1, 1), N, DP), _nan(N, SP), _nan(N, DP)
            ws_b = _nan(int(K.lib.qagnn_hop_bwd_workspace_elems(N, Ep, DP, SP, g.cls_part_rows)))
            hops = K._hop_chain(g, HP, 0.25, X, S, nt, prms, ys, (KMQ, aa, rows, stats), amax.data_ptr(), None, None, ws_b, True, 1e-5, 0.0, [0, 0], -1)
            raw_grads = []
            for l, h in enumerate(hops):  # (as _lib.HipKernels.stack_bwd chains them)
                h.dy = dy.data_ptr() if l == k - 1 else dxs.data_ptr() + l * N * DP * 4
                raw_grads.append(K._carve_grads(h, flat[l * per:(l + 1) * per], sizes, offs, g.C))
                h.dX, h.accumulate_dX = (dxs.data_ptr() + (l - 1) * N * DP * 4, 0) if l > 0 else (dX.data_ptr(), 0)
                h.dS, h.accumulate_dS = dS.data_ptr(), (0 if l == k - 1 else 1)
            assert K.lib.qagnn_stack_bwd_f32(hops, k, K._stream()) == 0, K.lib.qagnn_last_error()
            torch.cuda.synchronize()
            with fresh_buffers('zero'):
                y, saved = K.stack_fwd(g, HP, 0.25, X, S, nt, prms, True, 1e-5, 0.0, [0, 0], [None] * k)
                got = K.stack_bwd(g, HP, 0.25, X, S, nt, prms, True, 1e-5, 0.0, [0, 0], saved, dy, True, True)
            torch.cuda.synchronize()
            pairs = [('y', ys[-1], y), ('KMQ', KMQ, saved[0]), ('aa', aa, saved[1]), ('rows', rows, saved[2]), ('stats', stats, saved[3]),
                     ('amax', amax, saved[4]), ('dX', dX, got[0]), ('dS', dS, got[1])]
            pairs += [(f'grad {l}.{i}', a, b) for l in range(k) for i, (a, b) in enumerate(zip(raw_grads[l], got[2][l])) if b is not None]
        assert int(amax.view(-1)[_lib.HOP_AM_X]) not in (0, AMAX_CANARY), 'the maximum words are not live: the form did not run'
        for nm, a, b in pairs:
            n += _same_bits(a, b, f'{entry}: {nm}')
    note(f'FIGURE history raw {entry}: {len(pairs)} tensors, {n} elements equal to the binding from zeros; maximum words '
         f'{[hex(v) for v in amax.view(-1)[:8].tolist()]}')


@pytest.mark.gpu
def test_a_second_backward_on_the_same_saved_state_gives_the_bits_of_the_first():
    """The backward's own maximum words (d out, d h1, d K|M|Q) are merged into words the FORWARD zeroed: a second backward over the same saved
    state, here with a gradient 2^-20 times the first, must start from zeros again -- else it scales its operands by the first call's
    maxima (still a valid bound: nothing turns non-finite, the three-MFMA form only loses 20 bits).  csqa_b10 width (DP = 208, the width
    at which the backward runs the form), under form_everywhere."""
    K = hip()
    c, (ei, et, nt, R, T), X, S, prms = _hop_operands('csqa_b10', 1)
    dy = torch.randn(c['N'], c['DP'], generator=torch.Generator().manual_seed(2)).cuda()
    small = dy * 2.0 ** -20
    fixed = (c['HP'], c['qs'], X, S, nt, prms[0], True, 1e-5, 0.2, 4321, True)
    with helpers.form_everywhere():
        g = K.graph_prep(ei, et, nt, R, T)
        _, saved = K.hop_fwd(g, *fixed, None)
        want = K.hop_bwd(g, *fixed, saved, small, True, True)
        want_words = saved[6].clone()
        _, saved = K.hop_fwd(g, *fixed, None)
        K.hop_bwd(g, *fixed, saved, dy, True, True)
        got = K.hop_bwd(g, *fixed, saved, small, True, True)
        torch.cuda.synchronize()
    assert int(want_words[_lib.HOP_AM_DOUT]) != 0, 'the backward did not run the form'
    assert torch.equal(saved[6], want_words), f'maximum words {saved[6].tolist()} after the second backward, {want_words.tolist()} after a first one'
    for i, (a, b) in enumerate(zip(got, want)):
        _same_bits(a, b, f'output {i} of the second backward')


# =================================================================================================================================
# 4. The module, end to end (eager)
# =================================================================================================================================
MODULE_CASES = ('small_train', 'csqa_b10')


def _module_inputs(name):
    c = helpers.GOLDEN_CASES[name]
    x = helpers.make_case_inputs(c)
    B, n = c['nq'] * c['nc'], c['n']
    labels = torch.randint(0, c['nc'], (c['nq'],), generator=torch.Generator().manual_seed(c['seed']))
    args = cu(x['sent_vecs'], x['concept_ids'].view(B, n), x['node_type_ids'].view(B, n), x['node_scores'].view(B, n, 1), x['adj_lengths'].view(B))
    return c, args, tuple(cu(x['edge_index'], x['edge_type'])), labels.cuda()


def _module(name, ps):
    from qagnn_amd import modeling_qagnn as MQ
    c = helpers.GOLDEN_CASES[name]
    cfg = c['cfg']
    torch.manual_seed(0)
    m = MQ.QAGNN(None, cfg['k'], cfg['n_ntype'], cfg['n_etype'], cfg['sent_dim'], cfg['n_concept'], cfg['concept_dim'], cfg['concept_in_dim'],
                 cfg['n_attention_head'], cfg['fc_dim'], cfg['n_fc_layer'], ps['p_emb'], ps['p_gnn'], ps['p_fc'], pretrained_concept_emb=None,
                 freeze_ent_emb=True, init_range=cfg['init_range'])
    helpers.det_fill_(m, c['seed'], c['std'])
    m.pooler.dropout.p, m.pooler.attention.dropout.p = ps['p_pool'], ps['p_attn']
    return m.cuda()


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['cross_entropy', 'margin_rank'])
@pytest.mark.parametrize('form', helpers.FORMS)
@pytest.mark.parametrize('composed', [False, True], ids=['native', 'composed'])
@pytest.mark.parametrize('name', MODULE_CASES)
def test_module_step_eval_and_trace_ignore_what_fresh_buffers_held(name, composed, form, kind, monkeypatch):
    """Eagerly, with the run scripts' dropout: one training step (forward, compute_loss, backward, clip_grad_norm_, RAdam.step), one eval
    forward on the inference path, one explain.trace(edges=True) -- logits, loss, norm, every parameter gradient, every updated parameter
    and moment, the BatchNorm buffers, the eval logits, the trace's flow / best / pred and its edge tensors, bit for bit under the three
    fills.  No region exempted in the table above is read anywhere downstream."""
    import test_training_loop as TL
    from qagnn_amd import explain, losses
    from qagnn_amd import optimization_utils as OU
    from test_hip_parity import RUN_SCRIPT_DROPOUT
    hip()
    _lib.ERR_WATCH.poll(block=True)
    if composed:
        monkeypatch.setattr(ops, 'FUSED_HOP', False)
    c, args, adj, labels = _module_inputs(name)

    def call():
        model = _module(name, RUN_SCRIPT_DROPOUT).train()
        opt = TL.make_opt(model)
        ops.manual_seed(5)  # (behind the model's construction, which seeds torch for its own initialisation)
        logits, _ = model(*args, adj)
        loss = losses.compute_loss(logits.view(-1, c['nc']), labels, kind, TL.MARGIN, weight=0.5)
        loss.backward()
        norm = OU.clip_grad_norm_(list(model.parameters()), 1.0, defer_to=opt)
        opt.step()
        out = {'logits': logits.detach(), 'loss': loss.detach().reshape(-1), 'norm': norm.detach().reshape(-1)}
        for k_, p in model.named_parameters():
            out['param ' + k_] = p.detach()
            if p.grad is not None:
                out['grad ' + k_] = p.grad
            st = opt.state.get(p)
            if st:
                out['exp_avg ' + k_], out['exp_avg_sq ' + k_] = st['exp_avg'], st['exp_avg_sq']
        for k_, v in model.named_buffers():
            out['buffer ' + k_] = v.float() if v.dtype == torch.long else v
        model.eval()
        with torch.no_grad():
            with ops.inference_path():
                out['eval logits'] = model(*args, adj)[0]
            tr = explain.trace(model, *args, adj, edges=True)
        out.update({'trace flow': tr.flow, 'trace best': tr.best, 'trace pred': tr.pred, 'trace alpha': tr.alpha, 'trace edge_index': tr.edge_index,
                    'trace edge_type': tr.edge_type, 'trace logits': tr.logits})
        keys.clear()
        keys.extend(out)
        return [out[k_].float() if out[k_].dtype == torch.float64 else out[k_] for k_ in keys]
    keys = []
    with contextlib.ExitStack() as stack:
        if form == 'everywhere':
            stack.enter_context(helpers.form_everywhere())
        n, _ = check_history_free(call, reset=reset_seeds, what=f'module {name} {"composed" if composed else "native"} {form} {kind}', log=LOG)
    assert sum(1 for k_ in keys if k_.startswith('grad ')) > 40 and n > 100000
    _lib.ERR_WATCH.poll(block=True)
