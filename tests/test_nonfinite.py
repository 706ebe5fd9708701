"""Non-finite propagation, kernel by kernel and through the hop, the stack and the module (the contract in include/qagnn_hip.h).

A NaN or an inf that enters a kernel must come out where the float64 emulation (tests/emu_kernels.py: torch's semantics) puts it: the
set of non-finite output elements is the emulation's, and every element the emulation leaves finite stays finite and inside the bound
the kernel's own test uses, with the bound's |A| @ |B| terms formed from the operands with their poisoned entries zeroed.  One
comparison helper (check_nonfinite) does that for every test below.  The poisons are NaN, +inf and -inf in float data, never in an
index array.  The single exemption is the one-edge softmax segment of the edge kernels (a = alpha = 1 without reading the score, and
the exact zero of that segment's softmax gradient in the backward): the edge tests count the exempted positions and hold them equal to
the number of poisoned one-edge segments.
"""
import contextlib

import numpy as np
import pytest
import torch

import helpers
from emu_kernels import EmuGraph, EmuKernels
from test_hip_kernels import EPS, HEAD_DIM, _h2_bound, edge_case, edge_inputs, hip

EMU = EmuKernels()
NAN, INF = float('nan'), float('inf')
POISONS = (NAN, INF, -INF)
FWD = dict(rtol=1e-4, atol=1e-5)  # the forward bars of tests/test_hip_parity.py


def pname(v):
    return 'nan' if v != v else ('+inf' if v > 0 else '-inf')


def zeroed(t):
    """|t| with the non-finite entries zeroed: what the bounds' |A| @ |B| terms are formed from"""
    return torch.nan_to_num(t.double().abs(), nan=0.0, posinf=0.0, neginf=0.0)


def dbl(t):
    return None if t is None else (t.double() if t.is_floating_point() else t)


def check_nonfinite(what, got, ref, bound=None, exempt=None, outliers=0, superset=False):
    """The one comparison of this file.  isfinite(got) == isfinite(ref) elementwise (outside `exempt`, a bool mask), and
    |got - ref| <= bound where ref is finite; where the bound itself is not finite (an inf operand word) finiteness alone is asserted.
    `outliers`: how many finite elements may miss the bound (the ReLU-kink allowance of the BatchNorm backward tests).
    `superset`: for an inf poison through a CHAIN of kernels -- the contract lets one kernel turn an inf into a NaN (the low piece of a
    split inf), and relu(bn(-inf)) is 0 where relu(bn(NaN)) is NaN, so downstream of it the reference's non-finite set is only a lower
    bound: every element the reference leaves non-finite must be non-finite here, the bound holds where both are finite.
    Returns the number of non-finite reference elements."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, f'{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
    fg, fr = torch.isfinite(got), torch.isfinite(ref)
    differ = (fg & ~fr) if superset else (fg != fr)
    if exempt is not None:
        differ = differ & ~exempt
    if bool(differ.any()):
        idx = differ.nonzero()[0].tolist()
        laundered, invented = int((differ & fg).sum()), int((differ & fr).sum())
        raise AssertionError(f'{what}: non-finite sets differ at {int(differ.sum())} of {ref.numel()} elements ({laundered} finite where the '
                             f'reference is not, {invented} non-finite where the reference is finite; the reference has {int((~fr).sum())} '
                             f'non-finite), first at {idx}: got {got[tuple(idx)].item()}, reference {ref[tuple(idx)].item()}')
    if bound is not None:
        ok = fr & fg
        b = bound if torch.is_tensor(bound) else torch.full_like(ref, float(bound))
        b = b.detach().cpu().double().expand_as(ref)
        ok = ok & torch.isfinite(b)
        err = torch.where(ok, (got - ref).abs(), torch.zeros_like(ref))
        bad = ok & (err > b)
        if int(bad.sum()) > outliers:
            idx = torch.where(bad, err / b.clamp_min(1e-300), torch.zeros_like(err)).argmax()
            idx = np.unravel_index(int(idx), ref.shape) if ref.dim() else ()
            raise AssertionError(f'{what}: {int(bad.sum())} finite elements outside the bound, worst |d| = {err[idx].item():.3e} against '
                                 f'{b[idx].item():.3e} at {list(map(int, idx))}')
    return int((~fr).sum())


def close_bound(ref, rtol, atol):
    """helpers._close's bound on the finite part of `ref`: atol + rtol * max(|ref|, max finite |ref|)"""
    fin = torch.nan_to_num(ref.double().abs(), nan=0.0, posinf=0.0, neginf=0.0)
    return atol + rtol * torch.clamp(fin, min=fin.max().item() if fin.numel() else 0.0)


class Failures:
    """collects the failing sites of one parametrised case, so that one run names them all"""

    def __init__(self):
        self.msgs, self.checked, self.poisoned = [], 0, 0

    def run(self, fn):
        try:
            self.poisoned += fn() or 0
        except AssertionError as e:
            self.msgs.append(str(e))
        self.checked += 1

    def done(self, min_checked=1):
        assert self.checked >= min_checked
        assert not self.msgs, f'{len(self.msgs)} of {self.checked} sites failed:\n  ' + '\n  '.join(self.msgs[:12])
        assert self.poisoned > 0, 'no site produced a non-finite reference element: the poisons missed'


# ---------------------------------------------------------------------------------------------------------------------------------------
# One hop / a stack of hops on a small graph: operands on the CPU in fp32, run by the emulation in float64 or by the library
# ---------------------------------------------------------------------------------------------------------------------------------------
HOP_GRAPHS = {'small_train': 8, 'degree_ladder': 52}  # graph -> head pitch (120 rows, d = 32; 329 rows, d = 200)


def hop_case(name, k=1, seed=77):
    HP = HOP_GRAPHS[name]
    (ei, et, nt, R, T), _, _, _, qs = edge_inputs(name, HP, 5)
    gen = torch.Generator().manual_seed(seed)
    N, DP, C, SP = nt.numel(), 4 * HP, R * T * T + T, 112 if HP == 52 else 16
    rnd = lambda *shape, s=0.3: torch.randn(*shape, generator=gen) * s  # noqa: E731
    prms = []
    for _ in range(k):
        Wx_t, Ws_t, W1t, W2t = rnd(DP, 3 * DP, s=0.1), rnd(SP, 3 * DP, s=0.1), rnd(DP, DP, s=0.1), rnd(DP, DP, s=0.1)
        prms.append([Wx_t, None, Ws_t, None, rnd(T, 3 * DP), rnd(C, 2 * DP), W1t, None, rnd(DP), 1 + rnd(DP), rnd(DP), W2t, None, rnd(DP),
                     rnd(DP), 0.5 + rnd(DP).abs()])
    X, S = rnd(N, DP, s=1.0), rnd(N, SP, s=1.0)
    src = ei[0]
    deg = torch.bincount(src, minlength=N)
    node = int(src[(deg[src] > 1).nonzero()[0]])                      # a node with out-edges of its own
    e0 = int((deg[src] > 1).nonzero()[0])
    cls = int(et[e0] * T * T + nt[ei[0, e0]] * T + nt[ei[1, e0]])     # the class of a real edge (never a self loop's)
    return dict(name=name, HP=HP, qs=qs, graph=(ei, et, nt, R, T), prms=prms, X=X, S=S, N=N, DP=DP, node=node, cls=cls, k=k)


def poisoned(case, site, value):
    """a copy of the hop operands with one poison: a node row of X, W1t[3][5] of the first hop, or one Ek|Em class row of every hop"""
    c = dict(case, prms=[[None if t is None else t.clone() for t in p] for p in case['prms']], X=case['X'].clone())
    if site == 'X_row':
        c['X'][case['node']] = value
    elif site == 'W1t':
        c['prms'][0][6][3, 5] = value
    elif site == 'EkEm_row':
        for p in c['prms']:
            p[5][case['cls']] = value
    else:
        assert site == 'none'
    return c


def _prm(p, conv):
    p = [None if t is None else conv(t) for t in p]
    for nn_, t_ in ((1, 0), (3, 2), (7, 6), (12, 11)):  # the [No, K] layouts the split kernels take beside the [K, No] ones
        p[nn_] = p[t_].t().contiguous()
    return tuple(p)


def run_hops(case, K, batch_stats, native, device='cpu'):
    """-> the list, hop by hop, of dict(y, KMQ, aggr, h1, out, stats) (float64 through the emulation, fp32 through the library)"""
    from qagnn_amd import ops
    ei, et, nt, R, T = case['graph']
    emu = isinstance(K, EmuKernels)
    conv = (lambda t: t.double()) if emu else (lambda t: t.to(device))
    g = EmuGraph(ei, et, nt, R, T) if emu else K.graph_prep(ei.to(device), et.to(device), nt.to(device), R, T)
    x, S, ntype = conv(case['X']), conv(case['S']), nt.to(device)
    p, k = (0.2 if batch_stats else 0.0), case['k']
    prms = [_prm(pr, conv) for pr in case['prms']]
    seeds = [4321 + l for l in range(k)] if p else [0] * k
    names = ('KMQ', 'aa', 'aggr', 'h1', 'out', 'stats')
    if native and k > 1:
        y, saved = K.stack_fwd(g, case['HP'], case['qs'], x, S, ntype, prms, batch_stats, 1e-5, p, seeds, [None] * k)
        rows, stats = saved[2], saved[3]
        return [dict(aggr=rows[l, 0], h1=rows[l, 1], out=rows[l, 2], y=rows[l, 3], stats=stats[l]) for l in range(k)]
    res = []
    for l in range(k):
        args = (g, case['HP'], case['qs'], x, S, ntype, prms[l], batch_stats, 1e-5, p, seeds[l], True, None)
        y, saved = K.hop_fwd(*args) if native else ops.hop_fwd_composed(K, *args)
        res.append(dict(zip(names, saved[:6]), y=y))
        x = y
    return res


def check_hops(what, got, ref, batch_stats, superset=False):
    """every forward buffer of every hop through check_nonfinite; finite values at the forward bar; -> non-finite reference elements"""
    n = 0
    for l, (g_, r_) in enumerate(zip(got, ref)):
        for nm in ('KMQ', 'aggr', 'h1', 'out', 'y'):
            if nm in g_:
                n += check_nonfinite(f'{what} hop {l} {nm}', g_[nm], r_[nm], close_bound(r_[nm], **FWD), superset=superset)
        if batch_stats:  # mean | var | invstd | scale | shift of the batch (under running statistics rows 0, 1 are not written)
            n += check_nonfinite(f'{what} hop {l} stats', g_['stats'][:5], r_['stats'][:5], close_bound(r_['stats'][:5], **FWD), superset=superset)
    return n


HOP_SITES = ('X_row', 'W1t', 'EkEm_row')


# ---------------------------------------------------------------------------------------------------------------------------------------
# CPU: the yardsticks propagate as torch does, and the helper rejects a laundering answer that the finite-input comparisons accept
# ---------------------------------------------------------------------------------------------------------------------------------------
TINY = dict(shape='tiny', nq=3, nc=4, n=37, n_rel=17, std=0.6, seed=31, cfg=helpers.model_cfg(d=100, k=3, sent_dim=40, n_concept=500, concept_in_dim=24))
DEVICE = 'cuda'  # the CPU self-check (tests/test_host_logic_emu.py) runs module_vs_oracle with 'cpu' and the emulation
# poison -> the subgraphs whose logit the reference leaves non-finite in eval mode (train mode: BatchNorm's batch statistics spread it to all)
MODULE_POISONS = {'weight': set(range(12)), 'embedding': {5}, 'score': {7}}


def _module_poison(poison, model, args):
    """applies `poison` to a model (package or oracle: same parameter names) and / or to the input list, in place"""
    sv, cids, nt, ns, al, ei, et = args
    with torch.no_grad():
        if poison == 'weight':
            dict(model.named_parameters())['gnn.gnn_layers.1.mlp.0.weight'][3, 5] = NAN
        elif poison == 'embedding':
            ids = cids.cpu()
            mine = [int(i) for i in ids[5, 1:int(al[5])] if int((ids == i).sum()) == 1]  # a concept only subgraph 5 reads
            assert mine, 'subgraph 5 shares every concept with another subgraph'
            dict(model.named_parameters())['concept_emb.emb.weight'][mine[0] - 1] = NAN
        else:
            assert poison == 'score'
            ns[7, 3] = INF
    return args


def module_vs_oracle(poison, train, device=None):
    """The package's QAGNN against the fp32 oracle under one poison: equal non-finite logit sets, the finite logits at the forward bars,
    and after backward every parameter whose oracle gradient holds a non-finite value holds one here.  Returns (non-finite subgraphs,
    parameters with a non-finite gradient here but not in the oracle -- reported, not asserted: autograd forms 0 x NaN where a
    hand-derived backward need not)."""
    import test_hip_parity as T
    device = device or DEVICE
    case = dict(TINY, train=train)
    args, _ = T._case_args(case)
    B = case['nq'] * case['nc']
    w = torch.linspace(0.5, 1.5, B).view(B, 1)
    oracle = helpers.build_oracle(case)
    oargs = _module_poison(poison, oracle, [a.clone() for a in args])
    ologits, _ = oracle(*oargs[:5], (oargs[5], oargs[6]))
    (ologits * w).sum().backward()
    model = T._package_model(case, 'cpu')
    margs = _module_poison(poison, model, [a.clone() for a in args])
    model = model.to(device)
    margs = [a.to(device) for a in margs]
    logits, _ = model(*margs[:5], (margs[5], margs[6]))
    (logits * w.to(device)).sum().backward()
    check_nonfinite(f'logits [{poison}, {"train" if train else "eval"}]', logits, ologits.detach(), close_bound(ologits.detach(), **FWD))
    bad = set((~torch.isfinite(ologits.detach().view(-1))).nonzero().flatten().tolist())
    ours = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    theirs = {k: p.grad for k, p in oracle.named_parameters() if p.grad is not None}
    missing = [k for k, g in theirs.items() if not bool(torch.isfinite(g).all()) and (k not in ours or bool(torch.isfinite(ours[k]).all()))]
    assert not missing, f'{poison}: the oracle gradient of {missing[:6]} ({len(missing)} tensors) holds a non-finite value, the package gradient is finite'
    extra = [k for k, g in ours.items() if not bool(torch.isfinite(g).all()) and (k not in theirs or bool(torch.isfinite(theirs[k]).all()))]
    n_bad = sum(1 for g in theirs.values() if not bool(torch.isfinite(g).all()))
    print(f'FIGURE nonfinite module [{poison}, {"train" if train else "eval"}]: non-finite logits {sorted(bad)}; oracle gradients with a non-finite '
          f'value {n_bad}/{len(theirs)}; non-finite here only: {extra}')
    return bad, extra


@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('poison', list(MODULE_POISONS))
def test_emulation_and_oracle_give_the_same_logit_masks(poison, train):
    """`-m "not gpu"`: pins the yardsticks to torch's semantics -- the package on the emulation and the oracle leave the same logits
    non-finite: one subgraph's for a poisoned embedding row or node score in eval mode, all twelve otherwise."""
    from qagnn_amd import ops
    old = ops.set_kernels(EmuKernels())
    try:
        bad, _ = module_vs_oracle(poison, train, device='cpu')
    finally:
        ops.set_kernels(old)
    assert bad == (set(range(12)) if train else MODULE_POISONS[poison])


def test_batchnorm_running_statistics_of_a_poisoned_column():
    """`-m "not gpu"`: torch.nn.BatchNorm1d in train mode stores NaN running statistics for a column that holds a NaN, and so do
    EmuKernels.bn_finalize and EmuKernels.bn_stats_finalize (the yardsticks of the GPU tests below); the other columns agree."""
    g = torch.Generator().manual_seed(3)
    R, Cc = 129, 8
    x = torch.randn(R, Cc, generator=g, dtype=torch.float64) * 2 + 1
    x[77, 3] = NAN
    bn = torch.nn.BatchNorm1d(Cc).double().train()
    bn(x)
    want = torch.arange(Cc) == 3
    assert torch.equal(torch.isnan(bn.running_mean), want) and torch.equal(torch.isnan(bn.running_var), want)
    gamma, beta, pos, unb = torch.ones(Cc, dtype=torch.float64), torch.zeros(Cc, dtype=torch.float64), torch.arange(Cc), R / (R - 1.0)
    mean, var = x.mean(0), x.var(0, unbiased=False)
    for which in ('bn_finalize', 'bn_stats_finalize'):
        rm, rv = torch.zeros(Cc, dtype=torch.float64), torch.ones(Cc, dtype=torch.float64)
        running = (rm, rv, torch.tensor(0), pos, 0.1, unb)
        if which == 'bn_finalize':
            stats = torch.stack((mean, var) + tuple(EMU.bn_finalize(mean, var, gamma, beta, 1e-5, running)))
        else:
            stats = EMU.bn_stats_finalize(EMU.col_partials(x), R, gamma, beta, 1e-5, running)
        assert torch.equal(torch.isnan(stats), want.expand(5, Cc)), which
        check_nonfinite(which + ' running_mean', rm, bn.running_mean, 1e-12)
        check_nonfinite(which + ' running_var', rv, bn.running_var, 1e-12)


class LaunderingEmu(EmuKernels):
    """A wrong answer built from the reference: the ReLU of the operand prologue written as fmax(x, 0), which drops a NaN, and a
    nan_to_num on the batch variance -- what the kernels computed before the non-finite contract."""

    @staticmethod
    def _pre(A, a_scale, a_shift):
        return torch.fmax(A * a_scale + a_shift, torch.zeros((), dtype=A.dtype))

    def gemm_nn(self, A1, B1, A2=None, B2=None, bias=None, rowtab=None, rowidx=None, a_scale=None, a_shift=None, **kw):
        if a_scale is not None:
            A1, a_scale, a_shift = self._pre(A1, a_scale, a_shift), torch.ones_like(a_scale), torch.zeros_like(a_shift)
        return super().gemm_nn(A1, B1, A2, B2, bias, rowtab, rowidx, a_scale, a_shift, **kw)

    def bn_finalize(self, mean, var, gamma, beta, eps, running=None, ones_col=-1):
        return super().bn_finalize(mean, torch.nan_to_num(var, nan=0.0), gamma, beta, eps, running, ones_col)


@pytest.mark.parametrize('batch_stats', [False, True], ids=['running', 'batch'])
def test_the_helper_rejects_a_laundering_answer_the_finite_comparisons_accept(batch_stats):
    """`-m "not gpu"`: on finite inputs the laundering answer IS the reference (the comparisons the suite made before accept it); on a
    poisoned hop the helper rejects it and names the tensor."""
    case = hop_case('small_train')
    ref = run_hops(case, EMU, batch_stats, native=False)
    bad = run_hops(case, LaunderingEmu(), batch_stats, native=False)
    for nm in ('KMQ', 'aggr', 'h1', 'out', 'y'):
        helpers._close(bad[0][nm], ref[0][nm], what=nm, **FWD)
        assert bool(torch.isfinite(bad[0][nm]).all())
    pc = poisoned(case, 'W1t', NAN)
    ref = run_hops(pc, EMU, batch_stats, native=False)
    assert check_hops('the reference itself', ref, ref, batch_stats) > 0 and not bool(torch.isfinite(ref[0]['y']).any())
    with pytest.raises(AssertionError, match=r'hop 0 (out|stats): non-finite sets differ .* finite where the reference is not'):
        check_hops('laundering', run_hops(pc, LaunderingEmu(), batch_stats, native=False), ref, batch_stats)


def test_the_emulation_reads_a_zero_row_for_a_negative_index():
    """`-m "not gpu"`: _gather_rows selects the zero row (a NaN table row 0 does not leak into the rows of index -1), and the operand
    self-check of gemm_nn accepts a poisoned B with its poisoned transpose."""
    table = torch.ones(4, 3, dtype=torch.float64)
    table[0] = NAN
    got = EMU._gather_rows(table, torch.tensor([-1, 0, 2]))
    assert bool((got[0] == 0).all()) and bool(torch.isnan(got[1]).all()) and bool((got[2] == 1).all())
    B = torch.ones(3, 2, dtype=torch.float64)
    B[1, 1] = NAN
    out = EMU.gemm_nn(table, B, a_rowidx=torch.tensor([-1, 2]), B1n=B.t().contiguous())
    assert torch.equal(torch.isfinite(out), torch.tensor([[True, False], [True, False]]))  # (0 x NaN: the zero row meets B's NaN)
    with pytest.raises(AssertionError, match='B1n must be B1 transposed'):
        EMU.gemm_nn(table, B, B1n=torch.ones(2, 3, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU, per kernel, through the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------------
cu = lambda t: None if t is None else t.cuda()  # noqa: E731
NN_TRIPLES = [(208, 112, 624), (208, 0, 208), (32, 16, 96), (16, 0, 16)]


def _nn_call(K, route, o):
    """one NN product on `route`: 'fp32' (the fp32-MFMA kernels: no [No, K] layouts), 'six' (the exact bf16 split), 'three' (operand
    words from qagnn_absmax_f32, the caller holds helpers.form_everywhere)"""
    A1, B1, A2, B2 = o['A1'], o['B1'], o.get('A2'), o.get('B2')
    kw = {k: cu(o[k]) for k in ('bias', 'rowtab', 'rowidx', 'a_scale', 'a_shift', 'a_rowidx') if o.get(k) is not None}
    if route != 'fp32':
        kw.update(B1n=cu(B1.t().contiguous()), B2n=cu(B2.t().contiguous()) if A2 is not None else None)
    if route == 'three':
        # the word of A1 is that of the operand the MFMAs see: after the prologue, over the gathered table
        A1e = torch.relu(A1 * o['a_scale'] + o['a_shift']) if o.get('a_scale') is not None else A1
        kw.update(a_amax1=K.absmax(cu(A1e.contiguous()).view(-1)), a_amax2=K.absmax(cu(A2).view(-1)) if A2 is not None else None)
    old, K.gemm_split = K.gemm_split, (0 if route == 'fp32' else 2)
    try:
        out = cu(o['C0'].clone()) if o.get('C0') is not None else None
        return K.gemm_nn(cu(A1), cu(B1), cu(A2), cu(B2), out=out, accumulate=out is not None, **kw).cpu()
    finally:
        K.gemm_split = old


def _nn_ref_and_bound(route, o):
    A1, B1, A2, B2 = o['A1'], o['B1'], o.get('A2'), o.get('B2')
    kw = {k: dbl(o[k]) for k in ('bias', 'rowtab', 'rowidx', 'a_scale', 'a_shift', 'a_rowidx') if o.get(k) is not None}
    ref = EMU.gemm_nn(dbl(A1), dbl(B1), dbl(A2), dbl(B2), **kw)
    if o.get('C0') is not None:
        ref = ref + o['C0'].double()
    Ag = EMU._gather_rows(A1, o.get('a_rowidx'))
    A1e = torch.relu(Ag * o['a_scale'] + o['a_shift']) if o.get('a_scale') is not None else Ag
    refz = torch.nan_to_num(ref, nan=0.0, posinf=0.0, neginf=0.0)
    if route == 'three':  # test_gemm_nn_three_mfma_form's bound, the absolute floor written in the words the kernel was handed
        w1 = torch.relu(A1 * o['a_scale'] + o['a_shift']) if o.get('a_scale') is not None else A1
        w1 = w1[~torch.isnan(w1)].abs().max().item() if bool((~torch.isnan(w1)).any()) else 0.0
        w2 = A2[~torch.isnan(A2)].abs().max().item() if A2 is not None else None
        z = lambda t: None if t is None else torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)  # noqa: E731
        return ref, _h2_bound(z(A1e), z(B1), z(A2), z(B2), refz, w1, w2)
    bound = 8 * EPS * (zeroed(A1e) @ zeroed(B1)) + 1e-6 + 4 * EPS * refz.abs()  # test_gemm_nn's bound
    if A2 is not None:
        bound = bound + 8 * EPS * (zeroed(A2) @ zeroed(B2))
    return ref, bound


def _nn_sites(M, K1, K2, No, g):
    """(site name, operands) of one shape: every poison site of the NN products, each with the three poisons"""
    base = dict(A1=torch.randn(M, K1, generator=g), B1=torch.randn(K1, No, generator=g))
    if K2:
        base.update(A2=torch.randn(M, K2, generator=g), B2=torch.randn(K2, No, generator=g))
    bias, rowtab, rowidx = torch.randn(No, generator=g), torch.randn(4, No, generator=g), torch.randint(0, 4, (M,), generator=g)
    scale, shift, C0 = torch.randn(K1, generator=g), torch.randn(K1, generator=g), torch.randn(M, No, generator=g)
    V = 9
    table, idx = torch.randn(V, K1, generator=g), torch.randint(1, V, (M,), generator=g)
    idx[0] = 3
    idx[1::3] = -1
    idx[2::5] = 0
    r, j, k = M // 2, No // 3, K1 // 2
    c = lambda d, **kw: dict({n: (t.clone() if torch.is_tensor(t) else t) for n, t in d.items()}, **{n: t.clone() for n, t in kw.items()})  # noqa: E731
    for v in POISONS:
        def put(o, key, *index):
            o[key][index] = v
            return o
        yield f'A1[0][0]={pname(v)}', put(c(base), 'A1', 0, 0)
        yield f'A1[M-1][K1-1]={pname(v)}', put(c(base), 'A1', M - 1, K1 - 1)
        if K2:
            yield f'A2[r][0]={pname(v)}', put(c(base), 'A2', r, 0)
        yield f'B1[k][No-1]={pname(v)}', put(c(base), 'B1', k, No - 1)
        yield f'bias[j]={pname(v)}', put(c(base, bias=bias), 'bias', j)
        yield f'rowtab row={pname(v)}', put(c(base, bias=bias, rowtab=rowtab, rowidx=rowidx), 'rowtab', int(rowidx[0]))
        yield f'C0[r][j]={pname(v)}', put(c(base, C0=C0), 'C0', r, j)
        yield f'affine A1[r][k]={pname(v)}', put(c(base, a_scale=scale, a_shift=shift), 'A1', r, k)
        gat = dict(A1=table, B1=base['B1'], bias=bias, a_rowidx=idx)
        o = put(c(gat), 'A1', 3, slice(None))
        yield f'gathered table rows 0 and 3={pname(v)}', put(o, 'A1', 0, slice(None))
    yield 'affine a_scale[k]=nan', dict(c(base, a_shift=shift), a_scale=torch.where(torch.arange(K1) == k, torch.tensor(NAN), scale))
    yield 'affine a_shift[k]=nan', dict(c(base, a_scale=scale), a_shift=torch.where(torch.arange(K1) == k, torch.tensor(NAN), shift))
    o = c(base, a_scale=scale.abs() + 0.1, a_shift=shift)
    o['A1'][r, k] = -INF  # relu(-inf * positive + shift) = 0: stays finite, as in torch
    yield 'affine A1[r][k]=-inf under a positive scale', o


@pytest.mark.gpu
@pytest.mark.parametrize('route', ['fp32', 'six', 'three'])
@pytest.mark.parametrize('K1,K2,No', NN_TRIPLES)
@pytest.mark.parametrize('M', [1, 257])
def test_gemm_nn_nonfinite(M, K1, K2, No, route):
    """qagnn_gemm_nn_f32 / qagnn_gemm_nn_split_f32 under every poison site: one row / one column / one element / every row non-finite,
    as the emulation has it, the rest inside the route's bound."""
    K = hip()
    g = torch.Generator().manual_seed(M + K1 + K2 + No)
    F = Failures()
    finite_sites = 0
    with (helpers.form_everywhere() if route == 'three' else contextlib.nullcontext()):
        for site, o in _nn_sites(M, K1, K2, No, g):
            if route == 'three' and o.get('a_scale') is not None and K1 > 256:
                continue

            def one(site=site, o=o):
                ref, bound = _nn_ref_and_bound(route, o)
                return check_nonfinite(f'gemm_nn[{route}] {site}', _nn_call(K, route, o), ref, bound)
            F.run(one)
            finite_sites += 'positive scale' in site
    assert finite_sites == 1
    F.done(min_checked=25)


TN_SHAPES = [(7, 208, 208), (7, 32, 96), (7, 112, 624), (2049, 208, 208), (2049, 32, 96), (2049, 112, 624)]


def _tn_bound(Ae, B):
    return 16 * EPS * (zeroed(Ae).t() @ zeroed(B)) + 1e-6  # test_gemm_tn's bound


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['plain', 'affine', 'a_rowidx', 'colsum1', 'colsum4', 'h2'])
@pytest.mark.parametrize('R,Ka,No', TN_SHAPES)
def test_gemm_tn_nonfinite(R, Ka, No, variant):
    """qagnn_gemm_tn_colsum_f32 / qagnn_gemm_tn_h2_f32: a poisoned A[r][k] poisons row k of C, a poisoned B[r][j] column j of C and of
    the column-sum by-product; under the prologue a NaN a_scale[k] / a_shift[k] poisons row k."""
    K = hip()
    g = torch.Generator().manual_seed(R + Ka + No)
    A, B = torch.randn(R, Ka, generator=g), torch.randn(R, No, generator=g)
    scale, shift = torch.randn(Ka, generator=g), torch.randn(Ka, generator=g)
    V = 9
    table, idx = torch.randn(V, Ka, generator=g), torch.randint(1, V, (R,), generator=g)
    idx[0], idx[1::3], gidx = 3, -1, torch.randint(0, 4, (R,), generator=g)
    r, k, j = R // 2, Ka // 3, No - 1
    sites = [(f'{nm}={pname(v)}', nm, v) for v in POISONS for nm in ('A[r][k]', 'A[R-1][Ka-1]', 'B[r][j]', 'B[0][0]')]
    if variant in ('affine', 'h2'):
        sites += [('a_scale[k]=nan', 'scale', NAN), ('a_shift[k]=nan', 'shift', NAN)]
    F = Failures()
    for site, nm, v in sites:
        a, b, sc, sh = (table if variant == 'a_rowidx' else A).clone(), B.clone(), scale.clone(), shift.clone()
        if nm == 'A[r][k]':
            a[3 if variant == 'a_rowidx' else r, k] = v
            if variant == 'a_rowidx':
                a[0, k] = v  # (row 0 is read by nobody: the rows of index -1 read zeros)
        elif nm == 'A[R-1][Ka-1]':
            a[(int(idx[R - 1]) if idx[R - 1] >= 0 else 3) if variant == 'a_rowidx' else R - 1, Ka - 1] = v
        elif nm == 'B[r][j]':
            b[r, j] = v
        elif nm == 'B[0][0]':
            b[0, 0] = v
        elif nm == 'scale':
            sc[k] = v
        else:
            sh[k] = v

        def one(site=site, a=a, b=b, sc=sc, sh=sh):
            kw, kwd, n = {}, {}, 0
            if variant in ('affine', 'h2'):
                kw, kwd = dict(a_scale=cu(sc), a_shift=cu(sh)), dict(a_scale=sc.double(), a_shift=sh.double())
            if variant == 'a_rowidx':
                kw, kwd = dict(a_rowidx=cu(idx)), dict(a_rowidx=idx)
            groups = {'colsum1': 1, 'colsum4': 4}.get(variant, 0)
            ridx = gidx if groups == 4 else None
            ref = EMU.gemm_tn(a.double(), b.double(), **kwd)
            Ae = EMU._gather_rows(a, kwd.get('a_rowidx'))
            Ae = torch.relu(Ae * sc + sh) if 'a_scale' in kw else Ae
            if variant == 'h2':
                w = lambda t: K.absmax(cu(t.contiguous()).view(-1))  # noqa: E731
                got = K.gemm_tn_h2(cu(a), cu(b), w(Ae), w(b), **kw)
                fin = lambda t: t[torch.isfinite(t)].abs().max().item() if bool(torch.isfinite(t).any()) else 0.0  # noqa: E731
                wa, wb = (INF if bool(torch.isinf(t).any()) else fin(t) for t in (Ae, b))
                floor = 2.0 ** -38 * R * wa * wb if np.isfinite(wa) and np.isfinite(wb) else INF  # (test_gemm_tn_three_mfma_form's)
                n += check_nonfinite(f'gemm_tn_h2 {site}', got, ref, _tn_bound(Ae, b) + floor)
                return n
            got = K.gemm_tn(cu(a), cu(b), colsum_groups=groups, b_rowidx=cu(ridx), **kw)
            if groups:
                got, cs = got
                cs_ref = EMU.colsum(b.double(), ridx, groups)
                n += check_nonfinite(f'gemm_tn[{variant}] {site} bsum', cs, cs_ref, 8 * EPS * zeroed(b).sum(0).max().item() + 1e-6)
            return n + check_nonfinite(f'gemm_tn[{variant}] {site}', got, ref, _tn_bound(Ae, b))
        F.run(one)
    F.done(min_checked=12)


@pytest.mark.gpu
@pytest.mark.parametrize('R,Ka1,Ka2,No', [(700, 32, 16, 96), (2049, 208, 112, 624)])
def test_gemm_tn_nonfinite_two_operands(R, Ka1, Ka2, No):
    """qagnn_gemm_tn2_f32: [A1 | A2]^T B; a poison in A2 poisons a row of the lower block only, one in B a column of both."""
    K = hip()
    g = torch.Generator().manual_seed(R + Ka1 + Ka2)
    A1, A2, B = torch.randn(R, Ka1, generator=g), torch.randn(R, Ka2, generator=g), torch.randn(R, No, generator=g)
    F = Failures()
    for v in POISONS:
        for nm, (t, i) in dict(A1=(0, (R // 2, Ka1 - 1)), A2=(1, (R - 1, 0)), B=(2, (R // 3, No // 2))).items():
            ops_ = [A1.clone(), A2.clone(), B.clone()]
            ops_[t][i] = v

            def one(nm=nm, ops_=ops_):
                a = torch.cat(ops_[:2], 1)
                return check_nonfinite(f'gemm_tn2 {nm}={pname(v)}', K.gemm_tn2(*[cu(x) for x in ops_]), a.double().t() @ ops_[2].double(),
                                       _tn_bound(a, ops_[2]))
            F.run(one)
    F.done(min_checked=9)


@pytest.mark.gpu
@pytest.mark.parametrize('R,C', [(5, 32), (257, 208)])
def test_column_reductions_nonfinite(R, C):
    """qagnn_colreduce_f32 modes 0 (plain, grouped, row-weighted), 1 and 2: a poisoned element poisons its column's sums and no other."""
    K = hip()
    g = torch.Generator().manual_seed(R * 7 + C)
    X, H = torch.randn(R, C, generator=g), torch.randn(R, C, generator=g) * 2 + 0.3
    idx, w = torch.randint(0, 4, (R,), generator=g), torch.rand(R, generator=g) + 0.1
    mean = H.mean(0)
    invstd = torch.rsqrt(H.var(0, unbiased=False) + 1e-5)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    scale, shift = gamma * invstd, beta - mean * gamma * invstd
    r, c = R // 2, C - 1
    F = Failures()
    for v in POISONS:
        Xp, Hp = X.clone(), H.clone()
        Xp[r, c], Hp[r, c] = v, v
        tol0 = 4 * EPS * zeroed(Xp).sum(0).max().item() + 1e-6
        F.run(lambda: check_nonfinite(f'colsum {pname(v)}', K.colsum(cu(Xp)), EMU.colsum(Xp.double()), tol0))
        F.run(lambda: check_nonfinite(f'colsum grouped {pname(v)}', K.colsum(cu(Xp), cu(idx), 4), EMU.colsum(Xp.double(), idx, 4), tol0))
        F.run(lambda: check_nonfinite(f'colsum weighted {pname(v)}', K.colsum(cu(Xp), roww=cu(w)), EMU.colsum(Xp.double(), roww=w.double()), 2 * tol0))
        ref = EMU.colvar_sum(Hp.double(), mean.double())
        F.run(lambda: check_nonfinite(f'colvar_sum {pname(v)}', K.colvar_sum(cu(Hp), cu(mean)), ref, 8 * EPS * torch.nan_to_num(ref, nan=0.0, posinf=0.0) + 1e-6))
        # mode 2: sum dy | sum dy * hhat with dy = dR masked by relu'(bn(H)).  A poisoned dR poisons both sums of its column; a NaN H passes
        # the gradient (torch's relu backward), so the first sum stays finite and the second does not
        tol2 = 8 * EPS * (zeroed(X) * (1 + ((H - mean) * invstd).abs())).sum(0).max().item() + 3 * X.abs().max().item() * 4
        for nm, (xx, hh) in dict(dR=(Xp, H), H=(X, Hp)).items():
            args = (xx, hh, mean, invstd, scale, shift)
            F.run(lambda: check_nonfinite(f'bn_bwd_reduce {nm}={pname(v)}', K.bn_bwd_reduce(*[cu(t) for t in args]),
                                          EMU.bn_bwd_reduce(*[t.double() for t in args]), tol2))
    sc = scale.clone()
    sc[c] = NAN
    args = (X, H, mean, invstd, sc, shift)
    F.run(lambda: check_nonfinite('bn_bwd_reduce scale[c]=nan', K.bn_bwd_reduce(*[cu(t) for t in args]), EMU.bn_bwd_reduce(*[t.double() for t in args]), tol2))
    F.done(min_checked=19)


@pytest.mark.gpu
@pytest.mark.parametrize('train', [True, False])
def test_bn_finalize_nonfinite(train):
    """qagnn_bn_finalize_f32: a NaN / inf mean or variance of a column reaches invstd, scale, shift and (train) the running buffers of
    that column as in the emulation (= torch.nn.BatchNorm1d's bookkeeping); the other columns at the tolerances of the finite test."""
    from qagnn_amd.ops import HeadLayout
    L = HeadLayout(200, torch.device('cuda'))
    K = hip()
    g = torch.Generator().manual_seed(5)
    Cc, d = L.DP, 200
    mean0, var0 = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.1
    gamma, beta = torch.randn(Cc, generator=g), torch.randn(Cc, generator=g)
    rm0, rv0 = torch.randn(d, generator=g), torch.rand(d, generator=g) + 0.5
    col = int(L.dense_pos[17])
    F = Failures()
    for v in POISONS:
        for which in ('mean', 'var'):
            mean, var = mean0.clone(), var0.clone()
            (mean if which == 'mean' else var)[col] = v

            def one(mean=mean, var=var, which=which):
                rm_g, rv_g, nbt_g = rm0.cuda(), rv0.cuda(), torch.tensor(7).cuda()
                rm_e, rv_e, nbt_e = rm0.double(), rv0.double(), torch.tensor(7)
                running = (rm_g, rv_g, nbt_g, L.dense_pos, 0.1, 64000.0 / 63999.0) if train else None
                erunning = (rm_e, rv_e, nbt_e, L.dense_pos.cpu(), 0.1, 64000.0 / 63999.0) if train else None
                got = K.bn_finalize(cu(mean), cu(var), cu(gamma), cu(beta), 1e-5, running)
                ref = EMU.bn_finalize(mean.double(), var.double(), gamma.double(), beta.double(), 1e-5, erunning)
                n = 0
                for nm, a, b in zip(('invstd', 'scale', 'shift'), got, ref):
                    n += check_nonfinite(f'bn_finalize {which}={pname(v)} {nm}', a, b, 1e-6 + 2e-6 * torch.nan_to_num(b, nan=0.0, posinf=0.0, neginf=0.0).abs())
                n += check_nonfinite(f'bn_finalize {which}={pname(v)} running_mean', rm_g, rm_e, 1e-7 + 1e-6 * torch.nan_to_num(rm_e, nan=0.0, posinf=0.0, neginf=0.0).abs())
                n += check_nonfinite(f'bn_finalize {which}={pname(v)} running_var', rv_g, rv_e, 1e-7 + 1e-6 * torch.nan_to_num(rv_e, nan=0.0, posinf=0.0, neginf=0.0).abs())
                return n
            F.run(one)
    F.done(min_checked=6)


@pytest.mark.gpu
@pytest.mark.parametrize('M', [77, 129])
def test_bn_stats_finalize_nonfinite(M):
    """qagnn_bn_stats_finalize_f32 behind a colstats GEMM whose output has one poisoned column (a poisoned bias / weight element): that
    column's mean, variance, invstd, scale, shift and running buffers are non-finite, every other column is unchanged to the tolerances
    of test_gemm_column_statistics_and_bn_stats_finalize."""
    from qagnn_amd import ops
    g = torch.Generator().manual_seed(M)
    Kd, No, d = 208, 208, 200
    L = ops.HeadLayout(d, 'cpu')
    A, Bt = torch.randn(M, Kd, generator=g), torch.randn(Kd, No, generator=g) * 0.1
    bias0 = torch.randn(No, generator=g) * 3.0 + 5.0
    gamma, beta = torch.rand(No, generator=g) + 0.5, torch.randn(No, generator=g)
    rm0, rv0 = torch.randn(d, generator=g) * 0.1, torch.rand(d, generator=g) + 0.5
    K = hip()
    col = int(L.dense_pos[11])
    unb = M / max(M - 1.0, 1.0)
    F = Failures()
    for v in POISONS:
        for which in ('bias', 'weight'):
            bias, B = bias0.clone(), Bt.clone()
            if which == 'bias':
                bias[col] = v
            else:
                B[Kd // 2, col] = v

            def one(bias=bias, B=B, which=which):
                out, part = K.gemm_nn(cu(A), cu(B), bias=cu(bias), B1n=cu(B.t().contiguous()), colstats=True)
                ref_out = EMU.gemm_nn(A.double(), B.double(), bias=bias.double())
                n = check_nonfinite(f'colstats GEMM {which}={pname(v)}', out, ref_out,
                                    8 * EPS * (zeroed(A) @ zeroed(B)) + 1e-6 + 4 * EPS * torch.nan_to_num(ref_out, nan=0.0, posinf=0.0, neginf=0.0).abs())
                rm, rv, nbt = rm0.clone().cuda(), rv0.clone().cuda(), torch.tensor(7, dtype=torch.long, device='cuda')
                stats = K.bn_stats_finalize(part, M, cu(gamma), cu(beta), 1e-5, running=(rm, rv, nbt, L.dense_pos.cuda(), 0.1, unb))
                o64 = out.cpu().double()  # the statistics describe the GEMM's own output, as in the finite test
                rm_e, rv_e = rm0.double(), rv0.double()
                ref = EMU.bn_stats_finalize(EMU.col_partials(o64), M, gamma.double(), beta.double(), 1e-5, (rm_e, rv_e, torch.tensor(7), L.dense_pos, 0.1, unb))
                rz = torch.nan_to_num(ref, nan=0.0, posinf=0.0, neginf=0.0).abs()
                bars = torch.stack([2e-6 * rz[0].max().expand(No), 1e-5 * rz[1], 1e-5 * rz[2], 1e-5 * rz[3].max().expand(No), 2e-5 * rz[4].max().expand(No)])
                n += check_nonfinite(f'bn_stats_finalize {which}={pname(v)} stats', stats, ref, bars + 1e-12)
                assert bool((~torch.isfinite(ref[:, col])).all()), 'the poisoned column must be non-finite in all five rows of the reference'
                n += check_nonfinite(f'bn_stats_finalize {which}={pname(v)} running_mean', rm, rm_e, 1e-6 + 1e-5 * torch.nan_to_num(rm_e, nan=0.0).abs())
                n += check_nonfinite(f'bn_stats_finalize {which}={pname(v)} running_var', rv, rv_e, 1e-6 + 1e-5 * torch.nan_to_num(rv_e, nan=0.0).abs())
                assert int(nbt) == 8
                return n
            F.run(one)
    F.done(min_checked=6)


@pytest.mark.gpu
@pytest.mark.parametrize('R,C', [(5, 32), (257, 208)])
@pytest.mark.parametrize('colsum', [False, True])
def test_bn_relu_bwd_nonfinite(R, C, colsum):
    """qagnn_bn_relu_bwd_f32 / qagnn_bn_relu_bwd_colsum_f32: a poisoned dR[r][c] or H[r][c] poisons that element (and the column sum of
    its column); where the forward value is NaN the gradient passes, as in torch; a poisoned reduction word poisons its column."""
    K = hip()
    g = torch.Generator().manual_seed(R + C)
    dR, H = torch.randn(R, C, generator=g), torch.randn(R, C, generator=g) * 2 + 0.3
    mean = H.mean(0)
    invstd = torch.rsqrt(H.var(0, unbiased=False) + 1e-5)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    scale, shift = gamma * invstd, beta - mean * gamma * invstd
    red = EMU.bn_bwd_reduce(*[t.double() for t in (dR, H, mean, invstd, scale, shift)]).float().contiguous()
    r, c = R // 2, C // 2
    F = Failures()
    for v in POISONS:
        for nm in ('dR', 'H', 'red'):
            a, h, rd = dR.clone(), H.clone(), red.clone()
            if nm == 'dR':
                a[r, c] = v
            elif nm == 'H':
                h[r, c] = v
            else:
                rd[0, c] = v
            for inv_rows in (1.0 / R, 0.0):
                def one(a=a, h=h, rd=rd, nm=nm, inv_rows=inv_rows):
                    args = (a, h, mean, invstd, scale, shift, gamma, rd)
                    ref = EMU.bn_relu_bwd(*[t.double() for t in args], inv_rows)
                    bar = 1e-4 * (1 + torch.nan_to_num(ref, nan=0.0, posinf=0.0, neginf=0.0).abs())  # (the finite test's, with its two kink flips)
                    what = f'bn_relu_bwd{"_colsum" if colsum else ""} {nm}={pname(v)} inv_rows={inv_rows:.3g}'
                    if not colsum:
                        return check_nonfinite(what, K.bn_relu_bwd(*[cu(t) for t in args], inv_rows), ref, bar, outliers=2)
                    dH, cs = K.bn_relu_bwd_colsum(*[cu(t) for t in args], inv_rows)
                    n = check_nonfinite(what, dH, ref, bar, outliers=2)
                    # (the sums are those of the kernel's own output, as the finite test has it)
                    return n + check_nonfinite(what + ' colsum', cs, dH.cpu().double().sum(0), 4 * EPS * zeroed(dH.cpu()).sum(0).max().item() + 1e-6)
                F.run(one)
    F.done(min_checked=12)


@pytest.mark.gpu
@pytest.mark.parametrize('p', [0.0, 0.2])
@pytest.mark.parametrize('n', [4, 1028, 77 * 208])
def test_gelu_dropout_nonfinite_and_amax_words(n, p):
    """qagnn_gelu_dropout_{fwd,bwd}_f32 and their _amax variants (1028 = one full block plus one lane): values and non-finite sets against
    the emulation; the two variants write the same tensor; the word equals qagnn_absmax_f32 of the tensor the kernel wrote, bit for
    bit, on finite data, with a NaN (skipped) and with an inf (0x7F800000)."""
    K = hip()
    g = torch.Generator().manual_seed(n)
    X0, dY0 = torch.randn(n, generator=g) * 2, torch.randn(n, generator=g)
    seed = 0x1234567ABCDEF
    F = Failures()
    for v in (None,) + POISONS:
        X, dY = X0.clone(), dY0.clone()
        if v is not None:
            X[n // 3] = v
            dY[(2 * n) // 3] = v

        def one(X=X, dY=dY):
            tag = 'finite' if v is None else pname(v)
            y, (ya, wf) = K.gelu_dropout_fwd(cu(X), p, seed), K.gelu_dropout_fwd(cu(X), p, seed, amax=True)
            dx, (dxa, wb) = K.gelu_dropout_bwd(cu(X), cu(dY), p, seed), K.gelu_dropout_bwd(cu(X), cu(dY), p, seed, amax=True)
            yr, dxr = EMU.gelu_dropout_fwd(X.double(), p, seed), EMU.gelu_dropout_bwd(X.double(), dY.double(), p, seed)
            z = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0).abs().max().item()  # noqa: E731
            cnt = check_nonfinite(f'gelu_dropout_fwd {tag}', y, yr, 2e-6 * (1 + z(yr)))
            cnt += check_nonfinite(f'gelu_dropout_bwd {tag}', dx, dxr, 2e-6 * (1 + z(dxr)))
            for nm, a, b, w in (('fwd', y, ya, wf), ('bwd', dx, dxa, wb)):
                r_ = yr if nm == 'fwd' else dxr  # (the variant's own tensor: the same formula, an FMA contraction may differ by an ulp)
                check_nonfinite(f'gelu_dropout_{nm}_amax {tag}', b, r_, 2e-6 * (1 + z(r_)))
                assert w[0].item() == K.absmax(b)[0].item(), f'gelu_dropout_{nm}_amax {tag}: word {w[0].item():#x} != absmax of the written tensor'
                t = b.cpu()
                want = t[~torch.isnan(t)].abs().max() if bool((~torch.isnan(t)).any()) else torch.zeros(())
                assert w[0].item() == want.view(torch.int32).item(), f'gelu_dropout_{nm}_amax {tag}: word {w[0].item():#x}, max over the non-NaN elements {want}'
                if bool(torch.isinf(t).any()):
                    assert w[0].item() == 0x7F800000
            return cnt + (v is None)
        F.run(one)
    F.done(min_checked=4)


# ---- edge attention ------------------------------------------------------------------------------------------------------------------

def _edge_sites(case):
    """(name, tensor, index) poison sites of an edge case: whole K|M|Q rows of a one-edge, a register-path and a hub node, a whole
    Ek|Em row of a real edge's class, single elements in rows of degree > 1, single elements of G"""
    e, HP, DP = case.e, case.HP, 4 * case.HP
    deg_s = (e.rowptr_s[1:] - e.rowptr_s[:-1])
    deg_t = (e.rowptr_t[1:] - e.rowptr_t[:-1])
    pick = lambda m: int(m.nonzero()[-1]) if bool(m.any()) else None  # noqa: E731
    rows = dict(row_one_edge=pick((deg_s == 1) & (deg_t == 1)), row_register=pick((deg_s > 1) & (deg_s <= 64)), row_hub=pick(deg_s > 64))
    sites = [(nm, 'KMQ', (r, slice(None))) for nm, r in rows.items() if r is not None]
    real = e.cls_s[e.cls_s < e.R * e.T * e.T]
    sites.append(('class_row', 'EkEm', (int(real[0]), slice(None))))
    multi = int(((deg_s > 1) & (deg_t > 1)).nonzero()[0])
    sites += [('K elem', 'KMQ', (multi, 1)), ('M elem', 'KMQ', (multi, DP + HP + 1)), ('Q elem', 'KMQ', (multi, 2 * DP + 2 * HP)),
              ('Ek elem', 'EkEm', (int(real[-1]), 3)), ('Em elem', 'EkEm', (int(real[-1]), DP + 3)), ('G elem', 'G', (multi, HP + 2))]
    return sites


def _edge_reference(case, KMQ, EkEm, G):
    """the emulation in float64, with the documented exemption applied: at one-edge source segments a = alpha = 1 whatever the score"""
    e = case.e
    aggr, a, alpha = EMU.edge_attn_fwd(e, KMQ.double(), EkEm.double(), case.HP, case.qs)
    deg_s = (e.rowptr_s[1:] - e.rowptr_s[:-1])
    one = (deg_s == 1)[e.src_s.long()]                                  # positions of the one-edge segments
    exempt = (one & ~torch.isfinite(a).all(1)).unsqueeze(1).expand_as(a)   # ... whose reference value is not finite
    a1, alpha1 = torch.where(exempt, torch.ones_like(a), a), torch.where(exempt, torch.ones_like(alpha), alpha)
    dKMQ, dEkEm = EMU.edge_attn_bwd(e, KMQ.double(), EkEm.double(), case.HP, case.qs, a1, alpha1, G.double())
    return dict(aggr=aggr, a=a, alpha=alpha, dKMQ=dKMQ, dEkEm=dEkEm), exempt


@pytest.mark.gpu
@pytest.mark.parametrize('name,HP', [('class_ladder', 52), ('class_ladder', 8), ('degree_ladder', 52), ('degree_ladder', 8)])
def test_edge_attention_nonfinite(name, HP):
    """qagnn_edge_attn_{fwd,bwd}_f32 under poisoned node rows, class rows and single elements.  Exempt: a and alpha of a one-edge
    segment (the kernel writes 1 without reading the score) and, in the backward, dQ of such a segment (its softmax gradient is exactly
    zero, written without reading a row); the exempted positions are counted and must be exactly the poisoned one-edge segments."""
    base = edge_case(name, HP)
    K = hip()
    (ei, et, nt, R, T), DP = base.graph, 4 * HP
    g = K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R, T)
    e = base.e
    deg_s = (e.rowptr_s[1:] - e.rowptr_s[:-1])
    F = Failures()
    exempted = 0
    for site, which, index in _edge_sites(base):
        for v in POISONS:
            t = dict(KMQ=base.KMQ.clone(), EkEm=base.EkEm.clone(), G=base.G.clone())
            t[which][index] = v

            def one(t=t, site=site, v=v):
                nonlocal exempted
                ref, ex_a = _edge_reference(base, t['KMQ'], t['EkEm'], t['G'])
                aggr, a, alpha = K.edge_attn_fwd(g, cu(t['KMQ']), cu(t['EkEm']), HP, base.qs)
                dKMQ, dEkEm = K.edge_attn_bwd(g, cu(t['KMQ']), cu(t['EkEm']), HP, base.qs, a, alpha, cu(t['G']))
                got = dict(aggr=aggr, a=a, alpha=alpha, dKMQ=dKMQ, dEkEm=dEkEm)
                # the exempted positions: rows of a / alpha at the poisoned one-edge segments, dQ rows of the same source nodes
                seg = torch.unique(e.src_s.long()[ex_a[:, 0]])
                n_poisoned = int(((deg_s == 1) & ~torch.isfinite(t['KMQ'][:, 2 * DP:].double().sum(1) + t['KMQ'][:, :DP].double().sum(1)
                                                                 + t['EkEm'][:, :DP].double()[e.R * e.T * e.T + nt].sum(1))).sum())
                assert int(ex_a[:, 0].sum()) == seg.numel() == n_poisoned, f'{site}: {int(ex_a[:, 0].sum())} exempted positions, {n_poisoned} poisoned one-edge segments'
                exempted += seg.numel()
                ex_q = torch.zeros_like(ref['dKMQ'], dtype=torch.bool)
                ex_q[seg, 2 * DP:] = True
                if seg.numel():
                    assert bool((a.cpu()[ex_a] == 1).all()) and bool((alpha.cpu()[ex_a] == 1).all()) and bool((dKMQ.cpu()[ex_q] == 0).all())
                n = 0
                for nm in ('a', 'alpha', 'aggr', 'dKMQ', 'dEkEm'):
                    r_ = ref[nm]
                    scale = torch.nan_to_num(r_, nan=0.0, posinf=0.0, neginf=0.0).abs().max().item() + 1e-30
                    n += check_nonfinite(f'edge[{name}-{HP}] {site}={pname(v)} {nm}', got[nm], r_, base.bars[nm] * scale,
                                         exempt=ex_a if nm in ('a', 'alpha') else (ex_q if nm == 'dKMQ' else None))
                return n
            F.run(one)
    F.done(min_checked=24)
    if name == 'degree_ladder':
        assert exempted == 3, f'{exempted} exempted one-edge segments over the three poisons of the one-edge row'


# ---- the remaining kernels -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_pool_attention_nonfinite():
    """qagnn_pool_attn_{fwd,bwd}_f32 at (B, n, NH, Cc) = (3, 37, 4, 32): a poisoned unmasked row poisons its subgraph's softmax; a
    poisoned MASKED row has attention 0 and still poisons the weighted sum, the reference's 0 x NaN."""
    B, n, NH, Cc = 3, 37, 4, 32
    g = torch.Generator().manual_seed(B * 100 + n)
    u, c = torch.randn(B, NH, Cc, generator=g) * 0.3, torch.randn(B, NH, generator=g)
    Kx = torch.randn(B, n, Cc, generator=g)
    lens = torch.tensor([5, 37, 20])
    mask = torch.arange(n).unsqueeze(0) >= lens.unsqueeze(1)
    dz, da = torch.randn(B, NH, Cc, generator=g), torch.randn(B, NH, n, generator=g)
    K, seed, it = hip(), 12345, 0.2
    F = Failures()
    for v in POISONS:
        for site, (b, l) in dict(unmasked=(2, 7), masked=(0, 30)).items():
            for p in (0.0, 0.3):
                Kp = Kx.clone()
                Kp[b, l] = v

                def one(Kp=Kp, site=site, p=p):
                    what = f'pool {site} row={pname(v)} p={p}'
                    got = K.pool_attn_fwd(cu(u), cu(c), cu(Kp), cu(mask), it, p, seed)
                    ref = EMU.pool_attn_fwd(u.double(), c.double(), Kp.double(), mask, it, p, seed)
                    cnt = 0
                    for nm, a, r_, at in zip(('attn', 'attn_d', 'z'), got, ref, (1e-6, 1e-6, 1e-5)):
                        cnt += check_nonfinite(f'{what} {nm}', a, r_, at + 1e-4 * torch.nan_to_num(r_, nan=0.0, posinf=0.0, neginf=0.0).abs())
                    for dattn in (da, None):
                        gb = K.pool_attn_bwd(cu(u), cu(Kp), it, p, seed, got[0], got[1], cu(dz), cu(dattn))
                        rb = EMU.pool_attn_bwd(u.double(), Kp.double(), it, p, seed, ref[0], ref[1], dz.double(), dbl(dattn))
                        for nm, a, r_ in zip(('dK', 'du', 'dc'), gb, rb):
                            rz = torch.nan_to_num(r_, nan=0.0, posinf=0.0, neginf=0.0).abs()
                            cnt += check_nonfinite(f'{what} {nm}', a, r_, 2e-5 * max(1.0, rz.max().item()) + 2e-4 * rz)
                    return cnt
                F.run(one)
    F.done(min_checked=12)


@pytest.mark.gpu
def test_head_post_nonfinite():
    """qagnn_head_post_{fwd,bwd}_f32 at the smallest parameter set of their finite test: a poisoned z, sent or K3 element of one
    subgraph poisons that subgraph's logit and gradients only; a poisoned weight poisons every logit."""
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
    K, s1, s2 = hip(), 4711, 815
    base = dict(z=z, attn=attn, BDv=BDv, bv=bv, sent=sent, K3=K3, w=w, dl=dl)
    sites = dict(z=(1, 2, 3), attn=(1, 0, 5), sent=(2, 4), K3=(0, 0, 1), w=(NO + 3,), bv=(2,), dl=(1,))
    F = Failures()
    for v in POISONS:
        for nm, index in sites.items():
            t = {k: x.clone() for k, x in base.items()}
            t[nm][index] = v

            def one(t=t, nm=nm):
                what = f'head_post {nm}={pname(v)}'
                got = K.head_post_fwd(cu(t['z']), cu(t['attn']), cu(t['BDv']), cu(t['bv']), cu(t['sent']), cu(t['K3']), d, cu(t['w']), cu(bfc), p1, p2, s1, s2)
                ref = EMU.head_post_fwd(*[t[k].double() for k in ('z', 'attn', 'BDv', 'bv', 'sent', 'K3')], d, t['w'].double(), bfc.double(), p1, p2, s1, s2)
                cnt = 0
                for lbl, a, r_, at in zip(('logits', 'out', 'asum'), got, ref, (2e-4, 2e-5, 2e-5)):
                    cnt += check_nonfinite(f'{what} {lbl}', a.view_as(r_), r_, at + 2e-4 * torch.nan_to_num(r_, nan=0.0, posinf=0.0, neginf=0.0).abs())
                gb = K.head_post_bwd(cu(t['dl']), got[1], got[2], cu(t['BDv']), cu(t['bv']), cu(t['sent']), cu(t['K3']), d, cu(t['w']), p1, p2, s1, s2, n, True)
                rb = EMU.head_post_bwd(t['dl'].double(), ref[1], ref[2], t['BDv'].double(), t['bv'].double(), t['sent'].double(), t['K3'].double(), d,
                                       t['w'].double(), p1, p2, s1, s2, n, True)
                for lbl, a, r_ in zip(('dz', 'dattn', 'dout', 'dsent', 'dZ', 'part'), gb, rb):
                    rz = torch.nan_to_num(r_, nan=0.0, posinf=0.0, neginf=0.0).abs()
                    cnt += check_nonfinite(f'{what} {lbl}', a, r_, 2e-5 * max(1.0, rz.max().item()) + 2e-4 * rz)
                return cnt
            F.run(one)
    F.done(min_checked=21)


@pytest.mark.gpu
def test_node_prep_nonfinite():
    """qagnn_node_prep_f32 on small_train's loader tensors with an inf (and a NaN) raw score in a real slot, in a PAD slot and in the
    context slot: the subgraph's normalised scores are non-finite where the reference's elementwise ops leave them so; mask and row ids
    do not depend on the scores."""
    c = helpers.GOLDEN_CASES['small_train']
    inp = helpers.make_case_inputs('small_train')
    B, n = c['nq'] * c['nc'], c['n']
    ns, al = inp['node_scores'].view(B, n, 1).clone(), inp['adj_lengths'].view(B).clone()
    nt, cids = inp['node_type_ids'].view(B, n).clone(), inp['concept_ids'].view(B, n).clone()
    K = hip()
    F = Failures()
    for v in POISONS:
        for site, (b, l) in dict(real=(1, 1), pad=(2, n - 1), context=(3, 0)).items():
            if site == 'real':
                assert int(al[b]) > l
            if site == 'pad':
                assert int(al[b]) <= l
            nsp = ns.clone()
            nsp[b, l, 0] = v

            def one(nsp=nsp, site=site):
                score_e, mask_e, ridx_e = EMU.node_prep(nsp.double(), al, nt, cids.clone())
                score, mask, ridx = K.node_prep(cu(nsp), cu(al), cu(nt), cu(cids))
                assert torch.equal(mask.cpu(), mask_e) and torch.equal(ridx.cpu(), ridx_e)
                return check_nonfinite(f'node_prep {site} slot={pname(v)}', score, score_e, 4 * 1.2e-7 * torch.nan_to_num(score_e, nan=0.0, posinf=0.0, neginf=0.0).abs() + 1e-30)
            F.run(one)
    F.done(min_checked=9)


@pytest.mark.gpu
def test_sin_basis_nonfinite():
    """qagnn_sin_basis_f32: sin of a NaN or an inf score is NaN in all J live columns of that row; the pad columns stay 0."""
    g = torch.Generator().manual_seed(5)
    js = torch.pow(1.1, torch.arange(100).float())
    F = Failures()
    for v in POISONS:
        score = torch.randn(130, generator=g) * 3
        score[0], score[77] = v, v
        F.run(lambda: check_nonfinite(f'sin_basis {pname(v)}', hip().sin_basis(cu(score), cu(js), 112), EMU.sin_basis(score, js, 112), 5e-7))
    F.done(min_checked=3)


@pytest.mark.gpu
@pytest.mark.parametrize('step', [1, 6])
def test_radam_step_nonfinite(step):
    """qagnn_radam_step_f32 (step 1: the un-rectified branch, step 6: the rectified one): a non-finite gradient element poisons that
    element of p, m and v as the float64 oracle has it, and nothing else."""
    from oracle import radam_oracle as RO
    from qagnn_amd import optimization_utils as OU
    hip()
    g = torch.Generator().manual_seed(step)
    F = Failures()
    for v in POISONS:
        params = [torch.nn.Parameter(torch.randn(s, generator=g).cuda()) for s in ((7, 5), (1030,))]
        p0 = [p.detach().cpu().numpy().astype(np.float64) for p in params]
        grads = [torch.randn(p.shape, generator=g) for p in params]
        grads[0][3, 2], grads[1][1028] = v, v
        m0 = [0.01 * torch.randn(p.shape, generator=g) for p in params]
        v0 = [(0.01 * torch.randn(p.shape, generator=g)) ** 2 for p in params]
        opt = OU.RAdam(params, lr=1e-3, weight_decay=0.01)
        for p, gr, m, vv in zip(params, grads, m0, v0):
            p.grad = gr.cuda()
            opt.state[p] = dict(step=step - 1, exp_avg=m.clone().cuda(), exp_avg_sq=vv.clone().cuda())
        opt.step()

        def one():
            n = 0
            for i, (p, pb, gr, m, vv) in enumerate(zip(params, p0, grads, m0, v0)):
                with np.errstate(all='ignore'):
                    rp, rm, rv = RO.radam_step(pb, gr.numpy().astype(np.float64), m.numpy(), vv.numpy(), step, 1e-3, weight_decay=0.01)
                st = opt.state[p]
                for nm, got, ref, at in (('m', st['exp_avg'], rm, 3e-8), ('v', st['exp_avg_sq'], rv, 1e-10), ('p', p.detach(), rp, 1e-7)):
                    ref = torch.from_numpy(np.asarray(ref))
                    n += check_nonfinite(f'radam step {step} grad={pname(v)} tensor {i} {nm}', got, ref,
                                         at + 2e-6 * torch.nan_to_num(ref, nan=0.0, posinf=0.0, neginf=0.0).abs())
            return n
        F.run(one)
    F.done(min_checked=3)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: hop, stack, module
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('split', [1, 2])
@pytest.mark.parametrize('batch_stats', [False, True], ids=['running', 'batch'])
@pytest.mark.parametrize('name', list(HOP_GRAPHS))
def test_hop_nonfinite(name, batch_stats, split, monkeypatch):
    """The native hop (qagnn_hop_fwd_f32) and the composed hop against the emulation under a poisoned node row of X, W1t[3][5] and one
    Ek|Em row: with a NaN every forward buffer is non-finite exactly where the emulation's is -- under batch statistics every row of y;
    with an inf, through this chain of kernels, at least where the emulation's is (check_nonfinite, `superset`)."""
    K = hip()
    case = hop_case(name)
    F = Failures()
    with (helpers.form_everywhere() if split == 2 else contextlib.nullcontext()):  # (2: the three-MFMA form, at these row counts too)
        monkeypatch.setattr(K, 'gemm_split', split)
        for site in HOP_SITES:
            for v in POISONS:
                pc = poisoned(case, site, v)
                ref = run_hops(pc, EMU, batch_stats, native=False)
                if batch_stats and v != v:
                    assert not bool(torch.isfinite(ref[0]['y']).any())
                for native in (True, False):
                    F.run(lambda: check_hops(f'{"native" if native else "composed"} hop [{site}={pname(v)}]',
                                             run_hops(pc, K, batch_stats, native, 'cuda'), ref, batch_stats, superset=v == v))
    F.done(min_checked=18)


@pytest.mark.gpu
@pytest.mark.parametrize('split', [1, 2])
@pytest.mark.parametrize('batch_stats', [False, True], ids=['running', 'batch'])
@pytest.mark.parametrize('name', list(HOP_GRAPHS))
def test_stack_nonfinite(name, batch_stats, split, monkeypatch):
    """qagnn_stack_fwd_f32 over three hops: under running statistics the non-finite rows of y are, hop by hop, exactly the rows the
    emulation gives (the poisoned node's out-neighbourhood, growing by one hop each time); under batch statistics all rows."""
    K = hip()
    case = hop_case(name, k=3)
    F = Failures()
    with (helpers.form_everywhere() if split == 2 else contextlib.nullcontext()):  # (2: the three-MFMA form, at these row counts too)
        monkeypatch.setattr(K, 'gemm_split', split)
        for site in HOP_SITES:
            pc = poisoned(case, site, NAN)
            ref = run_hops(pc, EMU, batch_stats, native=False)
            bad_rows = [int((~torch.isfinite(r['y'])).any(1).sum()) for r in ref]
            if batch_stats:
                assert bad_rows == [case['N']] * 3
            elif site == 'X_row':
                assert 0 < bad_rows[0] <= bad_rows[1] <= bad_rows[2] and bad_rows[0] < case['N'], bad_rows
            F.run(lambda: check_hops(f'native stack [{site}=nan]', run_hops(pc, K, batch_stats, True, 'cuda'), ref, batch_stats))
    F.done(min_checked=3)


@pytest.fixture
def form(request):
    yield from helpers.apply_form(request.param)


@pytest.mark.gpu
@pytest.mark.parametrize('train', [False, True], ids=['eval', 'train'])
@pytest.mark.parametrize('poison,form', helpers.with_forms(list(MODULE_POISONS)), indirect=['form'])
def test_module_nonfinite(poison, form, train):
    """QAGNN.forward / backward on the HIP path against the oracle under the three poisons (module_vs_oracle)."""
    from qagnn_amd import ops
    ops.set_kernels(None)
    bad, _ = module_vs_oracle(poison, train)
    assert ops.kernels().name == 'hip'
    assert bad == (set(range(12)) if train else MODULE_POISONS[poison])
