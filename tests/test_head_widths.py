"""Every kernel family at the edges of the admitted head widths: H = 4 heads, head pitch HP % 4 == 0, dh <= 64 (include/qagnn_hip.h).

The width ladder (test_hip_kernels.WIDTH_LADDER, as (HP, dh), d = 4 dh):
    (4, 3) d = 12, (4, 4) d = 16      one active lane per DPP row of the edge kernels, with and without a pad column
    (32, 32) d = 128                   no pad column: db2 and dTT by column reduction in the Python layer
    (60, 60) d = 240                   K1 % 32 == 16 with a 128-wide second segment in the projection
    (64, 63) d = 252, (64, 64) d = 256 no idle lane in the edge kernels, with one pad column and with none; DP = 256 is the last width of the
                                       GEMM prologue's LDS vectors, and where the class reduction's thread count sits on its threshold
Here:
  * `-m "not gpu"`: the comparison of the edge tests rejects two kernels that are wrong at HP = 64 only;
  * `-m gpu`: edge attention forward and backward at every width, both operand kinds, and on a graph with E' >= 65 536 (the 1024-thread
    class reduction); one hop per width against the float64 composition of the emulation; widths outside the range are refused before
    anything is launched.
The GEMM shapes, the fused-hop identity, the three-MFMA hop, the pooling head and the module parity of these widths extend the
parametrisations of test_hip_kernels.py, test_hip_parity.py and test_host_logic_emu.py.
"""
import ctypes as C

import pytest
import torch

from emu_kernels import EmuGraph
from test_attention_edges import _answers
import test_hip_kernels
from test_hip_kernels import (EDGE_BARS, EDGE_OUTPUTS, EMU, WIDTH_LADDER, check_edge_outputs, edge_case, edge_inputs, hip, print_figures,
                              run_edge_kernels, side_width)
from test_nonfinite import FWD, _prm

WIDTH_IDS = [f'{HP}x{dh}' for HP, dh in WIDTH_LADDER]


# ---- CPU: the comparison against two kernels that are wrong at HP = 64 only (answers built from the reference) -------------------------------

def _score_without_the_last_float4(case):
    """(a) the score's dot product without the last float4 of every head (columns HP - 4 .. HP - 1): a lane map that stops one lane early."""
    HP, DP = case.HP, 4 * case.HP
    KMQ = case.KMQ.double().clone()
    KMQ[:, 2 * DP:].view(-1, 4, HP)[:, :, HP - 4:] = 0  # (Q of those columns: they drop out of the score; M is untouched)
    aggr, a, alpha = EMU.edge_attn_fwd(case.e, KMQ, case.EkEm.double(), HP, case.qs)
    return _answers(case, a, alpha, aggr)


def _dEkEm_without_lane_15(case):
    """(b) the right answer with columns 60 .. 63 of every head of dEk and dEm left as allocated (zero): lane 16 head + 15 of the class pass
    never stores.  At HP < 64 that lane is idle and the answer is the reference's."""
    got = [case.ref[nm].float() for nm in EDGE_OUTPUTS]
    HP = case.HP
    if HP > 60:
        got[4] = got[4].clone()
        got[4].view(-1, 8, HP)[:, :, 60:] = 0
    return got


def _currently_parametrised_pitches():
    (mark,) = [m for m in test_hip_kernels.test_edge_attention_forward_backward.pytestmark if m.name == 'parametrize']
    return mark.args[1]


def test_the_width_cases_reject_a_kernel_wrong_at_the_last_lane():
    """`-m "not gpu"`.  check_edge_outputs (the comparison the GPU tests use) on two wrong kernels, as answers built from the reference.
    (b) is accepted by every case the suite ran before the width ladder: none has a sixteenth lane (asserted on the full list of their
    pitches), so the flaw changes no element of any of them; that identity and the comparison are run on the small cached cases, not on
    the 400 000-edge graphs, for which it holds by the same construction.  (b) is rejected at both HP = 64 widths.  (a) is rejected at HP = 64 too; it ALREADY fails the old cases (at HP = 28 the last float4 holds
    the live column 24, at HP = 52 the live columns 48 and 49): kept, as the statement that a lane map one lane short never passed."""
    old_pitches = _currently_parametrised_pitches()
    assert len(old_pitches) >= 14 and all(HP < 64 for _, HP in old_pitches)
    for name, HP in [(n, p) for n, p in old_pitches if n in ('degree_ladder', 'class_ladder', 'rand_small')]:
        old = edge_case(name, HP)
        answer = _dEkEm_without_lane_15(old)
        assert all(torch.equal(x, old.ref[nm].float()) for nm, x in zip(EDGE_OUTPUTS, answer))
        check_edge_outputs(old, answer)
    for HP, dh in ((64, 63), (64, 64)):
        for kind in ('randn', 'offset'):
            new = edge_case('class_ladder', HP, kind, dh)
            check_edge_outputs(new, [new.ref[nm].float() for nm in EDGE_OUTPUTS])  # the right answer passes
            with pytest.raises(AssertionError, match=r'\bdEkEm: max err'):
                check_edge_outputs(new, _dEkEm_without_lane_15(new))
            with pytest.raises(AssertionError, match=r'\ba: max err'):
                check_edge_outputs(new, _score_without_the_last_float4(new))
    old = edge_case('rand_small', 28)
    with pytest.raises(AssertionError, match=r'\ba: max err'):  # (a) on what the suite ran before the ladders
        check_edge_outputs(old, _score_without_the_last_float4(old))


def test_the_ladder_bars_come_from_the_emulation():
    """`-m "not gpu"`.  Every width case carries the float32 yardstick, and its bars are max(fixed bar, 4 x yardstick) -- at dh == HP the pad
    mask is empty and check_edge_outputs still runs through."""
    for (HP, dh) in WIDTH_LADDER:
        case = edge_case('class_ladder', HP, 'randn', dh)
        assert case.dh == dh and set(case.emu32) == set(EDGE_OUTPUTS)
        assert case.bars == {nm: max(EDGE_BARS[nm], 4 * case.emu32[nm]) for nm in EDGE_OUTPUTS}
        assert max(case.emu32.values()) < 5e-6, case.emu32  # (the float32 emulation itself stays at round-off at every width)
        check_edge_outputs(case, [case.ref[nm].float() for nm in EDGE_OUTPUTS])


# ---- GPU: edge attention per width ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['randn', 'offset'])
@pytest.mark.parametrize('name', ['degree_ladder', 'class_ladder', 'rand_hub'])
@pytest.mark.parametrize('HP,dh', WIDTH_LADDER, ids=WIDTH_IDS)
def test_edge_attention_per_width(HP, dh, name, kind):
    """k_edge_* of csrc/edge_attn.hip at every width of the ladder, on the segment-length and class-count ladders and the hub graph, with
    O(1) scores and with scores of 128 + integer / 4: the assertions of test_edge_attention_forward_backward, bars by the ladders' rule."""
    case = edge_case(name, HP, kind, dh)
    log = []
    try:
        check_edge_outputs(case, run_edge_kernels(case), log)
    finally:
        print_figures(f'edge[{name}-{HP}x{dh}-{kind}]', log)


@pytest.mark.gpu
@pytest.mark.parametrize('HP,dh', [(64, 64), (4, 4)], ids=['64x64', '4x4'])
def test_edge_attention_with_the_wide_class_reduction(HP, dh):
    """E' = 66 000 >= 65 536: k_cls_reduce runs with 1024 threads (P = 8 row slices at HP = 64, 128 at HP = 4)."""
    case = edge_case('rand_64k', HP, 'randn', dh)
    assert case.e.Ep >= 65536
    log = []
    try:
        check_edge_outputs(case, run_edge_kernels(case), log)
    finally:
        print_figures(f'edge[rand_64k-{HP}x{dh}-randn]', log)


# ---- GPU: one hop per width against float64 --------------------------------------------------------------------------------------------------

HOP_TENSORS = ('y', 'KMQ', 'a|alpha', 'aggr', 'h1', 'out', 'mean', 'var', 'invstd', 'scale', 'shift', 'dX', 'dS', 'dWx_t', 'dWs_t', 'dTT', 'dEkEm', 'dW1t', 'db1', 'dgamma',
               'dbeta', 'dW2t', 'db2')


def _hop_operands(HP, dh):
    """the construction of test_nonfinite.hop_case on degree_ladder at the width (HP, dh), with beta = 9 +- 1 as in
    test_hip_kernels._native_hop_vs_exact: the BatchNorm outputs are positive but for a few dozen outliers of the hub rows, and those sit
    far from zero (asserted on the reference), so no ReLU kink is in play"""
    (ei, et, nt, R, T), _, _, _, qs = edge_inputs('degree_ladder', HP, 5, dh)
    gen = torch.Generator().manual_seed(77)
    N, DP, Cn, SP = nt.numel(), 4 * HP, R * T * T + T, side_width(HP)
    rnd = lambda *shape, s=0.3: torch.randn(*shape, generator=gen) * s  # noqa: E731
    Wx_t, Ws_t, W1t, W2t = rnd(DP, 3 * DP, s=0.1), rnd(SP, 3 * DP, s=0.1), rnd(DP, DP, s=0.1), rnd(DP, DP, s=0.1)
    prm = [Wx_t, None, Ws_t, None, rnd(T, 3 * DP), rnd(Cn, 2 * DP), W1t, None, rnd(DP), 1 + rnd(DP), 9 + rnd(DP), W2t, None, rnd(DP),
           rnd(DP), 0.5 + rnd(DP).abs()]
    return (ei, et, nt, R, T), qs, prm, rnd(N, DP, s=1.0), rnd(N, SP, s=1.0), rnd(N, DP, s=1.0)


def _run_hop(fwd, bwd, g, HP, qs, X, S, ntype, prm, dy):
    args = (g, HP, qs, X, S, ntype, prm, True, 1e-5, 0.0, 0, True)
    y, saved = fwd(*args, None)
    grads = bwd(*args, saved, dy, True, True)
    return [y] + list(saved[:5]) + list(saved[5][:5]) + list(grads)  # (the five rows of stats each against its own maximum)


@pytest.mark.gpu
@pytest.mark.parametrize('HP,dh', WIDTH_LADDER, ids=WIDTH_IDS)
def test_native_hop_against_float64_per_width(HP, dh, monkeypatch):
    """qagnn_hop_{fwd,bwd}_f32 with the exact products (gemm_split = 1) on degree_ladder, train mode, p = 0, against ops.hop_*_composed on
    the emulation in float64.  Bar per tensor, as a fraction of the float64 tensor's maximum: 4 x the error of the SAME composition on the
    emulation in float32 (4: the kernels' other summation order, as in the edge ladders), floored at the fixed forward bar of
    test_nonfinite.py (FWD: atol + rtol x maximum).  The gradients have no fixed bar there: they take the same floor.  db1 is zero by
    construction under batch statistics (BatchNorm's backward removes the mean): held against the size of dW1t, which sums the same rows.
    test_fused_hop_equals_composed_path compares two GPU paths bit for bit: a kernel wrong at a width passes it and fails here."""
    from qagnn_amd import ops
    (ei, et, nt, R, T), qs, prm, X, S, dy = _hop_operands(HP, dh)
    e = EmuGraph(ei, et, nt, R, T)
    comp = lambda conv: _run_hop(lambda *a: ops.hop_fwd_composed(EMU, *a), lambda *a: ops.hop_bwd_composed(EMU, *a), e, HP, qs, conv(X),  # noqa: E731
                                 conv(S), nt, _prm(prm, conv), conv(dy))
    ref, emu = comp(lambda t: t.double()), comp(lambda t: t.float())
    pre = ref[4] * ref[9] + ref[10]  # relu's input, bn(h1): no element within 1e-4 of the largest of the kink (round-off is 1e-6)
    assert pre.abs().min().item() > 1e-4 * pre.abs().max().item() and (pre > 0).double().mean().item() > 0.999
    K = hip()
    monkeypatch.setattr(K, 'gemm_split', 1)
    cu = lambda t: t.cuda()  # noqa: E731
    g = K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R, T)
    got = _run_hop(K.hop_fwd, K.hop_bwd, g, HP, qs, cu(X), cu(S), nt.cuda(), _prm(prm, cu), cu(dy))
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
    print_figures(f'hop[degree_ladder-{HP}x{dh}]', log)
    assert not failures, '; '.join(failures)


# ---- GPU: widths outside the range are refused before anything is launched --------------------------------------------------------------------

CANARY = -7.5
EUNSUPPORTED, EINVAL = 2, 1


def _canary(*shape):
    return torch.full(shape, CANARY, device='cuda')


@pytest.mark.gpu
@pytest.mark.parametrize('HP', [68, 6])
def test_edge_attention_refuses_a_pitch_outside_the_range(HP):
    """qagnn_edge_attn_{fwd,bwd}_f32 at HP = 68 (> 64) and HP = 6 (no multiple of 4): QAGNN_EUNSUPPORTED, and no output or scratch element
    is written."""
    K = hip()
    ei, et, nt, R, T = (t if isinstance(t, int) else t.cuda() for t in edge_case('rand_small', 28).graph)
    g = K.graph_prep(ei, et, nt, R, T)
    DP = 4 * HP
    gen = torch.Generator().manual_seed(HP)
    KMQ, EkEm, G = (torch.randn(r, c, generator=gen).cuda() for r, c in ((g.N, 3 * DP), (g.C, 2 * DP), (g.N, DP)))
    score, a, alpha, aggr = _canary(g.Ep, 4), _canary(g.Ep, 4), _canary(g.Ep, 4), _canary(g.N, DP)
    rc = K.lib.qagnn_edge_attn_fwd_f32(C.byref(g.c), KMQ.data_ptr(), 3 * DP, EkEm.data_ptr(), 2 * DP, HP, 0.25, score.data_ptr(), a.data_ptr(),
                                       alpha.data_ptr(), aggr.data_ptr(), DP, K._stream())
    torch.cuda.synchronize()
    assert rc == EUNSUPPORTED, (rc, K.lib.qagnn_last_error().decode())
    assert all(bool((t == CANARY).all()) for t in (score, a, alpha, aggr)), 'the refused forward wrote to an output'
    with pytest.raises(RuntimeError, match=r'\(code 2\)'):  # ... and through the binding
        K.edge_attn_fwd(g, KMQ, EkEm, HP, 0.25)
    a_in, alpha_in = torch.rand(g.Ep, 4).cuda(), torch.rand(g.Ep, 4).cuda()
    outs = [_canary(g.N, 3 * DP), _canary(g.C, 2 * DP), _canary(g.Ep, 4), _canary(g.N, 4), _canary(g.cls_part_rows, 2 * DP)]
    rc = K.lib.qagnn_edge_attn_bwd_f32(C.byref(g.c), KMQ.data_ptr(), 3 * DP, EkEm.data_ptr(), 2 * DP, HP, 0.25, a_in.data_ptr(), alpha_in.data_ptr(),
                                       G.data_ptr(), DP, *[t.data_ptr() for t in outs], K._stream())
    torch.cuda.synchronize()
    assert rc == EUNSUPPORTED, (rc, K.lib.qagnn_last_error().decode())
    assert all(bool((t == CANARY).all()) for t in outs), 'the refused backward wrote to an output'


def _canaried_hop(K, g, nt, HP, backward, T=4, canary=CANARY, amax_word=123):
    """a complete qagnn_hop_args at pitch HP (and a node-type table of T rows) on graph g whose every output, saved buffer and workspace
    holds the canary (the maximum words: amax_word) -> (struct, the canaried tensors, everything that must stay alive)"""
    from qagnn_amd import _lib
    _canary = lambda *shape: torch.full(shape, canary, device='cuda')  # noqa: E731
    DP, SP = 4 * HP, -(-2 * HP // 16) * 16
    gen = torch.Generator().manual_seed(HP)
    rnd = lambda *shape: (torch.randn(*shape, generator=gen) * 0.1).cuda()  # noqa: E731
    Wx_t, Ws_t, W1t, W2t = rnd(DP, 3 * DP), rnd(SP, 3 * DP), rnd(DP, DP), rnd(DP, DP)
    prm = (Wx_t, Wx_t.t().contiguous(), Ws_t, Ws_t.t().contiguous(), rnd(T, 3 * DP), rnd(g.C, 2 * DP), W1t, W1t.t().contiguous(), rnd(DP),
           1 + rnd(DP), rnd(DP), W2t, W2t.t().contiguous(), rnd(DP), rnd(DP), 0.5 + rnd(DP).abs())
    X, S, dy = rnd(g.N, DP), rnd(g.N, SP), rnd(g.N, DP)
    h = K._hop_struct(g, HP, 0.25, X, S, nt, prm, True, 1e-5, 0.0, 0, True)
    guarded = [_canary(g.N, 3 * DP), _canary(2, g.Ep, 4), _canary(4, g.N, DP), _canary(5, DP)]
    amax = torch.full((_lib.HOP_AMAX_WORDS,), amax_word, dtype=torch.int32, device='cuda')
    K._set_saved(h, *[t.data_ptr() for t in guarded], amax.data_ptr(), g.Ep, g.N * DP * 4)
    if backward:
        sizes, offs = K._grad_sizes(DP, SP, T, g.C)
        flat, dX, dS = _canary(offs[-1]), _canary(g.N, DP), _canary(g.N, SP)
        K._carve_grads(h, flat, sizes, offs, g.C)
        h.dy, h.dX, h.dS = dy.data_ptr(), dX.data_ptr(), dS.data_ptr()
        ws = _canary(int(K.lib.qagnn_hop_bwd_workspace_elems(g.N, g.Ep, DP, SP, g.cls_part_rows)))
        guarded += [flat, dX, dS]
    else:
        ws = _canary(int(K.lib.qagnn_hop_fwd_workspace_elems(g.N, g.Ep, DP)))
    h.ws, h.ws_elems = ws.data_ptr(), ws.numel()
    return h, guarded + [ws], (prm, X, S, dy, amax)


@pytest.mark.gpu
@pytest.mark.parametrize('entry', ['hop_fwd', 'stack_fwd', 'hop_bwd', 'stack_bwd'])
def test_hop_refuses_a_pitch_outside_the_range(entry):
    """qagnn_{hop,stack}_{fwd,bwd}_f32 with a hop at HP = 68 (DP = 272, a multiple of 16: nothing else about the shape is wrong): refused by
    check_hop before anything is enqueued -- every saved buffer, gradient and workspace element keeps its canary.  Before check_hop bounded
    HP the projection GEMM wrote KMQ and only the edge kernels' launcher refused.  The stacks hold a second, valid hop (HP = 16) that would
    run first -- hop 0 of the forward, hop 1 of the backward: all hops are validated before the first one is enqueued, so it must not."""
    from qagnn_amd import _lib
    K = hip()
    ei, et, nt, R, T = edge_case('rand_small', 28).graph
    g, nt = K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R, T), nt.cuda()
    backward, stack = entry.endswith('bwd'), entry.startswith('stack')
    bad = _canaried_hop(K, g, nt, 68, backward)
    good = _canaried_hop(K, g, nt, 16, backward) if stack else None
    order = [bad] if not stack else ([bad, good] if backward else [good, bad])
    hops = (_lib.qagnn_hop_args * len(order))(*[o[0] for o in order])
    fn = getattr(K.lib, f'qagnn_{entry}_f32')
    rc = fn(hops, len(order), K._stream()) if stack else fn(C.byref(hops[0]), K._stream())
    torch.cuda.synchronize()
    assert rc in (EUNSUPPORTED, EINVAL), (rc, K.lib.qagnn_last_error().decode())
    for h, guarded, keep in order:
        assert all(bool((t == CANARY).all()) for t in guarded), f'{entry}: a refused call wrote to a buffer'
        assert bool((keep[4] == 123).all())
