"""The two softmax-bearing kernel families (csrc/edge_attn.hip, csrc/pool.hip) at the segment lengths where their loops change shape and with
operands on which the softmax's max-subtraction has work to do.

The graphs (`degree_ladder`, `class_ladder`), the operand builders, the reference cache and the comparison live next to the other edge
tests in test_hip_kernels.py, which also runs the plain `randn` kind, the determinism check and the hop on the ladders.  Here:
  * `-m "not gpu"`: the ladders really hold the segment lengths, class counts and chunk lengths they were built for; the comparison
    rejects three kinds of wrong kernel on the new cases that it accepts on the old ones;
  * `-m gpu`: edge attention on the `offset` operand kind; pool attention at its row-count boundaries, both operand kinds.
"""
import pytest
import torch

from test_hip_kernels import (EDGE_OUTPUTS, EMU, LADDER_CLASS_COUNTS, LADDER_W, check_edge_outputs, edge_case, hip, print_figures,
                              run_edge_kernels)


def _degrees(e):
    return (e.rowptr_s[1:] - e.rowptr_s[:-1]), (e.rowptr_t[1:] - e.rowptr_t[:-1])


def test_the_ladders_hold_the_segments_they_were_built_for():
    """`-m "not gpu"`.  A changed seed, QAGNN_CLS_CHUNK or CLS_BLK shows here instead of the GPU cases silently covering less."""
    e = edge_case('degree_ladder', 52).e
    assert (e.N, e.E, e.Ep) == (329, 4520, 4849) and e.n_groups == 5 and e.n_chunks == 189
    deg_s, deg_t = _degrees(e)
    for side, deg in (('source', deg_s), ('target', deg_t)):
        missing = sorted(set(LADDER_W + [1]) - set(deg.tolist()))
        assert not missing, f'no {side} segment of length {missing}'
    # 43 .. 1510 was the hole between the golden graphs and rand_hub: the hub path and the second chunk run on 14 segments per side here
    assert int((deg_s > 64).sum()) == int((deg_t > 64).sum()) == sum(w > 64 for w in LADDER_W) == 14
    assert e.cls_count[torch.arange(7) * e.T * e.T].tolist() == LADDER_CLASS_COUNTS  # (one node type: type r is class r T^2)

    c = edge_case('class_ladder', 52).e
    assert (c.N, c.E, c.Ep) == (40, 577, 617) and c.n_groups == 1 and c.n_chunks == 13
    assert set(c.cls_count.tolist()) >= {0, 1, 40, 63, 64, 65, 127, 128, 129}
    assert set(c.chunk_len.tolist()) == {1, 40, 63, 64}
    # one group: a class's chunks are its count cut at 64, so 65 and 129 leave a one-edge chunk, 127 a 63-edge one, 64 and 128 none
    per_class = {k: sorted(c.chunk_len[c.chunk_cls == k * c.T * c.T].tolist()) for k in range(7)}
    assert per_class == {0: [1], 1: [63], 2: [64], 3: [1, 64], 4: [63, 64], 5: [64, 64], 6: [1, 64, 64]}


# ---- the comparison against deliberately wrong answers (all derived from the reference; nothing runs on a GPU) --------------------------------

def _answers(case, a=None, alpha=None, aggr=None):
    """What a kernel would hand back: float32 outputs; the backward from the emulation, fed the (possibly wrong) forward."""
    ref = case.ref
    a, alpha, aggr = (ref['a'] if a is None else a), (ref['alpha'] if alpha is None else alpha), (ref['aggr'] if aggr is None else aggr)
    bwd = EMU.edge_attn_bwd(case.e, case.KMQ.double(), case.EkEm.double(), case.HP, case.qs, a, alpha, case.G.double())
    return [t.float() for t in (aggr, a, alpha) + bwd]


def _softmax_without_max(case):
    """(a) float32, exp(score) / (sum exp(score) + 1e-16) with no maximum subtracted."""
    e, HP, DP = case.e, case.HP, 4 * case.HP
    s, t, c = e.src_s.long(), e.tgt_s.long(), e.cls_s.long()
    K, Q, Ek = case.KMQ[:, :DP], case.KMQ[:, 2 * DP:], case.EkEm[:, :DP]
    ex = (case.qs * (Q[s] * (K[t] + Ek[c])).view(-1, 4, HP).sum(-1)).exp()
    a = (ex / (torch.zeros(e.N, 4).index_add_(0, s, ex)[s] + 1e-16)).double()
    alpha = a * _degrees(e)[0][s].unsqueeze(1)
    M, Em = case.KMQ[:, DP:2 * DP].double(), case.EkEm[:, DP:].double()
    msg = ((M[s] + Em[c]).view(-1, 4, HP) * alpha.unsqueeze(2)).view(-1, DP)
    return _answers(case, a, alpha, torch.zeros(e.N, DP, dtype=torch.float64).index_add_(0, t, msg))


def _tail_positions(rowptr):
    """Last position of every segment of 65, 129, 193 ... entries: a chunked loop that lost its one-edge tail chunk skips exactly these."""
    deg = rowptr[1:] - rowptr[:-1]
    return (rowptr[1:][(deg > 64) & (deg % 64 == 1)] - 1).long()


def _drop_source_tails(case):
    """(b) the softmax and the aggregation without the last edge of those source segments (a = 0 there, the others renormalised)."""
    e, ref, HP, DP = case.e, case.ref, case.HP, 4 * case.HP
    s, t, c = e.src_s.long(), e.tgt_s.long(), e.cls_s.long()
    drop = torch.zeros(e.Ep, dtype=torch.bool)
    drop[_tail_positions(e.rowptr_s)] = True
    lost = torch.zeros(e.N, 4, dtype=torch.float64).index_add_(0, s[drop], ref['a'][drop])
    a = torch.where(drop.unsqueeze(1), torch.zeros_like(ref['a']), ref['a'] / (1 - lost[s]))
    alpha = a * _degrees(e)[0][s].unsqueeze(1)
    msg = (case.KMQ[:, DP:2 * DP].double()[s] + case.EkEm[:, DP:].double()[c]).view(-1, 4, HP)
    aggr = ref['aggr'] + torch.zeros_like(ref['aggr']).index_add_(0, t, ((alpha - ref['alpha']).unsqueeze(2) * msg).view(-1, DP))
    return _answers(case, a, alpha, aggr)


def _drop_target_tails(case):
    """(c) the aggregation without the last in-edge of those target segments."""
    e, ref, HP, DP = case.e, case.ref, case.HP, 4 * case.HP
    pos = e.pos_t.long()[_tail_positions(e.rowptr_t)]  # their positions in the source order, in which a / alpha are stored
    s, t, c = e.src_s.long()[pos], e.tgt_s.long()[pos], e.cls_s.long()[pos]
    msg = (case.KMQ[:, DP:2 * DP].double()[s] + case.EkEm[:, DP:].double()[c]).view(-1, 4, HP) * ref['alpha'][pos].unsqueeze(2)
    return _answers(case, aggr=ref['aggr'].clone().index_add_(0, t, -msg.view(-1, DP)))


@pytest.mark.parametrize('flaw,kind,output', [(_softmax_without_max, 'offset', 'a'), (_drop_source_tails, 'randn', 'a'),
                                              (_drop_source_tails, 'offset', 'a'), (_drop_target_tails, 'randn', 'aggr'),
                                              (_drop_target_tails, 'offset', 'aggr')],
                         ids=['no_max-offset', 'source_tail-randn', 'source_tail-offset', 'target_tail-randn', 'target_tail-offset'])
def test_the_new_cases_reject_a_wrong_kernel_the_old_ones_accept(flaw, kind, output):
    """`-m "not gpu"`.  Three wrong kernels, as answers built from the reference: the comparison of the edge tests (check_edge_outputs, the
    one the GPU tests use) accepts each on `rand_small` with `randn` operands -- what the suite ran before the ladders -- and rejects it on
    `degree_ladder`, naming the output and a segment of 65, 129 or 193 edges."""
    old = edge_case('rand_small', 28)
    check_edge_outputs(old, [old.ref[nm].float() for nm in EDGE_OUTPUTS])  # the right answer passes
    check_edge_outputs(old, flaw(old))
    new = edge_case('degree_ladder', 52, kind)
    check_edge_outputs(new, [new.ref[nm].float() for nm in EDGE_OUTPUTS])
    if flaw is _softmax_without_max:
        check_edge_outputs(edge_case('degree_ladder', 52), flaw(edge_case('degree_ladder', 52)))  # O(1) scores: nothing to see on the ladder either
    with pytest.raises(AssertionError, match=rf'\b{output}: max err') as exc:
        check_edge_outputs(new, flaw(new))
    if flaw is _softmax_without_max:
        assert 'inf' in str(exc.value)
    else:
        assert any(f'{"source" if flaw is _drop_source_tails else "target"} degree {w}' in str(exc.value) for w in (65, 129, 193)), str(exc.value)


def test_the_offset_operands_are_what_they_claim():
    """`-m "not gpu"`.  Raw scores are 128 + integer / 4 exactly, e^score is past fp32, and the softmax is not a one-hot."""
    for name, HP in (('degree_ladder', 52), ('degree_ladder', 8), ('class_ladder', 52), ('rand_hub', 52)):
        case = edge_case(name, HP, 'offset')
        e, DP = case.e, 4 * HP
        s, t, c = e.src_s.long(), e.tgt_s.long(), e.cls_s.long()
        sc = case.qs * (case.KMQ[:, 2 * DP:][s] * (case.KMQ[:, :DP][t] + case.EkEm[:, :DP][c])).view(-1, 4, HP).sum(-1)
        assert sc.dtype == torch.float32 and torch.equal(sc.double() * 4, (sc.double() * 4).round())
        assert sc.min().item() > 89 and not torch.isfinite(sc.exp()).any()
        if name != 'rand_hub':  # (its 3 008-edge segment has a = O(1e-4) at best)
            assert (case.ref['a'] < 1e-6).double().mean().item() < 1e-4


# ---- GPU: edge attention on the offset kind -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('name,HP', [('degree_ladder', 52), ('degree_ladder', 8), ('class_ladder', 52), ('class_ladder', 8), ('rand_hub', 52),
                                     ('csqa_b10', 52)])
def test_edge_attention_with_a_large_common_score_offset(name, HP):
    """Scores of 128 + integer / 4 (edge_inputs_offset): without the max-subtraction of k_edge_scores / scores_hub every exp overflows; with
    the maximum taken over the wrong slots (a padding slot of a partly filled 16-edge group, a clamped duplicate of a tail chunk) the
    result is off by factors of e^(1/4).  Same assertions as test_edge_attention_forward_backward."""
    case = edge_case(name, HP, 'offset')
    log = []
    try:
        check_edge_outputs(case, run_edge_kernels(case), log)
    finally:
        print_figures(f'edge[{name}-{HP}-offset]', log)


# ---- GPU: pool attention at its loop boundaries ----------------------------------------------------------------------------------------------

def _pool_operands(B, n, NH, Cc, kind):
    g = torch.Generator().manual_seed(B * 100 + n)
    if kind == 'randn':
        u, c, it = torch.randn(B, NH, Cc, generator=g) * 0.3, torch.randn(B, NH, generator=g), 0.2
        Kx, dz, da = torch.randn(B, n, Cc, generator=g), torch.randn(B, NH, Cc, generator=g), torch.randn(B, NH, n, generator=g)
    else:  # integers: u in -1 .. 1, the rest in -2 .. 2, c = 1024, 1 / temperature = 1/8: unmasked logits are 128 + integer / 8 exactly
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()  # noqa: E731
        u, c, it = ri(-1, 1, B, NH, Cc), torch.full((B, NH), 1024.0), 0.125
        Kx, dz, da = ri(-2, 2, B, n, Cc), ri(-2, 2, B, NH, Cc), ri(-2, 2, B, NH, n)
    lens = torch.randint(1, n + 1, (B,), generator=g)
    lens[0], lens[-1] = 1, n  # a subgraph whose only live row is row 0, and one without a masked row
    return u, c, Kx, lens, dz, da, it


def _close(nm, got, ref, emu, rtol, atol, log):
    """torch.allclose(got, ref, rtol, atol), with the figures for the record: the worst |d| / (atol + rtol |ref|) (passes at <= 1) of the
    kernel and of the float32 emulation."""
    ratio = lambda x: ((x.double() - ref).abs() / (atol + rtol * ref.abs())).max().item()  # noqa: E731
    log.append(f'{nm} {ratio(got):.2e} (f32 {ratio(emu):.2e})')
    assert torch.isfinite(got).all(), f'{nm} is not finite'
    assert torch.allclose(got.double(), ref, rtol=rtol, atol=atol), f'{nm}: {ratio(got):.3f} of the bar'


POOL_ROWS = [1, 3, 5, 31, 32, 33, 63, 64, 65, 200]  # below one wave step (4 rows), around one workgroup sweep (4 x POOL_W = 32), around the 64-lane softmax stride


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['randn', 'offset'])
@pytest.mark.parametrize('B,n,NH,Cc,p', [(6, n, 2, 208, 0.0) for n in POOL_ROWS] + [(5, n, 4, 32, 0.3) for n in (3, 33, 65)])
def test_pool_attention_at_its_loop_boundaries(B, n, NH, Cc, p, kind):
    """k_pool_fwd / k_pool_bwd against the emulation and the bars of test_pool_attention_forward_backward at the row counts where their loops
    change shape, with `randn` operands and with exact logits of 128 + integer / 8 (`offset`: wave_max has work to do)."""
    u, c, Kx, lens, dz, da, it = _pool_operands(B, n, NH, Cc, kind)
    mask = torch.arange(n).unsqueeze(0) >= lens.unsqueeze(1)
    K, seed = hip(), 12345
    label, log = f'pool[{B}-{n}-{NH}-{Cc}-{p}-{kind}]', []
    try:
        attn, attn_d, z = [t.cpu() for t in K.pool_attn_fwd(u.cuda(), c.cuda(), Kx.cuda(), mask.cuda(), it, p, seed)]
        r_attn, r_attn_d, r_z = EMU.pool_attn_fwd(u.double(), c.double(), Kx.double(), mask, it, p, seed)
        e_attn, e_attn_d, e_z = EMU.pool_attn_fwd(u, c, Kx, mask, it, p, seed)
        _close('attn', attn, r_attn, e_attn, 1e-4, 1e-6, log)
        assert ((attn_d == 0) == (r_attn_d == 0)).all(), 'dropout masks differ'
        _close('attn_d', attn_d, r_attn_d, e_attn_d, 1e-4, 1e-6, log)
        _close('z', z, r_z, e_z, 1e-4, 1e-5, log)
        assert (attn[mask.unsqueeze(1).expand_as(attn)] == 0).all()
        assert (attn.double().sum(2) - 1).abs().max().item() < 1e-5
        assert (attn[0, :, 0] == 1).all(), 'softmax over the one live row of subgraph 0 is not exactly 1'
        for tag, dattn in (('', da), ("'", None)):  # (' : without d attn)
            got = K.pool_attn_bwd(u.cuda(), Kx.cuda(), it, p, seed, attn.cuda(), attn_d.cuda(), dz.cuda(), None if dattn is None else dattn.cuda())
            ref = EMU.pool_attn_bwd(u.double(), Kx.double(), it, p, seed, r_attn, r_attn_d, dz.double(), None if dattn is None else dattn.double())
            emu = EMU.pool_attn_bwd(u, Kx, it, p, seed, e_attn, e_attn_d, dz, dattn)
            for nm, a, b_, e_ in zip(('dK', 'du', 'dc'), got, ref, emu):
                # (dc is structurally zero -- the softmax gradient sums to zero: round-off, held by the absolute term alone)
                _close(nm + tag, a.cpu(), b_, e_, 2e-4, 2e-5 * max(1.0, b_.abs().max().item()), log)
    finally:
        print(f'FIGURE {label} as fractions of the allclose bars: ' + ' | '.join(log))
