"""The native training losses: include/qagnn_hip_loss.h, ops.choice_loss / ops.ChoiceLossFn, qagnn_amd.losses, GraphedStep(loss=...).

The yardstick everywhere is torch in float64 on the fp32 inputs: F.cross_entropy, and nn.MarginRankingLoss applied per question to
(x[q][label].expand(nc - 1), x[q][others]) and averaged; margin = float(np.float32(margin)).  A row whose label lies outside [0, nc) has
its term set to zero, the denominators stay.  Loss and gradient are held to the bound the header states (_lib.choice_loss_bound).

  * `-m "not gpu"`: the header against the bindings, the built library and the build hash; the kernel's thread count read from the source;
    the plain-torch fallback and the emulation provider against the yardstick; the comparison helper rejects five wrong answers; the
    bound is not vacuous; unknown loss names.
  * `-m gpu`: the kernel through the C ABI on the ladder of (Q, nc), both kinds, four logit regimes, the exact kink, determinism and the
    meter, pitched operands and refused arguments, non-finite logits, labels out of range, autograd, the eager training step with the
    native loss against the torch loss, GraphedStep(loss=...) against the eager step.
"""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers
from emu_loss import EmuLossKernels
from qagnn_amd import _lib, graphed, losses, ops

KINDS = ('cross_entropy', 'margin_rank')
LOG = os.environ.get('QAGNN_LOSS_TEST_LOG')  # file that collects the measured figures of the GPU tests
W037 = float(np.float32(0.37))


def note(line):
    print(line)
    if LOG:
        with open(LOG, 'a') as f:
            f.write(line + '\n')


@contextlib.contextmanager
def provider(K):
    old = ops.set_kernels(K)
    try:
        yield K
    finally:
        ops.set_kernels(old)


def hip():
    ops.set_kernels(None)
    return ops.kernels()


# ---- the constants, read from the sources -------------------------------------------------------------------------------------------------
def _source(*path):
    with open(os.path.join(helpers.ROOT, *path)) as f:
        return f.read()


def _kernel_constants():
    """(T, nc boundaries): the thread count of k_choice_loss, and every nc at which the DEVICE code changes form -- comparisons of nc with
    a literal inside namespace qagnn (the host checks of the admitted range live behind it)"""
    src = _source('qagnn_amd', 'csrc', 'loss.hip')
    t = set(re.findall(r'constexpr int CL_THREADS = (\d+);', src))
    device = src.split('}  // namespace qagnn')[0]
    bounds = sorted({int(v) for v in re.findall(r'\bnc\s*(?:<=|>=|<|>|==)\s*(\d+)', device)})
    return (int(t.pop()) if len(t) == 1 else None), bounds


T, NC_BOUNDS = _kernel_constants()
Q_LADDER = [1, 2, 3, T - 1, T, T + 1, 4 * T + 3] if T else []
NC_LADDER = sorted({2, 4, 5, 8, 1024} | {b + d for b in NC_BOUNDS for d in (-1, 0, 1) if 2 <= b + d <= 1024})
PARITY_CASES = [('cross_entropy', 1)] + [(k, nc) for k in KINDS for nc in NC_LADDER]


# ---- the yardstick and the comparison helper ----------------------------------------------------------------------------------------------
def yardstick(x, labels, kind, margin=0.1, weight=1.0):
    """-> (loss, d loss / d x) in float64 from torch's own loss modules; x fp32 [Q, nc] (CPU), labels int64 [Q]"""
    Q, nc = x.shape
    xd = x.detach().cpu().double().clone().requires_grad_(True)
    lab = labels.cpu()
    valid = (lab >= 0) & (lab < nc)
    if kind == 'cross_entropy':
        rows = F.cross_entropy(xd, lab.clamp(0, nc - 1), reduction='none')
        loss = torch.where(valid, rows, torch.zeros_like(rows)).sum() / Q
    else:
        crit = torch.nn.MarginRankingLoss(margin=float(np.float32(margin)), reduction='mean')
        ones = torch.ones(nc - 1, dtype=torch.float64)
        terms = []
        for q in range(Q):
            l = int(lab[q])
            if not valid[q]:
                terms.append(xd.new_zeros(()))
                continue
            others = torch.cat([torch.arange(l), torch.arange(l + 1, nc)])
            terms.append(crit(xd[q, l].expand(nc - 1), xd[q, others], ones))
        loss = torch.stack(terms).sum() / Q
    loss = loss * weight
    loss.backward()
    return loss.detach(), xd.grad


def finite_max(x):
    f = x[torch.isfinite(x)]
    return float(f.abs().max()) if f.numel() else 0.0


def compare(loss, g, ref_loss, ref_g, kind, x, margin, weight, what, rows=None):
    """Hold (loss, g) to the yardstick under the header's bound.  rows: the gradient rows to compare (default: all).  Non-finite yardstick
    losses must be met exactly (NaN by NaN, inf by the same inf).  -> (loss error / bound, gradient error / bound)"""
    Q, nc = x.shape
    lb, gb = _lib.choice_loss_bound(kind, nc, Q, finite_max(x), margin, weight)
    loss, ref_loss = float(loss), float(ref_loss)
    if np.isfinite(ref_loss):
        le = abs(loss - ref_loss)
        assert le <= lb, f'{what}: loss {loss!r} vs {ref_loss!r}: |d| = {le:.3e} > bound {lb:.3e}'
    else:
        le = 0.0
        assert (np.isnan(loss) and np.isnan(ref_loss)) or loss == ref_loss, f'{what}: loss {loss!r} where float64 torch gives {ref_loss!r}'
    gd, rg = g.detach().cpu().double(), ref_g
    if rows is not None:
        gd, rg = gd[rows], rg[rows]
    err = (gd - rg).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err)
    ge = float(err.max()) if err.numel() else 0.0
    assert ge <= gb, f'{what}: gradient |d| = {ge:.3e} > bound {gb:.3e} (of |w| / Q: {ge * Q / max(abs(weight), 1e-300):.3e})'
    return le / lb, ge / gb


def make_logits(regime, Q, nc, seed, kind):
    """N(0, 1) | x30 (a saturated softmax) | + 1e4 (shift invariance) | all equal.  Margin-rank inputs lie on multiples of 1 / 8: with margin
    0.1 a hinge argument 0.1 + k / 8 is never within 0.025 of zero, so no pair's activity hangs on a rounding."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(Q, nc, generator=gen)
    if regime == 'x30':
        x = x * 30
    if regime == 'equal':
        x = torch.full((Q, nc), 0.75)
    if kind == 'margin_rank':
        x = torch.round(x * 8) / 8
    if regime == 'shift':
        x = x + 1e4
    labels = torch.randint(0, nc, (Q,), generator=gen)
    return x.float(), labels


REGIMES = ('normal', 'x30', 'shift', 'equal')


def kink_case():
    """margin 0.5, logits on multiples of 1 / 4 (everything exactly representable): many pairs have a hinge argument of exactly 0"""
    gen = torch.Generator().manual_seed(77)
    Q, nc = 37, 5
    x = torch.randint(-2, 3, (Q, nc), generator=gen).float() / 4
    labels = torch.randint(0, nc, (Q,), generator=gen)
    xl = x.gather(1, labels.unsqueeze(1))
    on_kink = ((0.5 - xl + x) == 0) & (torch.arange(nc).unsqueeze(0) != labels.unsqueeze(1))
    assert int(on_kink.sum()) >= 10
    return x, labels, on_kink


# =================================================================================================================================
# Without a GPU
# =================================================================================================================================
def test_loss_header_bindings_and_build_hash():
    """qagnn_hip_loss.h declares exactly EXPORTS_LOSS; the built library exports them; the build hash covers the header and loss.hip; the
    ABI number and the other export lists are where they were, and no name is in two lists."""
    from qagnn_amd import build as B
    hdr = _source('include', 'qagnn_hip_loss.h')
    declared = sorted(set(re.findall(r'^int (qagnn_[a-z0-9_]+)\(', hdr, flags=re.M)))
    assert declared == sorted(_lib.EXPORTS_LOSS) and len(declared) == 3
    B.build(verbose=False)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f'{name} declared in qagnn_hip_loss.h but not exported'
    lib = _lib.load_library()  # prototypes resolve
    assert lib.qagnn_loss_version() == 1
    hashed = {os.path.realpath(p) for p in B.hashed_files()}
    assert os.path.realpath(os.path.join(helpers.ROOT, 'include', 'qagnn_hip_loss.h')) in hashed
    assert os.path.realpath(os.path.join(B.CSRC, 'loss.hip')) in hashed and 'loss.hip' in B.SOURCES
    assert _lib.ABI_VERSION == 25 and len(_lib.EXPORTS) == 63 and len(_lib.EXPORTS_INFER) == 5
    lists = [_lib.EXPORTS, _lib.EXPORTS_TN, _lib.EXPORTS_INFER, _lib.EXPORTS_LOSS]
    assert sum(len(set(e)) for e in lists) == len(set().union(*lists))
    kinds = dict(re.findall(r'#define QAGNN_LOSS_(CROSS_ENTROPY|MARGIN_RANK) (\d+)', hdr))
    assert {k.lower(): int(v) for k, v in kinds.items()} == _lib.LOSS_KINDS and tuple(_lib.LOSS_KINDS) == ops.LOSS_KINDS == losses.LOSSES


def test_the_ladders_follow_the_kernel_constants():
    """the thread count the Q ladder rests on is in the source, equals the header's and the binding's; the device code compares nc with no
    literal, i.e. has one form for every nc (a new form adds its boundary to NC_LADDER through NC_BOUNDS -- and fails here until this
    test names it)"""
    hdr_t = re.findall(r'#define QAGNN_LOSS_THREADS (\d+)', _source('include', 'qagnn_hip_loss.h'))
    assert T is not None and [str(T)] == hdr_t and T == _lib.LOSS_THREADS
    assert NC_BOUNDS == []
    assert Q_LADDER == [1, 2, 3, 255, 256, 257, 1027] and NC_LADDER == [2, 4, 5, 8, 1024]


@pytest.mark.parametrize('kind', KINDS)
def test_fallback_and_emulation_equal_the_yardstick(kind):
    """CPU: ops.choice_loss through the plain-torch formulation (float64: to rounding; fp32: the header's bound plus torch's own fp32 sum
    over the rows, Q u of the loss's magnitude) and through the emulation provider (the header's bound), loss and autograd gradient;
    a bad label's row contributes nothing in both; the meter's doubles."""
    for Q, nc, bad in [(1, 2, False), (7, 5, False), (7, 5, True), (300, 4, False)]:
        x, labels = make_logits('normal', Q, nc, 100 + Q, kind)
        if bad:
            labels[2], labels[5] = -1, nc
        for w in (None, W037):
            wv = 1.0 if w is None else w
            ref_loss, ref_g = yardstick(x, labels, kind, 0.1, wv)
            # float64 through the fallback
            xd = x.double().requires_grad_(True)
            with provider(None):
                loss = ops.choice_loss(xd, labels, kind, 0.1, w)
            (loss * 3).backward()
            assert abs(float(loss.detach()) - float(ref_loss)) <= 1e-12 * max(1.0, abs(float(ref_loss))), (Q, nc, w)
            assert float((xd.grad - 3 * ref_g).abs().max()) <= 1e-12
            # fp32 through the fallback
            xf = x.clone().requires_grad_(True)
            stats = torch.zeros(2, dtype=torch.float64)
            with provider(None):
                loss = ops.choice_loss(xf, labels, kind, 0.1, w, stats)
            loss.backward()
            lb, gb = _lib.choice_loss_bound(kind, nc, Q, finite_max(x), 0.1, wv)
            slack = Q * 2.0 ** -24 * wv * (2 * max(1.0, finite_max(x)) + np.log(nc) + 0.1)
            assert abs(float(loss.detach()) - float(ref_loss)) <= lb + slack
            assert float((xf.grad.double() - ref_g).abs().max()) <= gb + 4 * 2.0 ** -24 * wv / Q
            assert stats.tolist() == [float(loss.detach().float()), 1.0]
            # the emulation provider: ChoiceLossFn on the CPU
            K = EmuLossKernels()
            xe = x.clone().requires_grad_(True)
            stats = torch.zeros(2, dtype=torch.float64)
            with provider(K):
                loss = ops.choice_loss(xe, labels, kind, 0.1, w, stats)
                assert loss.dim() == 0 and loss.grad_fn is not None and type(loss.grad_fn).__name__.startswith('ChoiceLossFn')
                g = K.choice_loss(x, labels, kind, 0.1, None if w is None else torch.tensor([w]))[1]
                (loss * 3).backward()
            compare(loss.detach(), g, ref_loss, ref_g, kind, x, 0.1, wv, f'emulation Q={Q} nc={nc} w={w}')
            assert torch.equal(xe.grad, g * 3)
            assert stats.tolist() == [float(loss.detach()), 1.0] and K.bad_labels == (4 if bad else 0)


def test_compare_rejects_wrong_answers():
    """the helper the GPU cases call accepts the float64 answer rounded to fp32 and rejects: a mean over Q nc instead of Q (nc - 1); the
    label's own pair counted; a strict > at the kink; a gradient without the weight; a bad-label row that changes the denominator"""
    Q, nc, m = 12, 5, 0.1
    x, labels = make_logits('normal', Q, nc, 5, 'margin_rank')
    for kind in KINDS:
        ref = yardstick(x, labels, kind, m, W037)
        compare(ref[0].float(), ref[1].float(), *ref, kind, x, m, W037, 'the yardstick rounded')
        with pytest.raises(AssertionError, match='gradient'):  # a gradient without the weight
            compare(ref[0].float(), (ref[1] / W037).float(), *ref, kind, x, m, W037, 'unweighted gradient')
        lab_bad = labels.clone()
        lab_bad[3] = nc
        ref_bad = yardstick(x, lab_bad, kind, m, W037)
        assert float(ref_bad[1][3].abs().max()) == 0.0
        compare(ref_bad[0].float(), ref_bad[1].float(), *ref_bad, kind, x, m, W037, 'bad label, the yardstick rounded')
        with pytest.raises(AssertionError, match='loss'):  # the bad row taken out of the denominator
            compare(ref_bad[0] * Q / (Q - 1), ref_bad[1], *ref_bad, kind, x, m, W037, 'denominator Q - 1')
    ref = yardstick(x, labels, 'margin_rank', m, W037)
    with pytest.raises(AssertionError, match='loss'):
        compare(ref[0] * (nc - 1) / nc, ref[1], *ref, 'margin_rank', x, m, W037, 'mean over Q nc')
    with pytest.raises(AssertionError, match='loss'):  # the label's own pair: max(0, margin) more per question
        compare(ref[0] + W037 * float(np.float32(m)) / (nc - 1), ref[1], *ref, 'margin_rank', x, m, W037, 'own pair counted')
    xk, lk, on_kink = kink_case()
    ref = yardstick(xk, lk, 'margin_rank', 0.5, W037)
    scale = W037 / (xk.size(0) * (nc - 1))
    assert torch.allclose(ref[1][on_kink], torch.full((int(on_kink.sum()),), scale, dtype=torch.float64), rtol=1e-12)  # torch: active on the kink
    compare(ref[0].float(), ref[1].float(), *ref, 'margin_rank', xk, 0.5, W037, 'kink, the yardstick rounded')
    strict = ref[1].clone()
    strict[on_kink] = 0.0
    strict[torch.arange(xk.size(0)), lk] += on_kink.sum(1) * scale
    with pytest.raises(AssertionError, match='gradient'):
        compare(ref[0], strict, *ref, 'margin_rank', xk, 0.5, W037, 'strict > at the kink')


def test_the_bound_is_not_vacuous():
    """the header's bound at Q = 1000, nc = 5, |x| <= 4 is below 1e-5 (a condition on the bound, not a measurement), for both kinds; the
    gradient bound stays below 2e-6 of |w| / Q"""
    for kind in KINDS:
        lb, gb = _lib.choice_loss_bound(kind, 5, 1000, 4.0, 0.1, 1.0)
        assert 0 < lb < 1e-5 and 0 < gb * 1000 < 2e-6, (kind, lb, gb)
    hdr = _source('include', 'qagnn_hip_loss.h')
    for piece in ('u (nc + 8 + 5 L) + v S (2 + L)', 'u (nc + 8 + L)', '(3 u + v S) (2 + |margin| / M)', '2 u'):
        assert piece in hdr, f'the bound evaluated by _lib.choice_loss_bound is not the one the header states: {piece!r}'


def test_unknown_loss_names_raise():
    x, labels = torch.zeros(2, 5), torch.zeros(2, dtype=torch.long)
    with pytest.raises(ValueError):
        losses.compute_loss(x, labels, loss='foo')
    with pytest.raises(ValueError):
        ops.choice_loss(x, labels, 'foo')
    with pytest.raises(ValueError):
        graphed.GraphedStep(None, 5, loss='foo')  # (before the model or a device is looked at)


def test_compute_loss_and_meter_on_the_cpu():
    """compute_loss casts to fp32 (the reference's autocast logits are fp16 / bf16), takes a float weight, feeds a LossMeter"""
    x, labels = make_logits('normal', 6, 5, 9, 'cross_entropy')
    meter = losses.LossMeter('cpu')
    with provider(None):
        want = [losses.compute_loss(x.bfloat16().float(), labels, k, 0.1, 0.25) for k in KINDS]
        got = [losses.compute_loss(x.bfloat16(), labels, k, 0.1, 0.25, meter) for k in KINDS]
    assert all(g.dtype == torch.float32 and torch.equal(g, w) for g, w in zip(got, want))
    assert meter.read() == (float(got[0].double() + got[1].double()), 2)
    meter.reset()
    assert meter.read() == (0.0, 0)
    assert ops._weight_word(0.25, x.device) is ops._weight_word(0.25, x.device)  # the word of a float weight is made once


# =================================================================================================================================
# On the GPU
# =================================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize('kind,nc', PARITY_CASES)
def test_kernel_parity_through_the_c_abi(kind, nc):
    """every Q of the ladder x {weight word 0.37, NULL} x four logit regimes: loss and g within the header's bound of float64 torch"""
    K = hip()
    wword = torch.tensor([0.37], device='cuda')
    worst = [0.0, 0.0]
    for Q in Q_LADDER:
        for regime in REGIMES:
            x, labels = make_logits(regime, Q, nc, 1000 * nc + Q, kind)
            ref_loss, ref_g = yardstick(x, labels, kind, 0.1, 1.0)
            xg, lg = x.cuda(), labels.cuda()
            for w, word in ((W037, wword), (1.0, None)):
                loss, g = K.choice_loss(xg, lg, kind, 0.1, word)
                r = compare(loss.item(), g, ref_loss * w, ref_g * w, kind, x, 0.1, w, f'{kind} Q={Q} nc={nc} {regime} w={w}')
                worst = [max(a, b) for a, b in zip(worst, r)]
    _lib.ERR_WATCH.poll(block=True)  # no label was out of range
    note(f'parity {kind} nc={nc}: worst loss error {worst[0]:.3f} of the bound, worst gradient error {worst[1]:.3f} of the bound')


@pytest.mark.gpu
def test_pairs_exactly_on_the_kink_are_active():
    """margin 0.5, logits on multiples of 1 / 4: a pair with hinge argument exactly 0 adds 0 to the loss and gets +scale, its label -scale"""
    K = hip()
    x, labels, on_kink = kink_case()
    Q, nc = x.shape
    ref_loss, ref_g = yardstick(x, labels, 'margin_rank', 0.5, W037)
    loss, g = K.choice_loss(x.cuda(), labels.cuda(), 'margin_rank', 0.5, torch.tensor([0.37], device='cuda'))
    compare(loss.item(), g, ref_loss, ref_g, 'margin_rank', x, 0.5, W037, 'exact kink')
    g = g.cpu()
    scale = np.float32(np.float64(np.float32(0.37)) / (Q * (nc - 1)))
    assert bool((g[on_kink] == float(scale)).all())
    hinge = (0.5 - x.gather(1, labels.unsqueeze(1)) + x)
    active = ((hinge >= 0) & (torch.arange(nc).unsqueeze(0) != labels.unsqueeze(1))).sum(1)
    assert torch.equal(g[torch.arange(Q), labels], -(active.float() * float(scale)))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_determinism_and_the_meter(kind):
    """two runs give identical bits; after k calls on different inputs stats = (the sequential double sum of the k fp32 losses, k), exactly"""
    K = hip()
    stats = torch.zeros(2, dtype=torch.float64, device='cuda')
    word = torch.tensor([0.37], device='cuda')
    got, total = [], 0.0
    for i, (Q, nc) in enumerate([(3, 5), (T + 1, 4), (4 * T + 3, 8), (2, 5), (T, 2)]):
        x, labels = make_logits('normal', Q, nc, 31 + i, kind)
        xg, lg = x.cuda(), labels.cuda()
        a = K.choice_loss(xg, lg, kind, 0.1, word, stats)
        b = K.choice_loss(xg, lg, kind, 0.1, word)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        got.append(a[0])
    for l in got:
        total += float(l.item())  # (a Python float is a double: the kernel's stats[0] += (double)loss, in call order)
    assert stats.tolist() == [total, float(len(got))]
    K.zero_words(stats)
    assert stats.tolist() == [0.0, 0.0]


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_pitched_logits_and_gradient(kind):
    """logits and g as views with ld > nc, 2^100 around the inputs, a canary around g: the bits of the contiguous call, the canary intact;
    the backward launch likewise, in place and into a pitched view"""
    from test_pitched_operands import BIG, CANARY, check_guard, pitched, same_bits
    K = hip()
    Q, nc = T + 3, 5
    x, labels = make_logits('normal', Q, nc, 8, kind)
    word, lg = torch.tensor([0.37], device='cuda'), labels.cuda()
    want_loss, want_g = K.choice_loss(x.cuda(), lg, kind, 0.1, word)
    _, xv = pitched(x, 16, 4, BIG, 'cuda')
    gbuf, gv = pitched(torch.zeros(Q, nc), 12, 4, CANARY, 'cuda')
    loss, g = K.choice_loss(xv, lg, kind, 0.1, word, g=gv)
    assert g is gv and same_bits(loss, want_loss) and same_bits(gv, want_g)
    check_guard(gbuf, gv, 'g')
    three = torch.tensor([3.0], device='cuda')
    want_d = K.choice_loss_bwd(want_g, three)
    assert torch.equal(want_d, want_g * 3)
    dbuf, dv = pitched(torch.zeros(Q, nc), 8, 0, CANARY, 'cuda')
    assert same_bits(K.choice_loss_bwd(gv, three, out=dv), want_d)
    check_guard(dbuf, dv, 'dlogits')
    assert same_bits(K.choice_loss_bwd(gv, three, out=gv), want_d)  # dlogits may alias g
    check_guard(gbuf, gv, 'g after the in-place backward')


@pytest.mark.gpu
def test_arguments_outside_the_admitted_range_are_refused():
    """ldl < nc, nc = 0, nc = 1025, margin-rank at nc = 1, Q = 0: QAGNN_EINVAL and nothing enqueued (loss and g keep their canary)"""
    from test_pitched_operands import CANARY
    K = hip()
    x = torch.zeros(4, 1032, device='cuda')
    labels = torch.zeros(4, dtype=torch.long, device='cuda')
    loss = torch.full((1,), CANARY, dtype=torch.int32, device='cuda')
    g = torch.full((4, 1032), CANARY, dtype=torch.int32, device='cuda')
    CE, MR = _lib.LOSS_KINDS['cross_entropy'], _lib.LOSS_KINDS['margin_rank']

    def call(Q, nc, kind, ldl, ldg=1032):
        return K.lib.qagnn_choice_loss_f32(x.data_ptr(), ldl, labels.data_ptr(), Q, nc, kind, 0.1, None, loss.data_ptr(), g.data_ptr(), ldg, None, None,
                                           K._stream())
    for kind in (CE, MR):
        assert call(4, 5, kind, 4) == 1, 'ldl < nc'
        assert call(4, 5, kind, 1032, 4) == 1, 'ldg < nc'
        assert call(4, 0, kind, 1032) == 1, 'nc = 0'
        assert call(4, 1025, kind, 1032) == 1, 'nc = 1025'
        assert call(0, 5, kind, 1032) == 1, 'Q = 0'
    assert call(4, 1, MR, 1032) == 1, 'margin-rank at nc = 1'
    assert call(4, 5, 2, 1032) == 1, 'an unknown kind'
    assert b'choice_loss' in K.lib.qagnn_last_error()
    go = torch.ones(1, device='cuda')
    for Q, nc, ldg, ldd in [(0, 5, 1032, 1032), (4, 0, 1032, 1032), (4, 1025, 1032, 1032), (4, 5, 4, 1032), (4, 5, 1032, 4)]:
        assert K.lib.qagnn_choice_loss_bwd_f32(g.data_ptr(), ldg, go.data_ptr(), g.data_ptr(), ldd, Q, nc, K._stream()) == 1
    torch.cuda.synchronize()
    assert bool((loss == CANARY).all()) and bool((g == CANARY).all())
    assert call(4, 1024, MR, 1032) == 0 and call(4, 1, CE, 1032) == 0  # the ends of the range are inside it
    torch.cuda.synchronize()


NONFINITE = [(v, on) for v in (float('nan'), float('inf'), float('-inf')) for on in (True, False)]


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_nonfinite_logits_behave_as_in_torch(kind):
    """one NaN, +inf or -inf logit, on or off the label column: the loss is NaN (or infinite) exactly where float64 torch's is; gradient
    rows whose yardstick row is finite stay within the bound, and for the cross-entropy only the other rows are non-finite"""
    K = hip()
    Q, nc = 5, 5
    base, labels = make_logits('normal', Q, nc, 21, kind)
    lg = labels.cuda()
    for value, on in NONFINITE:
        x = base.clone()
        col = int(labels[2]) if on else (int(labels[2]) + 1) % nc
        x[2, col] = value
        ref_loss, ref_g = yardstick(x, labels, kind, 0.1, W037)
        loss, g = K.choice_loss(x.cuda(), lg, kind, 0.1, torch.tensor([0.37], device='cuda'))
        ok_rows = torch.isfinite(ref_g).all(1)
        assert int(ok_rows.sum()) >= Q - 1
        compare(loss.item(), g, ref_loss, ref_g, kind, x, 0.1, W037, f'{kind} {value} {"on" if on else "off"} the label column', rows=ok_rows)
        assert np.isnan(loss.item()) == np.isnan(float(ref_loss))
        if kind == 'cross_entropy':
            assert torch.equal(torch.isfinite(g.cpu()).all(1), ok_rows), 'a non-finite gradient row where the yardstick row is finite (or the reverse)'
        note(f'nonfinite {kind} {value} {"on" if on else "off"}: loss {loss.item()} (float64 torch {float(ref_loss)}), finite yardstick rows {int(ok_rows.sum())}/{Q}')


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_labels_out_of_range(kind):
    """labels -1 and nc (nothing larger; the logits lie inside a larger buffer): a zero gradient row, the loss of the yardstick with the
    row's term zeroed and the denominators unchanged, the flag raised through ERR_WATCH and cleared once reported"""
    from test_pitched_operands import BIG, pitched
    K = hip()
    _lib.ERR_WATCH.poll(block=True)
    Q, nc = T + 2, 5
    x, labels = make_logits('normal', Q, nc, 55, kind)
    labels[1], labels[T] = -1, nc
    _, xv = pitched(x, 16, 4, BIG, 'cuda')
    ref_loss, ref_g = yardstick(x, labels, kind, 0.1, W037)
    loss, g = K.choice_loss(xv, labels.cuda(), kind, 0.1, torch.tensor([0.37], device='cuda'))
    compare(loss.item(), g, ref_loss, ref_g, kind, x, 0.1, W037, f'{kind} with labels -1 and nc')
    assert bool((g[1] == 0).all()) and bool((g[T] == 0).all())
    with pytest.raises(RuntimeError, match='labels'):
        _lib.ERR_WATCH.poll(block=True)
    labels[1], labels[T] = 0, nc - 1
    K.choice_loss(xv, labels.cuda(), kind, 0.1)  # the flag word was cleared with the report: a good batch raises nothing
    _lib.ERR_WATCH.poll(block=True)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_autograd_through_choice_loss(kind):
    """(ops.choice_loss(...) * 3).backward() gives 3 g; a second backward raises; compute_loss under autocast computes in fp32"""
    K = hip()
    x, labels = make_logits('normal', 9, 5, 3, kind)
    xg, lg = x.cuda().requires_grad_(True), labels.cuda()
    want_loss, g = K.choice_loss(xg.detach(), lg, kind, 0.1, torch.tensor([0.37], device='cuda'))
    loss = ops.choice_loss(xg, lg, kind, 0.1, 0.37)
    assert loss.dim() == 0 and torch.equal(loss.detach().view(1), want_loss)
    out = loss * 3
    out.backward()
    assert torch.equal(xg.grad, g * 3)
    with pytest.raises(RuntimeError):
        out.backward()
    meter = losses.LossMeter('cuda')
    with torch.autocast('cuda', dtype=torch.bfloat16):
        half = losses.compute_loss(xg.detach().bfloat16(), lg, kind, 0.1, 0.37, meter)
    full = losses.compute_loss(xg.detach().bfloat16().float(), lg, kind, 0.1, 0.37)
    assert half.dtype == torch.float32 and torch.equal(half, full)
    assert meter.read() == (float(half.item()), 1)
    meter.reset()
    assert meter.read() == (0.0, 0)


# ---- module level: the training step ------------------------------------------------------------------------------------------------------
SHIFT_NULL = re.compile(r'(pooler\.w_vs|fc\.layers\.0-Linear)\.bias$')  # (n_fc_layer = 0: the head is one Linear)


def _torch_loss(logits2d, labels, kind, lw):
    """the step's loss as stock torch computes it in fp32: F.cross_entropy, or the yardstick's per-question MarginRankingLoss"""
    if kind == 'cross_entropy':
        return F.cross_entropy(logits2d, labels) * lw
    Q, nc = logits2d.shape
    crit = torch.nn.MarginRankingLoss(margin=float(np.float32(0.1)), reduction='mean')
    ones = torch.ones(nc - 1, device=logits2d.device)
    terms = []
    for q, l in enumerate(labels.tolist()):
        others = torch.tensor([c for c in range(nc) if c != l], device=logits2d.device)
        terms.append(crit(logits2d[q, l].expand(nc - 1), logits2d[q, others], ones))
    return torch.stack(terms).mean() * lw


def _eager_step(model, b, nc, loss_fn, e_cap=None, keep_grads=False):
    """tests/test_graphed.py's eager step with the loss handed in; keep_grads: .grad accumulates over calls (an accumulation window)"""
    from qagnn_amd import data_utils
    if not keep_grads:
        for p in model.parameters():
            p.grad = None
    packed = b['packed']
    if e_cap is not None:  # the same blobs in a buffer laid out for e_cap edges
        blob = torch.zeros(packed.head + 2 * packed.n * packed.B + 3 * e_cap, dtype=torch.int32, device='cuda')
        blob[:packed.buf.numel()] = packed.buf
        packed = data_utils.PackedGraphBatch(blob, packed.B, packed.E, packed.store, packed.sample_ids, nc)
        packed.e_cap = e_cap
    logits, _ = model(b['sent'], b['cids'], b['nt'], b['ns'], b['al'], packed)
    loss = loss_fn(logits.view(-1, nc), b['labels'])
    loss.backward()
    return (logits.detach().clone(), loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
            {k: v.clone() for k, v in model.named_buffers()})


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('nq,nc', [(2, 5), (36, 5)])
def test_eager_step_with_the_native_loss_equals_the_torch_loss(nq, nc, kind):
    """the same model and batch, the loss by ops.choice_loss and by stock torch in fp32: identical logits, the losses within the header's
    bound of each other's float64 value, every gradient tensor within helpers.MIN_FLIP = 3e-5 of its scale (the bar of the issue).
    Tensors whose exact gradient is zero are rounding noise in both runs and have no scale of their own: helpers.has_null_gradient's are
    left out as everywhere else; SHIFT_NULL's -- both losses depend on differences of a question's logits only, sum_c g[q][c] = 0, so a
    bias that moves every logit of a question alike (the linear head's, the pooler's value bias in front of it) has gradient exactly 0
    -- are held to 3e-5 of the scale of their layer's WEIGHT gradient, a sum of the same terms without the cancellation."""
    import test_graphed as TG
    hip()
    b = TG._batch(nq, nc, 200, 3)
    m_nat, m_ref = TG._model(0.0), TG._model(0.0)
    nat = _eager_step(m_nat, b, nc, lambda lg, lab: ops.choice_loss(lg, lab, kind, 0.1, 0.5))
    ref = _eager_step(m_ref, b, nc, lambda lg, lab: _torch_loss(lg, lab, kind, 0.5))
    assert torch.equal(nat[0], ref[0]), 'logits differ'
    x = nat[0].view(-1, nc).cpu()
    want = yardstick(x, b['labels'], kind, 0.1, 0.5)[0]
    lb, _ = _lib.choice_loss_bound(kind, nc, nq, finite_max(x), 0.1, 0.5)
    assert abs(float(nat[1]) - float(want)) <= lb
    assert set(nat[2]) == set(ref[2])
    worst, bad = 0.0, []
    for k in nat[2]:
        if helpers.has_null_gradient(k, True):
            continue
        scale = float(ref[2][re.sub(r'bias$', 'weight', k) if SHIFT_NULL.search(k) else k].abs().max())
        rel = float((nat[2][k] - ref[2][k]).abs().max()) / scale if scale > 0 else float(nat[2][k].abs().max())
        worst = max(worst, rel)
        if not rel <= helpers.MIN_FLIP:
            bad.append(f'{k}: {rel:.2e}')
    note(f'eager step {kind} nq={nq}: native loss {float(nat[1])!r}, torch {float(ref[1])!r}, float64 {float(want)!r}; worst gradient difference {worst:.2e} of scale')
    assert not bad, bad[:8]


@pytest.mark.gpu
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('nq,nc', [(2, 5), (36, 5)])
def test_graphed_step_with_a_native_loss_replays_the_eager_step(nq, nc, kind, accumulate):
    """GraphedStep(loss=kind) over three replays with different batches and weights 1.0, 2 / 64, 0.5: logits, loss, every gradient (the
    window's running sum under accumulate=True) and every buffer have the bits of the eager step with ops.choice_loss on the same
    capacity layout; step.meter.read() is the three losses summed, and 3"""
    import test_graphed as TG
    hip()
    _lib.ERR_WATCH.poll(block=True)
    batches = [TG._batch(nq, nc, 200, seed) for seed in (3, 4, 5)]
    m_eager, m_graph = TG._model(0.0), TG._model(0.0)
    step = graphed.GraphedStep(m_graph, nc, loss=kind)
    total = 0.0
    for i, (b, lw) in enumerate(zip(batches, (1.0, 2 / 64, 0.5))):
        cap = graphed.edge_capacity(b['packed'].E)
        want = _eager_step(m_eager, b, nc, lambda lg, lab: ops.choice_loss(lg, lab, kind, 0.1, lw), e_cap=cap, keep_grads=accumulate and i > 0)
        logits, loss = step(b['sent'], b['cids'], b['nt'], b['ns'], b['al'], b['packed'], b['labels'], lw, accumulate=accumulate)
        got = (logits.detach().clone(), loss.detach().clone(), {k: p.grad.clone() for k, p in m_graph.named_parameters() if p.grad is not None},
               {k: v.clone() for k, v in m_graph.named_buffers()})
        TG._same(got, want, f'{kind} batch {i} (weight {lw}, accumulate={accumulate})')
        total += float(loss.item())
    assert step.meter.read() == (total, 3)
    torch.cuda.synchronize()
    _lib.ERR_WATCH.poll(block=True)
    step.meter.reset()
    assert step.meter.read() == (0.0, 0)
