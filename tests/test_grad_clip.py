"""Gradient-norm clipping in front of the optimiser step (reference qagnn.py:267-278: clip_grad_norm_; scheduler.step(); optimizer.step()).

Yardsticks: the reference's own call, torch.nn.utils.clip_grad_norm_, on float64 CPU copies of the gradients; for the update,
oracle.radam_oracle.radam_step in float64.

* not GPU: qagnn_amd.optimization_utils.clip_grad_norm_ on CPU parameters IS torch's function (same return value, same gradients);
  RAdam's deferred gradient scale on the CPU loop; the type check of defer_to.
* `-m gpu`: qagnn_grad_norm_f32 / qagnn_scale_multi_f32 / qagnn_radam_step_scaled_f32 through the C ABI on a tensor list that crosses
  the 24-tensor and the 320-block pack limits, with gradients that are misaligned views of one flat buffer.
"""
import math

import numpy as np
import pytest
import torch

import helpers  # noqa: F401  (puts the repository root on sys.path)
from oracle import radam_oracle as RO
from qagnn_amd import optimization_utils as OU

# 31 tensors: around the 256-thread and the 4096-element chunk boundaries, an empty one, 20 small ones (with the 10 before them: more than
# one 24-tensor pack), and one of 322 chunks (more than a 320-block pack: it is split across packs)
SIZES = [1, 3, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 1, 0] + [17 * (i + 1) for i in range(20)] + [321 * 4096 + 5]


def hip():
    from qagnn_amd import ops
    ops.set_kernels(None)
    return ops.kernels()


def views(flat, sizes=SIZES):
    out, off = [], 0
    for n in sizes:
        out.append(flat[off:off + n])
        off += n
    assert off == flat.numel()
    return out


def common_flat(seed=0, zero=False):
    """One flat fp32 buffer at a 12-byte offset into its allocation (no view of it is 16-byte aligned), tensor i scaled by 10^((i % 6) - 3)."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    total = sum(SIZES)
    flat = torch.randn(total + 3, generator=g, device='cuda')[3:]
    if zero:
        flat.zero_()
    for i, v in enumerate(views(flat)):
        v.mul_(10.0 ** ((i % 6) - 3))
    assert flat.data_ptr() % 16 == 12
    return flat


def clone_misaligned(flat):
    c = torch.empty(flat.numel() + 3, dtype=flat.dtype, device=flat.device)[3:]
    c.copy_(flat)
    return c


def torch_clip_f64(tensors, max_norm):
    """The yardstick: torch.nn.utils.clip_grad_norm_ on float64 CPU copies -> (norm, coefficient), the coefficient read off the largest
    gradient element before and after torch's own clip (1 where every gradient is zero: torch multiplies by clamp(1e6, max=1))."""
    ps = []
    for t in tensors:
        p = torch.nn.Parameter(torch.zeros(t.numel(), dtype=torch.float64))
        p.grad = t.detach().double().cpu().reshape(-1).clone()
        ps.append(p)
    before = torch.cat([p.grad for p in ps]).clone()
    norm = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    after = torch.cat([p.grad for p in ps])
    i = int(before.abs().argmax())
    coef = float(after[i] / before[i]) if float(before[i]) != 0.0 else 1.0
    return norm, coef


def norm_bar():
    """Worst-case relative error of the fp32 norm, from the reduction shape of csrc/optim.hip (all terms are non-negative, so every rounding
    is relative): 1 ulp per square, c sequential adds per thread, an L-level tree, halved by the square root, + 1 ulp for the final cast.
    (The second stage is in double.)"""
    from qagnn_amd._lib import HipKernels
    c = HipKernels.GRAD_NORM_CHUNK // HipKernels.GRAD_NORM_THREADS
    L = int(math.log2(HipKernels.GRAD_NORM_THREADS))
    assert 2 ** L == HipKernels.GRAD_NORM_THREADS
    return ((c + L + 1) / 2 + 1) * 2.0 ** -24


# ---- not GPU -----------------------------------------------------------------------------------------------------------------

def _cpu_params(seed=1, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(dtype)) for s in [(7, 5), (11,), (3, 2, 2), (1,)]]
    for i, p in enumerate(ps):
        p.grad = (torch.randn(p.shape, generator=g) * 10.0 ** (i - 1)).to(dtype)
    return ps


@pytest.mark.parametrize('kwargs', [dict(), dict(norm_type=1.5), dict(norm_type=float('inf')), dict(error_if_nonfinite=True)])
@pytest.mark.parametrize('max_norm', [1.0, 1e9])
def test_cpu_parameters_go_to_torch_unchanged(kwargs, max_norm):
    """On CPU parameters the function returns exactly what torch.nn.utils.clip_grad_norm_ returns and leaves exactly its gradients."""
    a, b = _cpu_params(), _cpu_params()
    ra = OU.clip_grad_norm_(a, max_norm, **kwargs)
    rb = torch.nn.utils.clip_grad_norm_(b, max_norm, **kwargs)
    assert ra.dim() == 0 and ra.dtype == rb.dtype and torch.equal(ra, rb)
    for p, q in zip(a, b):
        assert torch.equal(p.grad, q.grad)
    # a generator of parameters and a single tensor, as torch takes them
    c = _cpu_params()
    assert torch.equal(OU.clip_grad_norm_((p for p in c), max_norm, **kwargs), rb)
    assert torch.equal(c[0].grad, b[0].grad)
    d, e = _cpu_params()[0], _cpu_params()[0]
    assert torch.equal(OU.clip_grad_norm_(d, max_norm, **kwargs), torch.nn.utils.clip_grad_norm_(e, max_norm, **kwargs))
    assert torch.equal(d.grad, e.grad)


def test_cpu_error_if_nonfinite_raises_as_torch_does():
    a, b = _cpu_params(), _cpu_params()
    a[1].grad[3] = float('nan')
    b[1].grad[3] = float('nan')
    with pytest.raises(RuntimeError) as ea:
        OU.clip_grad_norm_(a, 1.0, error_if_nonfinite=True)
    with pytest.raises(RuntimeError) as eb:
        torch.nn.utils.clip_grad_norm_(b, 1.0, error_if_nonfinite=True)
    assert str(ea.value) == str(eb.value)
    # without the flag the NaN propagates into the norm and every gradient, as in torch
    ra, rb = OU.clip_grad_norm_(a, 1.0), torch.nn.utils.clip_grad_norm_(b, 1.0)
    assert torch.isnan(ra) and torch.isnan(rb) and all(torch.isnan(p.grad).all() for p in a)


def _radam_with_state(ps, step0=5):
    opt = OU.RAdam(ps, lr=1e-2, weight_decay=0.01)
    g = torch.Generator().manual_seed(9)
    for p in ps:
        opt.state[p] = dict(step=step0, exp_avg=0.01 * torch.randn(p.shape, generator=g), exp_avg_sq=(0.01 * torch.randn(p.shape, generator=g)) ** 2)
    return opt


def _same_state(pa, oa, pb, ob):
    for p, q in zip(pa, pb):
        assert torch.equal(p.detach(), q.detach())
        for k in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(oa.state[p][k], ob.state[q][k])
        assert oa.state[p]['step'] == ob.state[q]['step']


def test_cpu_radam_deferred_scale_equals_torch_clip_then_step():
    """CPU RAdam and the deferred form, against torch.nn.utils.clip_grad_norm_ followed by a plain step, bit for bit, on clones.

    CPU gradients are on the fallback path of clip_grad_norm_, where defer_to is ignored (torch clips in place, the optimiser is given
    nothing): part (a) holds that.  The CPU loop of RAdam.step() applies a deferred coefficient all the same (it serves parameters of a
    GPU run that are not fp32 / contiguous): part (b) hands it the coefficient the way clip_grad_norm_ does on the fused path,
    RAdam.defer_grad_scale, computed from torch's returned norm by torch's formula."""
    for step0 in (0, 5):  # step 1: the SGD-like branch, step 6: the rectified branch
        ref = _cpu_params()
        oref = _radam_with_state(ref, step0)
        norm = torch.nn.utils.clip_grad_norm_(ref, 1.0)
        clipped = [p.grad.clone() for p in ref]
        oref.step()
        # (a) the public call on CPU parameters
        a = _cpu_params()
        oa = _radam_with_state(a, step0)
        ra = OU.clip_grad_norm_(a, 1.0, defer_to=oa)
        assert torch.equal(ra, norm)
        for p, c in zip(a, clipped):
            assert torch.equal(p.grad, c)
        oa.step()
        for p, c in zip(a, clipped):
            assert torch.equal(p.grad, c)      # the step leaves the gradients alone
        _same_state(a, oa, ref, oref)
        # (b) the deferred coefficient on the CPU loop
        b = _cpu_params()
        ob = _radam_with_state(b, step0)
        raw = [p.grad.clone() for p in b]
        coef = torch.clamp(1.0 / (norm + 1e-6), max=1.0)   # torch's clip_coef_clamped, from the norm torch returned
        assert float(coef) < 1.0
        ob.defer_grad_scale(coef.reshape(1))
        ob.step()
        for p, g0 in zip(b, raw):
            assert torch.equal(p.grad, g0)     # gradients unchanged by the deferred step
        _same_state(b, ob, ref, oref)
        # a second step() without a new clip call applies no scale: equal to a plain step on the UNclipped gradients
        for p, g0 in zip(ref, raw):
            p.grad = g0.clone()
        oref.step()
        ob.step()
        _same_state(b, ob, ref, oref)


def test_defer_to_rejects_other_optimizers():
    ps = _cpu_params()
    for other in (torch.optim.SGD(ps, lr=0.1), OU.AdamW(ps, lr=0.1), torch.optim.RAdam(ps, lr=0.1), object()):
        before = [p.grad.clone() for p in ps]
        with pytest.raises(TypeError, match='RAdam'):
            OU.clip_grad_norm_(ps, 1.0, defer_to=other)
        assert all(torch.equal(p.grad, b) for p, b in zip(ps, before))   # rejected before anything is clipped
    OU.clip_grad_norm_(ps, 1.0, defer_to=OU.RAdam(ps))


def test_new_entry_points_are_declared_and_bound():
    """(tests/test_hip_kernels.py::test_library_exports_every_declared_symbol holds header, library and EXPORTS together)"""
    from qagnn_amd import _lib
    for name in ('qagnn_grad_norm_workspace_elems', 'qagnn_grad_norm_f32', 'qagnn_scale_multi_f32', 'qagnn_radam_step_scaled_f32'):
        assert name in _lib.EXPORTS
    assert set(OU.OPTIMIZER_CLASSES) == {'sgd', 'adam', 'adamw', 'radam'}


# ---- GPU ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('one_tensor', [False, True], ids=['31-tensors', 'flat-bucket'])
def test_norm_and_coefficient_vs_float64(one_tensor):
    """Norm and coefficient against torch.nn.utils.clip_grad_norm_ in float64, on the 31-tensor list and on ONE tensor holding the whole
    flat buffer (what parallel.GradBucket.flat looks like).  The bar is derived, not measured -- norm_bar(): ((c + L + 1) / 2 + 1) 2^-24 from
    the kernel's own constants (c = 4096 / 256 = 16 adds per thread, L = 8 tree levels: 8.05e-7); the coefficient gets 2^-24 more."""
    k = hip()
    bar = norm_bar()
    assert abs(bar - 8.05e-7) < 1e-8
    flat = common_flat()
    grads = [flat] if one_tensor else views(flat)
    for max_norm in (1.0, 1e9):
        want_norm, want_coef = torch_clip_f64(grads, max_norm)
        out = k.grad_norm(grads, max_norm).cpu().double().numpy()
        print(f'max_norm {max_norm:g}: norm {out[0]!r} vs {want_norm!r} (rel {abs(out[0] - want_norm) / want_norm:.3e}, bar {bar:.3e}); '
              f'coef {out[1]!r} vs {want_coef!r} (rel {abs(out[1] - want_coef) / want_coef:.3e})')
        assert 6.0e3 < want_norm < 8.0e3
        assert abs(out[0] - want_norm) <= bar * want_norm
        if max_norm == 1e9:
            assert want_coef == 1.0 and out[1] == 1.0     # exactly 1.0f
        else:
            assert want_coef < 1.0 and abs(out[1] - want_coef) <= (bar + 2.0 ** -24) * want_coef
    zflat = common_flat(zero=True)
    zgrads = [zflat] if one_tensor else views(zflat)
    assert torch_clip_f64(zgrads, 1.0) == (0.0, 1.0)
    out = k.grad_norm(zgrads, 1.0).cpu()
    assert not torch.isnan(out).any() and float(out[0]) == 0.0 and float(out[1]) == 1.0
    total = OU.clip_grad_norm_([_with_grad(g) for g in zgrads], 1.0)
    assert float(total) == 0.0 and not torch.isnan(zflat).any() and float(zflat.abs().max()) == 0.0


def _with_grad(g, p=None):
    p = torch.nn.Parameter(torch.zeros_like(g) if p is None else p)
    p.grad = g
    return p


@pytest.mark.gpu
def test_norm_is_deterministic_and_covers_its_workspace():
    """Two calls on the same input, each with its workspace pre-filled with NaN (a slot that no block wrote would surface): bit-identical,
    finite results.  No atomics, fixed summation order."""
    k = hip()
    grads = views(common_flat())
    need = k.grad_norm_workspace_elems(grads)
    assert need == sum(-(-n // k.GRAD_NORM_CHUNK) for n in SIZES)
    outs = []
    for _ in range(2):
        ws = torch.full((need,), float('nan'), device='cuda')
        outs.append(k.grad_norm(grads, 1.0, workspace=ws))
    a, b = (o.cpu() for o in outs)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(AssertionError):
        k.grad_norm(grads, 1.0, workspace=torch.empty(need - 1, device='cuda'))


@pytest.mark.gpu
def test_in_place_clip_is_one_fp32_product_per_element():
    """After the in-place form every gradient equals fl32(g * coef_device) bit for bit (expectation computed on the CPU in fp32 from the
    coefficient word read back; the coefficient itself is held to float64 in test_norm_and_coefficient_vs_float64).  The public
    clip_grad_norm_(defer_to=None) is the same two calls."""
    k = hip()
    flat = common_flat()
    before = flat.cpu().clone()
    grads = views(flat)
    out = k.grad_norm(grads, 1.0)
    k.scale_multi(grads, out[1:2])
    coef = out[1].cpu()
    assert 0.0 < float(coef) < 1.0
    want = before * coef
    assert torch.equal(flat.cpu().view(torch.int32), want.view(torch.int32))
    flat2 = clone_misaligned(torch.empty_like(flat).copy_(before))
    total = OU.clip_grad_norm_([_with_grad(g) for g in views(flat2)], 1.0)
    assert total.dim() == 0 and total.is_cuda and torch.equal(total.cpu(), out[0].cpu())
    assert torch.equal(flat2.cpu().view(torch.int32), want.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize('step,wd', [(1, 0.01), (6, 0.01)])
def test_deferred_clip_radam_decoder_tensor_list_vs_float64(step, wd):
    """clip_grad_norm_(params, 1.0, defer_to=opt); opt.step() on all trainable tensors of the CSQA decoder (the set-up of
    test_optimization.py::test_fused_radam_decoder_tensor_list_vs_float64: 74 tensors, misaligned gradient views, random m and v), at a
    step of the SGD-like branch and one of the rectified branch, against the float64 oracle fed g64 * float64(coef_device) at that
    test's bars, unchanged (the one extra rounding of g * coef is 6e-8 relative).  The gradients are bit-identical before and after."""
    from qagnn_amd import modeling_qagnn as MQ
    k = hip()
    torch.manual_seed(0)
    model = MQ.QAGNN(None, 5, 4, 38, 1024, 3000, 200, 1024, 2, 200, 0, 0.2, 0.2, 0.2).cuda()
    params = [p for p in model.parameters() if p.requires_grad]
    total = sum(p.numel() for p in params)
    assert len(params) >= 70 and total > 2_500_000
    g = torch.Generator(device='cuda').manual_seed(step)
    flat = torch.randn(total + 3, generator=g, device='cuda')[3:]      # 12-byte offset: no view is 16-byte aligned by construction
    off, p0 = 0, []
    for p in params:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
        p0.append(p.detach().cpu().numpy().astype(np.float64))
    flat0 = flat.cpu().clone()
    opt = OU.RAdam(params, lr=1e-3, weight_decay=wd)
    m0 = [0.01 * torch.randn_like(p) for p in params]
    v0 = [(0.01 * torch.randn_like(p)) ** 2 for p in params]
    for p, m, v in zip(params, m0, v0):
        opt.state[p] = dict(step=step - 1, exp_avg=m.clone(), exp_avg_sq=v.clone())
    word = k.grad_norm([p.grad for p in params], 1.0).cpu()     # the coefficient word (the same bits on every call: see the determinism test)
    want_norm, want_coef = torch_clip_f64([p.grad for p in params], 1.0)
    norm = OU.clip_grad_norm_(params, 1.0, defer_to=opt)
    assert torch.equal(norm.cpu(), word[0]) and abs(float(norm) - want_norm) <= norm_bar() * want_norm
    coef = np.float64(word[1].item())
    assert 0.0 < coef < 1.0 and abs(coef - want_coef) <= (norm_bar() + 2.0 ** -24) * want_coef
    assert torch.equal(flat.cpu().view(torch.int32), flat0.view(torch.int32))   # the clip call does not touch them
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(flat.cpu().view(torch.int32), flat0.view(torch.int32))   # nor does the step
    worst = dict(m=0.0, v=0.0, p=0.0)   # max over all elements of |got - ref| / (atol + rtol |ref|): assert_allclose's criterion is <= 1
    for p, pb, m, v in zip(params, p0, m0, v0):
        g64 = p.grad.cpu().numpy().astype(np.float64) * coef
        rp, rm, rv = RO.radam_step(pb, g64, m.cpu().numpy(), v.cpu().numpy(), step, 1e-3, weight_decay=wd)
        st = opt.state[p]
        assert st['step'] == step
        for key, got, ref, atol in (('m', st['exp_avg'], rm, 3e-8), ('v', st['exp_avg_sq'], rv, 1e-10), ('p', p.detach(), rp, 1e-7)):
            got = got.cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all()
            worst[key] = max(worst[key], float(np.max(np.abs(got - ref) / (atol + 2e-6 * np.abs(ref)))))
    print(f'step {step}: worst |got - ref| / (atol + 2e-6 |ref|), atol 3e-8 / 1e-10 / 1e-7 for m / v / p: {worst}')
    assert worst['m'] <= 1.0 and worst['v'] <= 1.0 and worst['p'] <= 1.0, worst


class _Run:
    """Parameters, RAdam state and gradient views over the common input: clones of one (p, m, v, g) set."""

    def __init__(self, p0, m0, v0, gflat, step0):
        self.flat = clone_misaligned(gflat)
        self.params = [_with_grad(g, p.clone()) for g, p in zip(views(self.flat), p0)]
        self.opt = OU.RAdam(self.params, lr=1e-3, weight_decay=0.01)
        for p, m, v in zip(self.params, m0, v0):
            self.opt.state[p] = dict(step=step0, exp_avg=m.clone(), exp_avg_sq=v.clone())

    def bits(self):
        torch.cuda.synchronize()
        out = []
        for p in self.params:
            st = self.opt.state[p]
            out += [p.detach().cpu().view(torch.int32), st['exp_avg'].cpu().view(torch.int32), st['exp_avg_sq'].cpu().view(torch.int32)]
        return out


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.bits(), b.bits()))


@pytest.mark.gpu
@pytest.mark.parametrize('step0', [0, 5], ids=['step1-sgd-branch', 'step6-rectified'])
def test_equivalences_without_tolerance(step0):
    """On the 31-tensor input with random p, m, v, all on clones, bit for bit:
    deferred step with max_norm = 1e9 (coefficient exactly 1) == plain step();  deferred step with max_norm = 1 == in-place clip + plain
    step();  a second step() after a deferred one == a plain step() (the coefficient is consumed once)."""
    hip()
    gflat = common_flat()
    gen = torch.Generator(device='cuda').manual_seed(11)
    p0 = [torch.randn(n, generator=gen, device='cuda') for n in SIZES]
    m0 = [0.01 * torch.randn(n, generator=gen, device='cuda') for n in SIZES]
    v0 = [(0.01 * torch.randn(n, generator=gen, device='cuda')) ** 2 for n in SIZES]
    make = lambda: _Run(p0, m0, v0, gflat, step0)  # noqa: E731

    plain, big = make(), make()
    plain.opt.step()
    OU.clip_grad_norm_(big.params, 1e9, defer_to=big.opt)
    big.opt.step()
    assert _equal(plain, big)
    assert any(not torch.equal(p.detach(), q) for p, q in zip(plain.params, p0) if q.numel())  # (the step did move the parameters)

    deferred, inplace = make(), make()
    na = OU.clip_grad_norm_(deferred.params, 1.0, defer_to=deferred.opt)
    deferred.opt.step()
    nb = OU.clip_grad_norm_(inplace.params, 1.0)
    inplace.opt.step()
    assert torch.equal(na.cpu(), nb.cpu())
    assert _equal(deferred, inplace)
    assert not _equal(deferred, plain)                                   # (and the clip did change the update)
    assert torch.equal(deferred.flat.cpu().view(torch.int32), gflat.cpu().view(torch.int32))
    assert not torch.equal(inplace.flat.cpu(), gflat.cpu())

    # second step: `deferred` again without a clip call, against a plain step from the same state on the same (unclipped) gradients
    inplace.flat.copy_(gflat)
    deferred.opt.step()
    inplace.opt.step()
    assert _equal(deferred, inplace)
