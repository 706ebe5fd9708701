"""The forward-only (evaluation) path: include/qagnn_hip_infer.h, ops.inference_path / ops.stack_infer, qagnn_amd.inference.

Without a GPU: the extension header against the bindings and the built library, the module's routing, the emulation of the new entry
points, evaluate_accuracy and the eval golden cases through the emulated path.  `-m gpu`: the two new kernels against float64 /
torch.argmax, the inference stack against the stack forward (form off: bit for bit, on shared buffers) and against the float64
emulation (form on), its operand maxima, its memory, GraphedForward against the eager inference forward, evaluate_accuracy.
"""
import contextlib
import ctypes
import os
import re

import pytest
import torch

import helpers
from emu_infer import EmuInferKernels
from emu_kernels import EmuKernels
from qagnn_amd import _lib, data_utils, graphed, inference, ops, synthetic
from test_host_logic_emu import FWD, build, golden_inputs

EVAL_CASES = [c for c in helpers.GOLDEN_CASES if not helpers.GOLDEN_CASES[c]['train']]
AM_X, AM_S, AM_AGGR, AM_H1, AM_Y = _lib.HOP_AM_X, _lib.HOP_AM_S, _lib.HOP_AM_AGGR, _lib.HOP_AM_H1, _lib.HOP_AM_Y  # a hop's amax words
LOG = os.environ.get('QAGNN_INFER_TEST_LOG')  # file that collects the measured figures of the GPU tests


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


# =================================================================================================================================
# Without a GPU
# =================================================================================================================================
def test_infer_header_bindings_and_build_hash():
    """qagnn_hip_infer.h declares exactly EXPORTS_INFER; the built library exports them; the build hash covers the header and
    infer.hip; the ABI number and the export list of qagnn_hip.h are where they were."""
    from qagnn_amd import build as B
    hdr = open(os.path.join(helpers.ROOT, 'include', 'qagnn_hip_infer.h')).read()
    declared = sorted(set(re.findall(r'\b(qagnn_[a-z0-9_]+)\s*\(', hdr)))
    assert declared == sorted(_lib.EXPORTS_INFER) and len(declared) == 5
    B.build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in qagnn_hip_infer.h but not exported'
    lib = _lib.load_library()  # prototypes resolve
    assert lib.qagnn_infer_version() == 1
    hashed = {os.path.realpath(p) for p in B.hashed_files()}
    assert os.path.realpath(os.path.join(helpers.ROOT, 'include', 'qagnn_hip_infer.h')) in hashed
    assert os.path.realpath(os.path.join(B.CSRC, 'infer.hip')) in hashed and 'infer.hip' in B.SOURCES
    assert _lib.ABI_VERSION == 25 and len(_lib.EXPORTS) == 63
    assert not set(_lib.EXPORTS_INFER) & set(_lib.EXPORTS + _lib.EXPORTS_TN)
    # host-only entry points need no GPU: the scratch of the maximum pass never exceeds what the hop workspace leaves it (N floats)
    for R in (1, 7, 8, 255, 8200, 64000):
        for Cc in (16, 208, 256, 2048):
            n = lib.qagnn_bn_relu_absmax_scratch_elems(R, Cc)
            assert 1 <= n <= max(R, 1) and n <= 2048, (R, Cc, n)


class _Spy(EmuInferKernels):
    def __init__(self):
        self.calls = []

    def stack_fwd(self, *a, **kw):
        self.calls.append('stack_fwd')
        return super().stack_fwd(*a, **kw)

    def stack_infer(self, *a, **kw):
        self.calls.append('stack_infer')
        return super().stack_infer(*a, **kw)


class _SpyWithout(EmuKernels):
    def __init__(self):
        self.calls = []

    def stack_fwd(self, *a, **kw):
        self.calls.append('stack_fwd')
        return super().stack_fwd(*a, **kw)


def _forward(model, args, grad=False, switch=True):
    with (contextlib.nullcontext() if grad else torch.no_grad()), ops.inference_path(switch):
        return model(*args[:5], (args[5], args[6]))


def test_module_routing():
    """stack_infer only with the switch on, in eval mode, without autograd, with running statistics and a provider that has it."""
    case = 'small_eval'
    args = golden_inputs(case, helpers.load_golden(case))
    assert ops.INFERENCE_PATH is False
    with provider(_Spy()) as K:
        model = build(case)
        assert not model.training
        _forward(model, args)
        assert K.calls == ['stack_infer']
        want = _forward(model, args)[0]
        for what, kw in (('switch off', dict(switch=False)), ('grad enabled', dict(grad=True))):
            K.calls.clear()
            got = _forward(model, args, **kw)[0]
            assert K.calls == ['stack_fwd'], what
            assert torch.equal(got, want), what  # (on the emulation both routes are the composed per-kernel path)
        K.calls.clear()
        with torch.no_grad():
            model(*args[:5], (args[5], args[6]))  # (never entered the scope)
        assert K.calls == ['stack_fwd'] and ops.INFERENCE_PATH is False
        K.calls.clear()
        model.train()
        _forward(model, args)
        assert K.calls == ['stack_fwd'], 'training'
        model.eval()
        K.calls.clear()
        for layer in model.gnn.gnn_layers:
            layer.mlp[1].track_running_stats = False
        _forward(model, args)
        assert K.calls == ['stack_fwd'], 'track_running_stats=False'
    with provider(_SpyWithout()) as K:
        _forward(build(case), args)
        assert K.calls == ['stack_fwd'], 'a provider without stack_infer'


def _choice_case(Q, nc, seed):
    """logits with ties (a coarse grid), NaN rows, -inf rows, a +inf; labels with values outside [0, nc)"""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randint(-2, 3, (Q, nc), generator=g).float() * 0.5
    labels = torch.randint(0, nc, (Q,), generator=g)
    for q in range(0, Q, 5):
        logits[q, int(torch.randint(0, nc, (1,), generator=g))] = float('nan')
    for q in range(1, Q, 7):
        logits[q] = float('-inf')
    for q in range(2, Q, 11):
        logits[q, nc - 1] = float('nan')
        logits[q, 0] = float('nan') if q % 2 else float('inf')
    for q in range(3, Q, 6):
        labels[q] = (-1, nc, 10 ** 12)[q % 3]
    return logits, labels


@pytest.mark.parametrize('Q,nc', [(1, 2), (7, 4), (40, 5), (33, 8)])
def test_choice_eval_emulation_against_torch_argmax(Q, nc):
    logits, labels = _choice_case(Q, nc, 3 + Q)
    counts, pred = torch.tensor([5, 9]), torch.empty(Q, dtype=torch.long)
    EmuInferKernels().choice_eval(logits, labels, counts, pred)
    want = torch.argmax(logits, dim=1)
    assert torch.equal(pred, want)
    assert counts.tolist() == [5 + int((want == labels).sum()), 9 + Q]
    EmuInferKernels().choice_eval(logits, None, counts)
    assert counts.tolist() == [5 + int((want == labels).sum()), 9 + 2 * Q]


_SET_CFG = helpers.model_cfg(d=32, k=2, sent_dim=24, n_concept=300, concept_in_dim=16)


def _eval_set(sizes, nc, n, cfg, shape, device='cpu', seed0=60):
    """decoder-level batches (qids, labels, sent_vecs, concept_ids, node_type_ids, node_scores, adj_lengths, (edge_index, edge_type))"""
    out = []
    for i, nq in enumerate(sizes):
        c = dict(shape=shape, nq=nq, nc=nc, n=n, n_rel=17, seed=seed0 + i, cfg=cfg)
        x = helpers.make_case_inputs(c)
        B = nq * nc
        labels = torch.randint(0, nc, (nq,), generator=torch.Generator().manual_seed(seed0 + 100 + i))
        t = [x['sent_vecs'], x['concept_ids'].view(B, n), x['node_type_ids'].view(B, n), x['node_scores'].view(B, n, 1), x['adj_lengths'].view(B)]
        t = [v.to(device) for v in t]
        out.append((list(range(nq)), labels.to(device), *t, (x['edge_index'].to(device), x['edge_type'].to(device))))
    return out


def _reference_accuracy(eval_set, model, nc):
    """the reference's loop (qagnn.py:30-38), with the decoder's [B, 1] logits viewed as [questions, choices]"""
    n_samples, n_correct = 0, 0
    model.eval()
    with torch.no_grad():
        for qids, labels, *input_data in eval_set:
            logits, _ = model(*input_data)
            n_correct += (logits.view(-1, nc).argmax(1) == labels).sum().item()
            n_samples += labels.size(0)
    return n_correct, n_samples


def _half_right(eval_set, model, nc):
    """the set with labels the model gets right for every second question (its own argmax) and wrong for the others (the next choice):
    6 hits of 11 -- a count that a dropped or doubled hit moves"""
    out, q = [], 0
    model.eval()
    with torch.no_grad():
        for qids, labels, *input_data in eval_set:
            pred = model(*input_data)[0].view(-1, nc).argmax(1)
            idx = torch.arange(q, q + labels.size(0), device=pred.device)
            out.append((qids, torch.where(idx % 2 == 0, pred, (pred + 1) % nc), *input_data))
            q += labels.size(0)
    return out


def test_evaluate_accuracy_on_the_emulation():
    nc = 3
    with provider(_Spy()) as K:
        model = build('small_eval')
        es = _half_right(_eval_set([2, 2, 2, 2, 2, 1], nc, 20, _SET_CFG, 'tiny'), model, nc)
        K.calls.clear()
        got = inference.evaluate_accuracy(es, model.train())
        assert not model.training and set(K.calls) == {'stack_infer'} and len(K.calls) == 6
        n_correct, n_samples = _reference_accuracy(es, model, nc)
        assert (n_correct, n_samples) == (6, 11) and got == n_correct / n_samples
        assert ops.INFERENCE_PATH is False
        with pytest.raises(ZeroDivisionError):  # (the reference's answer to an empty set)
            inference.evaluate_accuracy([], model)
        with pytest.raises(ZeroDivisionError):
            inference.evaluate_accuracy([], model, graphed=True)


def test_evaluate_accuracy_through_lm_qagnn_on_the_emulation():
    """LM_QAGNN: logits [bs, nc], the encoder eager, nested edge lists as the reference's loader yields them"""
    from qagnn_amd import modeling_qagnn as MQ
    case = 'small_train'
    c, fix = helpers.GOLDEN_CASES[case], helpers.load_golden(case)
    cfg = c['cfg']
    with provider(EmuInferKernels()):
        torch.manual_seed(0)
        model = MQ.LM_QAGNN(None, 'stub', cfg['k'], cfg['n_ntype'], cfg['n_etype'], cfg['n_concept'], cfg['concept_dim'], cfg['concept_in_dim'],
                            cfg['n_attention_head'], cfg['fc_dim'], cfg['n_fc_layer'], 0.0, 0.0, 0.0, init_range=0.02,
                            encoder=helpers.StubTextEncoder(sent_dim=cfg['sent_dim'], in_dim=helpers.LM_CASES[case]['in_dim']))
        helpers.det_fill_(model, 5, 0.8)
        _, cids, nt, ns, al, _, _ = golden_inputs(case, fix)
        nq, nc, n = c['nq'], c['nc'], c['n']
        nei, net = helpers.nested_graph_lists(case, fix)
        inp = [helpers.lm_inputs(case), cids.view(nq, nc, n), nt.view(nq, nc, n), ns.view(nq, nc, n, 1), al.view(nq, nc), nei, net]
        es = [(None, torch.tensor([l0, l1]), *inp) for l0, l1 in ((0, 1), (2, 2), (1, 0))]
        got = inference.evaluate_accuracy(es, model)
        model.eval()
        with torch.no_grad():
            pred = model(*inp)[0].argmax(1)
        assert got == sum(int((pred == b[1]).sum()) for b in es) / 6


@pytest.mark.parametrize('what', ['model', 'stack'])
@pytest.mark.parametrize('case', EVAL_CASES)
def test_eval_golden_cases_through_the_emulated_inference_path(case, what):
    fix = helpers.load_golden(case)
    c = helpers.GOLDEN_CASES[case]
    with provider(_Spy()) as K:
        model = build(case)
        sv, cids, nt, ns, al, ei, et = golden_inputs(case, fix)
        with torch.no_grad(), ops.inference_path():
            if what == 'model':
                logits, pool_attn = model(sv, cids, nt, ns, al, (ei, et))
                helpers.check_plain(fix, 'logits', logits, **FWD)
                helpers.check_plain(fix, 'pool_attn', pool_attn, **FWD)
            else:
                H, nsc, _, _ = helpers.mp_inputs(case)
                nsc = nsc * (torch.arange(c['n']) < al.unsqueeze(1)).float().unsqueeze(2)
                helpers.check_stored(fix, 'mp_out', model.gnn(H, (ei, et), nt, nsc), **FWD)
        assert K.calls == ['stack_infer']


# =================================================================================================================================
# On the GPU: the two kernels
# =================================================================================================================================
def _bits(x):
    return int(torch.tensor(float(x), dtype=torch.float32).view(torch.int32).item())


def _pitched(H, fill=2.0 ** 100):
    """H as a view into a larger buffer of 2^100: rows a pitch apart, guard rows above and below, guard columns left and right"""
    R, Cc = H.shape
    buf = torch.full((R + 2, Cc + 8), fill, dtype=torch.float32, device='cuda')
    buf[1:R + 1, 4:4 + Cc] = H
    return buf[1:R + 1, 4:4 + Cc]


def _bra_reference(H, scale, shift):
    """the float64 maximum of the prologue's values, rounded to fp32 (NaNs skipped; nothing positive: 0) -> bit pattern"""
    return int(EmuInferKernels().bn_relu_absmax(H.cpu(), scale.cpu(), shift.cpu())[0])


def _bra_operands(R, Cc, seed):
    g = torch.Generator().manual_seed(seed)
    H = torch.randn(R, Cc, generator=g) * 3
    scale = torch.randn(Cc, generator=g)
    scale[::5] = 0.0           # (the column of ones: scale 0, shift 1)
    scale[1::3] = -scale[1::3].abs()
    shift = torch.randn(Cc, generator=g)
    shift[::5] = 1.0
    return H, scale, shift


def _held(word, ref, what):
    """never below the float64 maximum rounded to fp32, never more than 2 ulp above it (positive floats order like their bit patterns)"""
    assert 0 <= word - ref <= 2, f'{what}: word {word:#x} against {ref:#x}'


@pytest.mark.gpu
@pytest.mark.parametrize('Cc', [16, 208, 256])
@pytest.mark.parametrize('R', [1, 255, 256, 257, 1025])
def test_bn_relu_absmax(R, Cc):
    K = hip()
    H, scale, shift = _bra_operands(R, Cc, 100 * R + Cc)
    Hd, sc, sh = _pitched(H.cuda()), scale.cuda(), shift.cuda()
    assert not Hd.is_contiguous() or R == 1
    ref = _bra_reference(H, scale, shift)
    assert ref > 0
    w = K.bn_relu_absmax(Hd, sc, sh)
    _held(int(w[0]), ref, 'pitched')
    assert w[1:].tolist() == [0, 0, 0]
    _held(int(K.bn_relu_absmax(H.cuda(), sc, sh)[0]), ref, 'dense')
    # a second call into the same word keeps the larger, in either order
    small = H * 0.25
    ref_small = _bra_reference(small, scale, shift)
    first = int(w[0])
    K.bn_relu_absmax(_pitched(small.cuda()), sc, sh, out=w)
    assert int(w[0]) == max(first, int(K.bn_relu_absmax(small.cuda(), sc, sh)[0]))
    w2 = K.bn_relu_absmax(small.cuda(), sc, sh)
    _held(int(w2[0]), ref_small, 'small')
    K.bn_relu_absmax(Hd, sc, sh, out=w2)
    _held(int(w2[0]), max(ref, ref_small), 'small, then large')


@pytest.mark.gpu
def test_bn_relu_absmax_signs_and_non_finite_values():
    K = hip()
    R, Cc = 257, 208
    H, scale, shift = _bra_operands(R, Cc, 7)
    # everything negative: the word stays 0
    w = K.bn_relu_absmax(_pitched(H.abs().cuda()), (-scale.abs() - 0.1).cuda(), (-shift.abs()).cuda())
    assert int(w[0]) == 0
    # a NaN must not hide the finite maximum, wherever it sits (first element, last element, the row of the maximum)
    v = torch.relu(H.double() * scale.double() + shift.double())
    r_max = int(v.max(1).values.argmax())
    for r, c in ((0, 0), (R - 1, Cc - 1), (r_max, 3)):
        Hn = H.clone()
        Hn[r, c] = float('nan')
        ref = _bra_reference(Hn, scale, shift)
        assert ref > 0
        _held(int(K.bn_relu_absmax(_pitched(Hn.cuda()), scale.cuda(), shift.cuda())[0]), ref, f'NaN at {r, c}')
    # +inf under a positive scale: 0x7F800000; under a negative one it is relu(-inf) = 0 and the finite maximum stands
    pos, neg = int((scale > 0).nonzero()[0]), int((scale < 0).nonzero()[0])
    Hi = H.clone()
    Hi[100, pos] = float('inf')
    assert int(K.bn_relu_absmax(_pitched(Hi.cuda()), scale.cuda(), shift.cuda())[0]) == 0x7F800000
    Hi = H.clone()
    Hi[100, neg] = float('inf')
    _held(int(K.bn_relu_absmax(_pitched(Hi.cuda()), scale.cuda(), shift.cuda())[0]), _bra_reference(Hi, scale, shift), '+inf under a negative scale')
    # a pitch below the width, a width that is no multiple of 4, a misaligned operand: refused on the host
    buf, sc = torch.zeros(64, 16, device='cuda'), torch.zeros(16, device='cuda')
    words, scratch = torch.zeros(4, dtype=torch.int32, device='cuda'), torch.zeros(64, device='cuda')
    args = lambda p, ld, cc: (p, ld, 8, cc, sc.data_ptr(), sc.data_ptr(), words.data_ptr(), scratch.data_ptr(), None)  # noqa: E731
    assert K.lib.qagnn_bn_relu_absmax_f32(*args(buf.data_ptr(), 12, 16)) != 0
    assert K.lib.qagnn_bn_relu_absmax_f32(*args(buf.data_ptr(), 16, 6)) != 0
    assert K.lib.qagnn_bn_relu_absmax_f32(*args(buf.data_ptr() + 4, 16, 8)) != 0
    assert K.lib.qagnn_bn_relu_absmax_f32(*args(buf.data_ptr(), 16, 16)) == 0
    torch.cuda.synchronize()
    assert words.tolist() == [0, 0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize('nc', [2, 4, 5, 8])
@pytest.mark.parametrize('Q', [1, 7, 257])
def test_choice_eval(Q, nc):
    K = hip()
    logits, labels = _choice_case(Q, nc, 17 * Q + nc)
    want = torch.argmax(logits, dim=1)
    hits = int((want == labels).sum())
    wide = torch.full((Q, nc + 3), 9.0, device='cuda')  # (a pitched view: what sits beside a row is never read as a logit)
    wide[:, :nc] = logits.cuda()
    counts = torch.zeros(2, dtype=torch.long, device='cuda')
    pred = torch.full((Q + 8,), -7, dtype=torch.long, device='cuda')
    for i, lg in enumerate((logits.cuda(), wide[:, :nc], logits.cuda())):
        pred[:Q] = -7
        K.choice_eval(lg, labels.cuda(), counts, pred[:Q])
        assert torch.equal(pred[:Q].cpu(), want), f'call {i}'
        assert pred[Q:].tolist() == [-7] * 8, 'the canary behind pred'
    assert counts.tolist() == [3 * hits, 3 * Q]
    K.choice_eval(logits.cuda(), None, counts)          # without labels only `seen` moves
    K.choice_eval(logits.cuda(), labels.cuda(), counts)  # without pred
    assert counts.tolist() == [4 * hits, 5 * Q]


# =================================================================================================================================
# On the GPU: the inference stack at the C ABI
# =================================================================================================================================
def _tn():
    import test_nonfinite as TN
    return TN


def _stack_operands(case, dev='cuda'):
    """the operands of tests/test_nonfinite.py's hop cases on the device -> (graph, x, S, ntype, prms)"""
    TN = _tn()
    K = ops.kernels()
    ei, et, nt, R, T = case['graph']
    g = K.graph_prep(ei.to(dev), et.to(dev), nt.to(dev), R, T)
    conv = lambda t: t.to(dev)  # noqa: E731
    return g, conv(case['X']), conv(case['S']), nt.to(dev), [TN._prm(p, conv) for p in case['prms']]


def _stack_fwd_eval(K, case):
    """the existing eval forward: qagnn_stack_fwd_f32 with running statistics, a set of buffers per hop -> per hop dict(aggr, h1, out, y)"""
    g, x, S, ntype, prms = _stack_operands(case)
    k = case['k']
    y, saved = K.stack_fwd(g, case['HP'], case['qs'], x, S, ntype, prms, False, 1e-5, 0.0, [0] * k, [None] * k)
    rows, stats, KMQ = saved[2], saved[3], saved[0]
    return y, [dict(KMQ=KMQ[l], aggr=rows[l, 0], h1=rows[l, 1], out=rows[l, 2], y=rows[l, 3], stats=stats[l]) for l in range(k)], saved[4]


def _stack_infer(K, case, keep):
    g, x, S, ntype, prms = _stack_operands(case)
    res = K.stack_infer(g, case['HP'], case['qs'], x, S, ntype, prms, 1e-5, keep=keep)
    if not keep:
        return res[0], None, res[1]
    KMQ, aa, rows, stats = res[2]
    k = case['k']
    return res[0], [dict(KMQ=KMQ[l], aggr=rows[l, 0], h1=rows[l, 1], out=rows[l, 2], y=rows[l, 3], stats=stats[l]) for l in range(k)], res[1]


def _emu64(case):
    """the float64 emulation of the same stack, hop by hop"""
    TN = _tn()
    return TN.run_hops(case, TN.EMU, False, native=False)


@pytest.mark.gpu
@pytest.mark.parametrize('name,k', [('small_train', 2), ('small_train', 3), ('degree_ladder', 3)])
def test_stack_infer_with_the_form_off_is_the_stack_forward(name, k):
    """Default gate, a few hundred rows: one shared set of hop buffers and two alternating y give, bit for bit, what
    qagnn_stack_fwd_f32 (eval) gives with a set of buffers per hop -- and so does the per-hop-buffer layout of the inference call."""
    K = hip()
    case = _tn().hop_case(name, k=k)
    assert case['N'] < K.PACK_MIN_M
    y_fwd, hops_fwd, am_fwd = _stack_fwd_eval(K, case)
    y_shared, _, amax = _stack_infer(K, case, keep=False)
    y_keep, hops_keep, _ = _stack_infer(K, case, keep=True)
    assert torch.equal(y_shared, y_fwd) and torch.equal(y_keep, y_fwd)
    for l in range(k):
        for nm in ('KMQ', 'aggr', 'h1', 'out', 'y'):
            assert torch.equal(hops_keep[l][nm], hops_fwd[l][nm]), (l, nm)
        assert torch.equal(hops_keep[l]['stats'][2:], hops_fwd[l]['stats'][2:]), l  # (rows 0, 1 are not written under running statistics)


def _raw_hops(K, case, y_is_x=False, batch_stats=False, x_inside=False):
    """qagnn_hop_args of a 2-hop inference stack over canary-filled buffers, as _lib.HipKernels.stack_infer lays them out.
    x_inside: the stack input is a view INTO the shared result block, half a matrix past the start of aggr (it starts where no result
    buffer starts, and overlaps aggr and h1)"""
    g, x, S, ntype, prms = _stack_operands(case)
    N, DP, Ep = g.N, 4 * case['HP'], g.Ep
    CANARY = 7.25
    bufs = dict(KMQ=torch.full((N, 3 * DP), CANARY, device='cuda'), aa=torch.full((2, Ep, 4), CANARY, device='cuda'),
                rows=torch.full((5, N, DP), CANARY, device='cuda'), stats=torch.full((5, DP), CANARY, device='cuda'),
                amax=torch.full((2, _lib.HOP_AMAX_WORDS), 12345, dtype=torch.int32, device='cuda'),
                ws=torch.full((K.lib.qagnn_hop_fwd_workspace_elems(N, Ep, DP),), CANARY, device='cuda'))
    hops = (_lib.qagnn_hop_args * 2)()
    xin = bufs['rows'].view(-1)[N * DP // 2:N * DP // 2 + N * DP].view(N, DP) if x_inside else x
    for l in range(2):
        h = K._hop_struct(g, case['HP'], case['qs'], xin, S, ntype, prms[l], batch_stats and l == 1, 1e-5, 0.0, 0, True, -1, running=None)
        K._set_saved(h, bufs['KMQ'].data_ptr(), bufs['aa'].data_ptr(), bufs['rows'].data_ptr(), bufs['stats'].data_ptr(),
                     bufs['amax'].data_ptr() + l * _lib.HOP_AMAX_WORDS * 4, Ep, N * DP * 4)
        y = bufs['rows'][3 + l]
        h.y = xin.data_ptr() if (y_is_x and l == 1) else y.data_ptr()
        h.ws, h.ws_elems = bufs['ws'].data_ptr(), bufs['ws'].numel()
        hops[l] = h
        xin = y
    keep = (g, x, S, ntype, prms)
    return hops, bufs, CANARY, keep


@pytest.mark.gpu
@pytest.mark.parametrize('fault', ['y_is_x', 'batch_stats', 'x_inside'])
def test_stack_infer_refuses_before_the_first_enqueue(fault):
    K = hip()
    case = _tn().hop_case('small_train', k=2)
    hops, bufs, canary, keep = _raw_hops(K, case, y_is_x=fault == 'y_is_x', batch_stats=fault == 'batch_stats', x_inside=fault == 'x_inside')
    x_before = keep[1].clone()
    rc = K.lib.qagnn_stack_infer_f32(hops, 2, None)
    torch.cuda.synchronize()
    assert rc != 0, K.lib.qagnn_last_error()
    for nm in ('KMQ', 'aa', 'rows', 'stats', 'ws'):
        assert bool((bufs[nm] == canary).all()), f'{nm} was written by a refused call'
    assert bool((bufs['amax'] == 12345).all()) and torch.equal(keep[1], x_before)
    # (the same blocks, untampered, run)
    hops, bufs, canary, keep = _raw_hops(K, case)
    assert K.lib.qagnn_stack_infer_f32(hops, 2, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(bufs['rows'][4], _stack_fwd_eval(K, case)[0])


def _row_dev(got, ref):
    """helpers.HIDDEN_RTOL's statistic: per row, rms_c(ref - got) over the row's own scale rms_c(ref) + 1; rows finite on both sides"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    ok = torch.isfinite(got).all(1) & torch.isfinite(ref).all(1)
    d = (got[ok] - ref[ok]).pow(2).mean(1).sqrt() / (ref[ok].pow(2).mean(1).sqrt() + 1.0)
    return float(d.max()) if d.numel() else 0.0


def _hidden(h):
    """the BatchNorm output of every element: h1 * scale + shift"""
    return h['h1'].double().cpu() * h['stats'][3].double().cpu() + h['stats'][4].double().cpu()


def _wf(w):
    return torch.tensor([int(w)], dtype=torch.int32).view(torch.float32).item()


def _tbits(t):
    return t.detach().abs().max().cpu().view(torch.int32).item()


@pytest.mark.gpu
def test_operand_maxima_of_the_inference_stack_are_the_true_maxima(monkeypatch):
    """Form on (form_everywhere, 329 rows x 208 columns, 3 hops, a set of buffers per hop so that h1 survives): the words of X, S, aggr
    and y are the tensors' maxima bit for bit; the h1 word is the maximum of relu(bn(h1)) at the bar of the kernel's own test."""
    K = hip()
    case = _tn().hop_case('degree_ladder', k=3)
    with helpers.form_everywhere():
        monkeypatch.setattr(K, 'gemm_split', 2)
        y, hops, amax = _stack_infer(K, case, keep=True)
        monkeypatch.setattr(K, 'gemm_split', 1)
        y1, _, _ = _stack_infer(K, case, keep=True)
    assert not torch.equal(y, y1), 'bit-identical to the exact products: the three-MFMA form did not run'
    w = amax.cpu()
    assert w[0, AM_X].item() == _tbits(case['X']) and w[0, AM_S].item() == _tbits(case['S'])
    for l in range(3):
        assert w[l, AM_AGGR].item() == _tbits(hops[l]['aggr']), f'hop {l}: aggr word'
        assert w[l, AM_Y].item() == _tbits(hops[l]['y']), f'hop {l}: y word'
        st = hops[l]['stats'].cpu()
        _held(w[l, AM_H1].item(), _bra_reference(hops[l]['h1'], st[3], st[4]), f'hop {l}: h1 word')
        if l:
            assert w[l, AM_X].item() == 0 and w[l, AM_S].item() == 0  # (read from the chain: hop l - 1's y word, hop 0's S word)


def _big_case(k, seed=5):
    """41 subgraphs x 200 node slots = 8 200 rows (the default gate opens at 8 192), d = 200 (DP = 208), as the hop cases of
    tests/test_nonfinite.py are made"""
    B, n, HP, T, R = 41, 200, 52, 4, 38
    recs = synthetic.make_records(B, seed=seed, shape='csqa', n_rel=17, n_concept_vocab=2000)
    _, cids, nt, ns, al, ei, et, _ = data_utils.records_to_tensors(recs, n, 1)
    ei, et = data_utils.batch_graph(ei, et, n)
    nt = nt.reshape(-1)
    gen = torch.Generator().manual_seed(seed)
    N, DP, C, SP = B * n, 4 * HP, R * T * T + T, 112
    rnd = lambda *shape, s=0.3: torch.randn(*shape, generator=gen) * s  # noqa: E731
    prms = []
    for _ in range(k):
        Wx_t, Ws_t, W1t, W2t = rnd(DP, 3 * DP, s=0.1), rnd(SP, 3 * DP, s=0.1), rnd(DP, DP, s=0.1), rnd(DP, DP, s=0.1)
        prms.append([Wx_t, None, Ws_t, None, rnd(T, 3 * DP), rnd(C, 2 * DP), W1t, None, rnd(DP), 1 + rnd(DP), rnd(DP), W2t, None, rnd(DP),
                     rnd(DP), 0.5 + rnd(DP).abs()])
    return dict(name='gate', HP=HP, qs=1.0 / (50 ** 0.5), graph=(ei, et, nt, R, T), prms=prms, X=rnd(N, DP, s=1.0), S=rnd(N, SP, s=1.0), N=N, DP=DP, k=k)


_GATE_CASE = dict(shape='csqa', nq=41, nc=1, n=200, n_rel=17, std=0.6, train=False, seed=45,
                  cfg=helpers.model_cfg(d=200, k=2, sent_dim=64, n_concept=2000, concept_in_dim=32))


def _gate_model():
    from qagnn_amd import modeling_qagnn as MQ
    cfg = _GATE_CASE['cfg']
    torch.manual_seed(0)
    model = MQ.QAGNN(None, cfg['k'], cfg['n_ntype'], cfg['n_etype'], cfg['sent_dim'], cfg['n_concept'], cfg['concept_dim'], cfg['concept_in_dim'],
                     cfg['n_attention_head'], cfg['fc_dim'], cfg['n_fc_layer'], 0.0, 0.0, 0.0, init_range=cfg['init_range'])
    helpers.det_fill_(model, _GATE_CASE['seed'], _GATE_CASE['std'])
    return model.eval()


class _KeepEmu(EmuInferKernels):
    """the emulation, keeping every hop's buffers of its inference stack"""

    def stack_infer(self, *a, **kw):
        y, amax, self.kept = super().stack_infer(*a, **dict(kw, keep=True))
        return y, amax


@pytest.mark.gpu
def test_inference_stack_at_the_size_where_the_default_gate_opens(monkeypatch):
    """N = 8 200 rows (41 subgraphs x 200 slots), d = 200, k = 2, the library's default threshold, the deterministic fill of the golden
    cases: the form is on (the result differs from the switch-off forward's exact products), and the hidden BatchNorm outputs and y of
    every node row of both hops are within helpers.HIDDEN_RTOL of the float64 emulation of the same module -- the bar the train-mode form
    is held to.  Measured (MI355X, profiles/inference_path_gpu_tests.txt): hidden 3.5e-5 / 4.4e-5, y 1.7e-5 / 1.8e-5 at hops 0 / 1."""
    K = hip()
    assert K.PACK_MIN_M == 8192 and K.gemm_split == 2
    c = _GATE_CASE
    x = helpers.make_case_inputs(c)
    B, n = c['nq'] * c['nc'], c['n']
    args = [x['sent_vecs'], x['concept_ids'].view(B, n), x['node_type_ids'].view(B, n), x['node_scores'].view(B, n, 1), x['adj_lengths'].view(B)]
    adj = (x['edge_index'], x['edge_type'])
    assert B * n == 8200
    # float64, on the emulation (the model is filled in fp32, like the one on the GPU, then widened)
    ref_model = _gate_model().double()
    torch.set_default_dtype(torch.float64)
    try:
        with provider(_KeepEmu()) as E, torch.no_grad(), ops.inference_path():
            ref_logits, _ = ref_model(args[0].double(), args[1], args[2], args[3].double(), args[4], adj)
            ref = E.kept
    finally:
        torch.set_default_dtype(torch.float32)
    ops.set_kernels(K)
    kept = []
    orig = K.stack_infer

    def spy(*a, **kw):
        y, amax, saved = orig(*a, **dict(kw, keep=True))
        kept.append((amax, saved))
        return y, amax

    monkeypatch.setattr(K, 'stack_infer', spy)
    model = _gate_model().cuda()
    dargs, dadj = cu(*args), tuple(cu(*adj))
    with torch.no_grad(), ops.inference_path():
        logits, _ = model(*dargs, dadj)
    with torch.no_grad():
        logits_off, _ = model(*dargs, dadj)
    assert len(kept) == 1 and not torch.equal(logits, logits_off), 'the three-MFMA form did not run at 8 200 rows'
    amax, (KMQ, aa, rows, stats) = kept[0]
    worst = 0.0
    for l in range(2):
        assert amax[l, AM_H1].item() != 0 and amax[l, AM_Y].item() == _tbits(rows[l, 3])
        hid = _hidden(dict(h1=rows[l, 1], stats=stats[l]))
        ref_hid = ref[l]['h1'] * ref[l]['stats'][3] + ref[l]['stats'][4]
        dev_h, dev_y = _row_dev(hid, ref_hid), _row_dev(rows[l, 3], ref[l]['y'])
        note(f'inference stack, N = 8200, d = 200, hop {l}: worst row deviation from float64: hidden {dev_h:.2e}, y {dev_y:.2e} (bar {helpers.HIDDEN_RTOL:g})')
        worst = max(worst, dev_h, dev_y)
    dl = (logits.cpu().double() - ref_logits).abs().max().item() / ref_logits.abs().max().item()
    note(f'inference stack, N = 8200, d = 200: logits {dl:.2e} of scale from float64 (switch off: '
         f'{(logits_off.cpu().double() - ref_logits).abs().max().item() / ref_logits.abs().max().item():.2e})')
    assert worst <= helpers.HIDDEN_RTOL, worst


@pytest.mark.gpu
def test_inference_stack_non_finite_inputs(monkeypatch):
    """One NaN and one +inf in X through the inference stack with the form on: non-finite where the float64 emulation puts them (an inf
    may turn into a NaN inside a split product, so the emulation's set is a lower bound: tests/test_nonfinite.py, `superset`), and every
    row that is finite on both sides stays inside the bar of the test above."""
    TN = _tn()
    K = hip()
    case = TN.hop_case('degree_ladder', k=3)
    pc = TN.poisoned(case, 'none', 0.0)
    pc['X'][case['node'], 3] = float('nan')
    other = (case['node'] + 17) % case['N']
    pc['X'][other, 5] = float('inf')
    ref = _emu64(pc)
    with helpers.form_everywhere():
        monkeypatch.setattr(K, 'gemm_split', 2)
        y, hops, amax = _stack_infer(K, pc, keep=True)
        y_shared, _, _ = _stack_infer(K, pc, keep=False)
    n = TN.check_hops('inference stack [X: one NaN, one +inf]', hops, ref, False, superset=True)
    assert n > 0
    bad_rows = [int((~torch.isfinite(r['y'])).any(1).sum()) for r in ref]
    assert 0 < bad_rows[0] <= bad_rows[1] <= bad_rows[2] and bad_rows[0] < case['N'], bad_rows
    assert torch.equal(torch.isfinite(y_shared), torch.isfinite(y))
    for l in range(3):
        assert _row_dev(hops[l]['y'], ref[l]['y']) <= helpers.HIDDEN_RTOL, l
        assert _row_dev(_hidden(hops[l]), ref[l]['h1'] * ref[l]['stats'][3] + ref[l]['stats'][4]) <= helpers.HIDDEN_RTOL, l


@pytest.mark.gpu
def test_inference_stack_peak_memory():
    """N = 8 200, k = 5: the peak of the inference stack call is below half of the peak of the existing eval forward (a condition, from
    the buffer counts -- 8 against 35 [N, DP] matrices -- the ratio should be near 0.3)."""
    K = hip()
    case = _big_case(5)
    g, x, S, ntype, prms = _stack_operands(case)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        del out
        return p

    p_fwd = peak(lambda: K.stack_fwd(g, case['HP'], case['qs'], x, S, ntype, prms, False, 1e-5, 0.0, [0] * 5, [None] * 5))
    p_inf = peak(lambda: K.stack_infer(g, case['HP'], case['qs'], x, S, ntype, prms, 1e-5))
    note(f'peak memory, N = 8200, k = 5: stack forward (eval) {p_fwd / 2 ** 20:.1f} MiB, inference stack {p_inf / 2 ** 20:.1f} MiB, ratio {p_inf / p_fwd:.3f}')
    assert p_inf < 0.5 * p_fwd, (p_inf, p_fwd)


# =================================================================================================================================
# On the GPU: the module, GraphedForward, evaluate_accuracy
# =================================================================================================================================
def cu(*ts):
    return [t.cuda() for t in ts]


@pytest.mark.gpu
@pytest.mark.parametrize('case', EVAL_CASES)
def test_the_inference_path_takes_the_three_mfma_form(case, monkeypatch):
    """THE test that fails without the feature.  Under form_everywhere, the module forward inside inference_path() + no_grad with
    gemm_split = 2 against 1: both within the fixtures' forward bars (logits, pool_attn, mp_out) and NOT bit-identical -- the stack ran
    the form under running statistics.  With the switch off the stack forward IS bit-identical between the two: the existing contract
    (tests/test_hip_parity.py, test_the_three_mfma_form_runs_where_the_threshold_lets_it: mp_out), restated.  (The whole model's
    logits are not part of that contract: its input stage takes the form from the entity table's maximum, batch statistics or not.)"""
    fix = helpers.load_golden(case)
    c = helpers.GOLDEN_CASES[case]
    with helpers.form_everywhere() as K:
        out = {}
        for switch in (True, False):
            for mode in (2, 1):
                monkeypatch.setattr(K, 'gemm_split', mode)
                model = build(case).cuda()
                sv, cids, nt, ns, al, ei, et = cu(*golden_inputs(case, fix))
                H, nsc, _, _ = helpers.mp_inputs(case)
                nsc = nsc * (torch.arange(c['n']) < al.cpu().unsqueeze(1)).float().unsqueeze(2)
                with torch.no_grad(), ops.inference_path(switch):
                    logits, pool_attn = model(sv, cids, nt, ns, al, (ei, et))
                    y = model.gnn(H.cuda(), (ei, et), nt, nsc.cuda())
                helpers.check_plain(fix, 'logits', logits, **FWD)
                helpers.check_plain(fix, 'pool_attn', pool_attn, **FWD)
                helpers.check_stored(fix, 'mp_out', y, **FWD)
                out[switch, mode] = (logits, y)
    assert torch.equal(out[False, 2][1], out[False, 1][1]), 'switch off: the stack forward took the three-MFMA form without batch statistics'
    assert torch.equal(out[True, 1][0], out[False, 1][0]) and torch.equal(out[True, 1][1], out[False, 1][1]), \
        'gemm_split = 1: the inference stack must equal the stack forward'
    assert not torch.equal(out[True, 2][1], out[True, 1][1]), 'mp_out bit-identical: the three-MFMA form did not run on the inference path'
    assert not torch.equal(out[True, 2][0], out[True, 1][0]), 'logits bit-identical: the three-MFMA form did not run on the inference path'


def _gf_model(p=0.0):
    import test_graphed as TG
    return TG._model(p)


def _gf_batches(nq, nc, n, seeds):
    """batches out of ONE blob store (so that a device store can name them by sample ids) -> (host store, device store, [batch dicts])"""
    per = nq * nc
    recs = []
    for s in seeds:
        recs += synthetic.make_records(per, seed=s, shape='csqa', n_rel=17, n_concept_vocab=2000)
    _, cids, nt, ns, al, ei, et, _ = data_utils.records_to_tensors(recs, n, nc)
    store = data_utils.GraphBlobStore.build(ei, et, nt, 38, 4)
    S = len(seeds) * per
    cids, nt, ns, al = cids.view(S, n), nt.view(S, n), ns.view(S, n, 1), al.view(S)
    dstore = data_utils.DeviceGraphStore.from_host(store, cids, nt, ns, al, 'cuda')
    out = []
    for i, s in enumerate(seeds):
        ids = list(range(i * per, (i + 1) * per))
        buf, B, E = store.pack(ids)
        g = torch.Generator().manual_seed(s)
        sl = slice(i * per, (i + 1) * per)
        out.append(dict(sent=torch.randn(per, 64, generator=g).cuda(), cids=cids[sl].cuda(), nt=nt[sl].cuda(), ns=ns[sl].cuda(), al=al[sl].cuda(),
                        labels=torch.randint(0, nc, (nq,), generator=g).cuda(), ids=ids,
                        packed=data_utils.PackedGraphBatch(buf.cuda(), B, E, store, ids, nc)))
    return store, dstore, out


def _holder(kind, b, dstore, nc):
    """-> (the four node tensors or Nones, the graph input) of batch b as one of the four kinds GraphedStep accepts"""
    fields = (b['cids'], b['nt'], b['ns'], b['al'])
    if kind == 'blobs':
        return fields, b['packed']
    if kind == 'store':
        return (None,) * 4, dstore.batch(b['ids'], nc)
    ei, et = b['packed'].batched(device='cuda')
    return fields, (data_utils.EdgeListBatch(ei, et) if kind == 'edge lists' else (ei, et))


def _state(model):
    return ({k: v.clone() for k, v in model.named_buffers()}, ops._seed_counter[0], {k: p.grad for k, p in model.named_parameters()},
            {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['blobs', 'edge lists', 'pair', 'store'])
def test_graphed_forward_equals_the_eager_inference_forward(kind):
    """Three different batches in one capacity bucket: logits bit-identical to the eager inference forward, one capture, the device
    counters equal the Python count; BatchNorm buffers, batch counters, the seed counter and every .grad as they were."""
    ops.set_kernels(None)
    _lib.ERR_WATCH.poll(block=True)
    nq, nc, n = 2, 5, 200
    _, dstore, batches = _gf_batches(nq, nc, n, (3, 4, 5))
    cap = max(graphed.edge_capacity(b['packed'].E) for b in batches)
    m_eager, m = _gf_model().eval(), _gf_model()
    # (a .grad on every parameter and moved BatchNorm buffers: what the forward must leave alone)
    b0 = batches[0]
    logits, _ = m(b0['sent'], b0['cids'], b0['nt'], b0['ns'], b0['al'], b0['packed'])
    logits.sum().backward()
    m.eval()
    m_eager.load_state_dict(m.state_dict())
    before = _state(m)
    fwd = inference.GraphedForward(m, nc, capacity=lambda E: cap)
    hits = 0
    for i, b in enumerate(batches):
        fields, adj = _holder(kind, b, dstore, nc)
        got = fwd(b['sent'], *fields, adj, labels=b['labels']).clone()
        with torch.no_grad(), ops.inference_path():
            want, _ = m_eager(b['sent'], b['cids'], b['nt'], b['ns'], b['al'], b['packed'])
        assert torch.equal(got, want), f'batch {i}: logits differ by {(got - want).abs().max().item():.3e}'
        hits += int((want.view(-1, nc).argmax(1) == b['labels']).sum())
    assert fwd.n_graphs == 1
    assert fwd.counts() == (hits, nq * len(batches))
    fwd.reset_counts()
    assert fwd.counts() == (0, 0)
    after = _state(m)
    assert all(torch.equal(before[0][k], after[0][k]) for k in before[0]), 'a buffer moved'
    assert before[1] == after[1], 'a dropout seed was drawn'
    assert all(before[2][k] is after[2][k] for k in before[2]) and all(torch.equal(before[3][k], after[3][k]) for k in before[3]), 'a .grad moved'
    m.train()
    with pytest.raises(RuntimeError, match='eval'):
        fwd(b0['sent'], *_holder(kind, b0, dstore, nc)[0], _holder(kind, b0, dstore, nc)[1])
    torch.cuda.synchronize()
    _lib.ERR_WATCH.poll(block=True)


@pytest.mark.gpu
def test_graphed_forward_between_training_replays():
    """GraphedStep replay, two GraphedForward replays, a second training replay == the two training replays alone (dropout on: the
    seed epoch must have advanced equally): logits, loss, every gradient, every buffer."""
    ops.set_kernels(None)
    nc = 5
    _, _, batches = _gf_batches(2, nc, 200, (21, 22))
    res = []
    for with_eval in (True, False):
        ops.manual_seed(5)
        m = _gf_model(0.2)
        step = graphed.GraphedStep(m, nc)
        fwd = inference.GraphedForward(m, nc)
        outs = []
        for i, b in enumerate(batches):
            m.train()
            logits, loss = step(b['sent'], b['cids'], b['nt'], b['ns'], b['al'], b['packed'], b['labels'])
            outs.append((logits.clone(), loss.clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None},
                         {k: v.clone() for k, v in m.named_buffers()}))
            if with_eval and i == 0:
                m.eval()
                for bb in batches:
                    ev = fwd(bb['sent'], bb['cids'], bb['nt'], bb['ns'], bb['al'], bb['packed'], labels=bb['labels'])
                assert torch.isfinite(ev).all() and fwd.counts()[1] == 4
        res.append(outs)
    for i in range(2):
        (la, sa, ga, ba), (lb, sb, gb, bb_) = res[0][i], res[1][i]
        assert torch.equal(la, lb) and torch.equal(sa, sb), f'training replay {i}: logits / loss'
        assert not [k for k in ga if not torch.equal(ga[k], gb[k])], f'training replay {i}: gradients'
        assert not [k for k in ba if not torch.equal(ba[k], bb_[k])], f'training replay {i}: buffers'
    torch.cuda.synchronize()
    _lib.ERR_WATCH.poll(block=True)


@pytest.mark.gpu
def test_graphed_forward_corrupt_batch_raises_one_call_late():
    ops.set_kernels(None)
    _lib.ERR_WATCH.poll(block=True)
    _, _, (good,) = _gf_batches(2, 5, 200, (11,))
    m = _gf_model().eval()
    fwd = inference.GraphedForward(m, 5)
    call = lambda b: fwd(b['sent'], b['cids'], b['nt'], b['ns'], b['al'], b['packed'])  # noqa: E731
    call(good)
    bad = dict(good, cids=good['cids'].clone())
    bad['cids'][3, 7] = 10 ** 6
    call(bad)  # clamped on the device, flagged
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='out-of-range input'):
        call(good)
    _lib.ERR_WATCH.poll(block=True)  # nothing left over
    call(good)
    torch.cuda.synchronize()
    _lib.ERR_WATCH.poll(block=True)


@pytest.mark.gpu
@pytest.mark.parametrize('graphed_', [False, True], ids=['eager', 'graphed'])
def test_evaluate_accuracy(graphed_):
    """six batches, the last one ragged, labels the model gets right for every second question: the fraction equals the reference
    loop's exactly (6 / 11).  Graphed: a GraphedForward kept by the caller serves a second pass without a new capture."""
    ops.set_kernels(None)
    nc = 5
    cfg = helpers.model_cfg(d=200, k=5, sent_dim=64, n_concept=2000, concept_in_dim=32)
    m = _gf_model()
    es = _half_right(_eval_set([2, 2, 2, 2, 2, 1], nc, 200, cfg, 'csqa', device='cuda'), m, nc)
    got = inference.evaluate_accuracy(es, m.train(), graphed=graphed_)
    assert not m.training
    n_correct, n_samples = _reference_accuracy(es, m, nc)
    assert (n_correct, n_samples) == (6, 11) and got == n_correct / n_samples
    note(f'evaluate_accuracy ({"graphed" if graphed_ else "eager"}): {n_correct} / {n_samples}')
    if graphed_:
        fwd = inference.GraphedForward(m, nc)
        assert inference.evaluate_accuracy(es, m, graphed=fwd) == got
        n = fwd.n_graphs
        assert inference.evaluate_accuracy(es[:3], m, graphed=fwd) == sum(int((b[1] == _pred(m, b, nc)).sum()) for b in es[:3]) / 6
        assert fwd.n_graphs == n, 'the second pass captured again'


def _pred(model, batch, nc):
    with torch.no_grad():
        return model(*batch[2:])[0].view(-1, nc).argmax(1)


@pytest.mark.gpu
@pytest.mark.parametrize('case', EVAL_CASES)
def test_small_eval_batches_on_the_inference_path_are_the_parent_forward_bit_for_bit(case, monkeypatch):
    """The configuration every small eval batch meets: switch on, the default row gate, the default gemm_split = 2, N < 8 192 -- the
    form is off, the inference stack runs on ONE shared set of hop buffers.  small_eval and trunc_eval (truncated subgraphs): mp_out,
    logits and pool_attn equal the forward with the switch off bit for bit, and so does stack_infer against qagnn_stack_fwd_f32 on the
    very operands the module handed the stack."""
    K = hip()
    fix = helpers.load_golden(case)
    c = helpers.GOLDEN_CASES[case]
    assert K.gemm_split == 2 and K.PACK_MIN_M == 8192 > c['nq'] * c['nc'] * c['n']
    calls, orig_f, orig_i = [], K.stack_fwd, K.stack_infer

    def spy_f(*a, **kw):
        y, saved = orig_f(*a, **kw)
        calls.append(('stack_fwd', a, kw, y))
        return y, saved

    def spy_i(*a, **kw):
        calls.append(('stack_infer', a, kw, None))
        return orig_i(*a, **kw)

    monkeypatch.setattr(K, 'stack_fwd', spy_f)
    monkeypatch.setattr(K, 'stack_infer', spy_i)
    model = build(case).cuda()
    sv, cids, nt, ns, al, ei, et = cu(*golden_inputs(case, fix))
    H, nsc, _, _ = helpers.mp_inputs(case)
    nsc = (nsc * (torch.arange(c['n']) < al.cpu().unsqueeze(1)).float().unsqueeze(2)).cuda()
    out = {}
    for switch in (False, True):
        with torch.no_grad(), ops.inference_path(switch):
            logits, pool_attn = model(sv, cids, nt, ns, al, (ei, et))
            y = model.gnn(H.cuda(), (ei, et), nt, nsc)
        out[switch] = (logits, pool_attn, y)
    assert [x[0] for x in calls] == ['stack_fwd'] * 2 + ['stack_infer'] * 2
    for nm, a, b in zip(('logits', 'pool_attn', 'mp_out'), out[False], out[True]):
        assert torch.equal(a, b), f'{nm}: the inference path differs from the forward as it was by {(a - b).abs().max().item():.3e}'
    helpers.check_plain(fix, 'logits', out[True][0], **FWD)
    helpers.check_stored(fix, 'mp_out', out[True][2], **FWD)
    # the stack alone, on the operands of the switch-off forward: (graph, HP, qscale, X, S, ntype, prms, batch_stats, eps, p, seeds, runnings, cols)
    for _, a, kw, y_fwd in calls[:2]:
        assert a[7] is False and a[9] == 0.0
        y_inf, _ = orig_i(*a[:7], a[8], a[12], **kw)
        assert torch.equal(y_inf, y_fwd)
