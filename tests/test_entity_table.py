"""A TRAINABLE entity table on the fused input stage (include/qagnn_hip_rows.h): QAGNN(..., freeze_ent_emb=False).

The table's gradient is the transpose of a gather in which ids repeat heavily; the library groups the positions by row id
(qagnn_row_groups), sums the gradient rows of each group in a fixed order (qagnn_row_segment_sum_f32), projects the U group sums with
the existing product and scatters the rows into a zeroed dense gradient (qagnn_rows_scatter_f32).

  `-m "not gpu"`  symbols, constants and the build hash; the oracle's table gradient against the REFERENCE's (tests/golden/
                  entity_table.npz, written by tests/golden/make_golden_entity_table.py); the module on the emulation (tests/emu_rows.py)
                  against the float64 yardstick; the path taken; the comparison rejects three stand-ins that are right on a batch
                  without repeated ids.
  `-m gpu`        the grouping bit for bit against a numpy sort; segment sums and scatter against float64 under the header's bound and
                  bit for bit against a numpy twin that adds in the stated order; refusals; history-free outputs; the module against the
                  float64 oracle and the reference fixture; the path taken; a replayed training run, bit for bit against the eager one.
"""
import copy
import math
import os
import re

import numpy as np
import pytest
import torch

import helpers
from emu_rows import EmuRowKernels
from qagnn_amd import _lib, build, ops
from qagnn_amd import modeling_qagnn as MQ

TABLE = 'concept_emb.emb.weight'
ROW_METHODS = ('row_groups', 'row_segment_sum', 'rows_scatter')
BWD = dict(rtol=5e-3, atol=1e-5)  # (tests/test_host_logic_emu.py: gradients against the reference's fixtures)
U32, EPS32 = 2.0 ** -24, 2.0 ** -23


def note(line):
    print(line)


@pytest.fixture(autouse=True)
def _leave_the_seed_counter_where_it_was():
    """ops.next_seed() counts calls per process, and the dropout masks of every later test follow from the count: the tests of this file
    that draw seeds hand the counter back as they found it (as tests/test_dropout_masks.py does), so that the files behind this one see
    the masks they saw before it existed."""
    before = ops._seed_counter[0]
    yield
    ops._seed_counter[0] = before


def _source(*parts):
    with open(os.path.join(helpers.ROOT, *parts)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r'#define\s+' + name + r'\s+\(?([0-9x<\s]+?)\)?\s*(/\*|//|$)', text, re.M)
    assert m, name
    return int(eval(m.group(1)))  # ("64", "(1 << 20)")


HEADER = _source('include', 'qagnn_hip_rows.h')
ROWS_HIP = _source('qagnn_amd', 'csrc', 'rows.hip')
CHUNK = _define(HEADER, 'QAGNN_ROWS_CHUNK')
MAX_N, MAX_TABLE = _define(HEADER, 'QAGNN_ROWS_MAX_N'), _define(HEADER, 'QAGNN_ROWS_MAX_TABLE')
RG_BITS, RG_BLK, RG_SCAN_ITEMS, RS_WAVES = (_define(ROWS_HIP, n) for n in ('RG_BITS', 'RG_BLK', 'RG_SCAN_ITEMS', 'RS_WAVES'))


# ---- without a GPU: symbols and constants -----------------------------------------------------------------------------------------------------
def test_the_header_declares_exactly_the_row_exports_and_the_build_hash_covers_it():
    declared = re.findall(r'^(?:int|int64_t)\s+(qagnn_\w+)\s*\(', HEADER, re.M)
    assert sorted(declared) == sorted(_lib.EXPORTS_ROWS) and len(set(declared)) == len(declared)
    assert re.search(r'int qagnn_rows_version\(void\)\s*{\s*return 1;\s*}', ROWS_HIP)
    hashed = [os.path.basename(p) for p in build.hashed_files()]
    assert 'qagnn_hip_rows.h' in hashed and 'rows.hip' in hashed and 'rows.hip' in build.SOURCES
    assert CHUNK == _lib.ROWS_CHUNK == 64 and (MAX_N, MAX_TABLE) == (_lib.ROWS_MAX_N, _lib.ROWS_MAX_TABLE)
    assert re.search(r'static_assert\(QAGNN_ROWS_CHUNK == 64', ROWS_HIP), 'csrc/ pins the constant it was written for'
    assert MAX_TABLE <= (1 << RG_BITS) ** 2 and MAX_N >= 1 << 20 and MAX_TABLE >= 1 << 26
    # the other extension headers and the ABI number stand where they stood
    assert (len(_lib.EXPORTS_TN), len(_lib.EXPORTS_INFER), len(_lib.EXPORTS_LOSS), len(_lib.EXPORTS_EXPLAIN), len(_lib.EXPORTS_DEFER)) == (4, 5, 3, 3, 3)
    assert _lib.ABI_VERSION == 25 and not set(_lib.EXPORTS_ROWS) & set(_lib.EXPORTS)
    for m in ROW_METHODS:
        assert callable(getattr(_lib.HipKernels, m))
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load_library()
        assert lib.qagnn_rows_version() == 1 and all(hasattr(lib, s) for s in _lib.EXPORTS_ROWS)
        assert lib.qagnn_row_groups_workspace_elems(0) == 0 and lib.qagnn_row_groups_workspace_elems(MAX_N + 1) == 0


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------------
def trainable_case(case):
    c = copy.deepcopy(helpers.GOLDEN_CASES[case] if isinstance(case, str) else case)
    c['cfg']['freeze_ent_emb'] = False
    return c


def repeat_share(concept_ids):
    """the share of the non-context positions whose id an earlier position of the batch carries too"""
    ids = concept_ids[:, 1:].reshape(-1)
    return 1.0 - ids.unique().numel() / ids.numel()


def _unfrozen(orig):
    def make(case_dict, device, ps=None):
        model = orig(case_dict, device, ps)
        model.concept_emb.emb.weight.requires_grad_(True)
        return model
    return make


class CallCounter:
    """Kernel-provider proxy (ops.set_kernels): counts the calls of every method; the calls run unchanged"""

    def __init__(self, inner):
        self._inner, self.name, self.counts = inner, inner.name, {}

    def __getattr__(self, attr):
        fn = getattr(self._inner, attr)
        if not callable(fn):
            return fn

        def counted(*a, **kw):
            self.counts[attr] = self.counts.get(attr, 0) + 1
            return fn(*a, **kw)
        return counted


# The module cases.  small_train and config1_train are the shapes of the reference fixture (entity_table.npz); in config1_train and in
# sapbert_b4 as the golden cases draw them only a fifth of the non-context positions repeat an id (0.20, 0.23), so the cases held to the
# float64 oracle on the GPU are small_train (0.79) and the same two shapes with more questions, at which a third and more repeat:
MODULE_CASES = {
    'small_train': 'small_train',
    'config1_x2': dict(helpers.GOLDEN_CASES['config1_train'], nq=2),
    'sapbert_x3': dict(helpers.GOLDEN_CASES['sapbert_b4'], nq=3,
                       cfg=helpers.model_cfg(d=200, k=2, n_etype=34, sent_dim=768, n_concept=3000, concept_in_dim=768)),
}


def module_vs_oracle(case, device, monkeypatch, dropout=None, trainable=True, min_share=1.0 / 3.0):
    """test_hip_parity.oracle_vs_package with the table trainable on both sides -> (report, model, inputs)"""
    import test_hip_parity as T
    c = trainable_case(case) if trainable else copy.deepcopy(helpers.GOLDEN_CASES[case] if isinstance(case, str) else case)
    if trainable:
        monkeypatch.setattr(T, '_package_model', _unfrozen(T._package_model))
    args, _ = T._case_args(c)
    assert repeat_share(args[1]) >= min_share, f'only {repeat_share(args[1]):.2f} of the non-context positions repeat an id'
    seen = {}
    report = T.oracle_vs_package(c, device=device, dropout=dropout, seen=seen)
    assert (TABLE in report) == trainable
    return report, seen['model'], args


def check_table_gradient(model, args, case=None):
    """rows no node names are exactly 0; for a fixture case: the gradient against the reference's"""
    g = model.concept_emb.emb.weight.grad.detach().cpu()
    named = torch.zeros(g.size(0), dtype=torch.bool)
    named[(args[1][:, 1:] - 1).reshape(-1)] = True
    assert bool((g[~named] == 0).all()) and int((~named).sum()) > 0, 'a table row no node names has a gradient'
    assert bool((g[named].abs().sum(1) > 0).any())
    if case is not None:
        fix = helpers.load_golden('entity_table')
        worst = helpers._close(g, torch.from_numpy(fix[f'{case}::grad::{TABLE}']), what=f'{case} table gradient vs the reference', **BWD)
        note(f'FIGURE entity table {case}: table gradient within {worst:.2e} of the reference fixture (scale {float(g.abs().max()):.2e})')


# ---- without a GPU: the oracle against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['small_train', 'config1_train'])
def test_oracle_table_gradient_matches_the_reference(case):
    fix = helpers.load_golden('entity_table')
    c = trainable_case(case)
    B = c['nq'] * c['nc']
    model = helpers.build_oracle(c)
    assert model.concept_emb.emb.weight.requires_grad
    sv, cids, nt, ns, al, ei, et = helpers.golden_inputs(case, helpers.load_golden(case))
    logits, _ = model(sv, cids, nt, ns, al, (ei, et))
    (logits * torch.linspace(0.5, 1.5, B).view(B, 1)).sum().backward()
    torch.testing.assert_close(logits.detach(), torch.from_numpy(fix[case + '::logits']), rtol=1e-5, atol=1e-5)
    for name in (TABLE, 'concept_emb.cpt_transform.weight'):
        g = dict(model.named_parameters())[name].grad
        helpers._close(g, torch.from_numpy(fix[f'{case}::grad::{name}']), rtol=1e-4, atol=1e-5, what=f'{case} {name}')


# ---- without a GPU: the module on the emulation -------------------------------------------------------------------------------------------------
@pytest.fixture
def emu():
    old = ops.set_kernels(EmuRowKernels())
    yield ops.kernels()
    ops.set_kernels(old)


@pytest.mark.parametrize('case', ['small_train', 'config1_train'])
def test_module_on_the_emulation_meets_the_float64_yardstick(case, emu, monkeypatch):
    report, model, args = module_vs_oracle(case, 'cpu', monkeypatch, min_share=0.2)
    check_table_gradient(model, args, case)
    note(f'FIGURE entity table emulation {case}: {len(report)} gradient tensors, table {report[TABLE]:.2e} of scale, worst {max(report.values()):.2e}')


def _forbid_embedding(monkeypatch):
    def raising(*a, **kw):
        raise AssertionError('torch.nn.functional.embedding was called: the stock input stage ran')
    monkeypatch.setattr(torch.nn.functional, 'embedding', raising)


def _one_step(case, device, trainable):
    import test_hip_parity as T
    c = trainable_case(case) if trainable else copy.deepcopy(helpers.GOLDEN_CASES[case])
    args, _ = T._case_args(c)
    model = T._package_model(c, device)
    model.concept_emb.emb.weight.requires_grad_(trainable)
    dargs = [a.to(device) for a in args]
    logits, _ = model(*dargs[:5], (dargs[5], dargs[6]))
    logits.sum().backward()
    return model


def check_path_taken(device, monkeypatch):
    counter = CallCounter(ops.kernels())
    old = ops.set_kernels(counter)
    try:
        with monkeypatch.context() as mp:
            _forbid_embedding(mp)
            model = _one_step('small_train', device, True)
        assert model.concept_emb.emb.weight.grad is not None
        assert [counter.counts.get(m, 0) for m in ROW_METHODS] == [1, 1, 1], counter.counts
        counter.counts.clear()
        model = _one_step('small_train', device, False)
        assert model.concept_emb.emb.weight.grad is None and not any(counter.counts.get(m, 0) for m in ROW_METHODS), counter.counts
        counter.counts.clear()
        with monkeypatch.context() as mp:
            mp.setattr(ops, 'TRAINABLE_TABLE_FUSED', False)
            model = _one_step('small_train', device, True)
            assert model.concept_emb.emb.weight.grad is not None and not any(counter.counts.get(m, 0) for m in ROW_METHODS), counter.counts
            with pytest.raises(AssertionError, match='stock input stage'):
                _forbid_embedding(mp)
                _one_step('small_train', device, True)
    finally:
        ops.set_kernels(old)


def test_a_trainable_table_takes_the_fused_stage_on_the_emulation(emu, monkeypatch):
    """fails on a tree without the feature: the trainable table falls to nn.Embedding"""
    check_path_taken('cpu', monkeypatch)


def test_a_provider_without_the_row_methods_keeps_the_stock_path(monkeypatch):
    from emu_loss import EmuLossKernels
    old = ops.set_kernels(EmuLossKernels())
    try:
        assert not ops.table_rows_supported()
        model = _one_step('small_train', 'cpu', True)
        assert model.concept_emb.emb.weight.grad is not None
        with pytest.raises(AssertionError, match='stock input stage'):
            _forbid_embedding(monkeypatch)
            _one_step('small_train', 'cpu', True)
    finally:
        ops.set_kernels(old)


# ---- without a GPU: the comparison rejects stand-ins ---------------------------------------------------------------------------------------------
class _DropsTheLastOfASegment(EmuRowKernels):
    def row_segment_sum(self, X, order, seg, count, G, workspace):
        G.zero_()
        for u in range(min(int(count[0]), G.size(0))):
            rows = order[int(seg[u]):int(seg[u + 1])].long()
            G[u] = X[rows[:max(1, rows.numel() - 1)]].double().sum(0).to(G.dtype)
        return G


class _AssignsPerPosition(EmuRowKernels):
    def row_segment_sum(self, X, order, seg, count, G, workspace):
        G.zero_()
        for u in range(min(int(count[0]), G.size(0))):
            G[u] = X[int(order[int(seg[u + 1]) - 1])]  # (`=` per position: the last one stays)
        return G


class _CountsTheContextRows(EmuRowKernels):
    def row_groups(self, ridx, table_rows, order, seg, uniq, count, workspace):
        return super().row_groups(ridx.clamp(min=0), table_rows, order, seg, uniq, count, workspace)  # (-1 read as row 0)


STAND_INS = {'drops_last': _DropsTheLastOfASegment, 'assigns': _AssignsPerPosition, 'counts_context': _CountsTheContextRows}


def _row_gradient_case(repeats, N=40, DP=16, width=32, T=64, seed=5):
    g = torch.Generator().manual_seed(seed)
    if repeats:
        ridx = torch.randint(0, 9, (N,), generator=g)
    else:
        ridx = torch.randperm(T, generator=g)[:N]  # distinct ids and no context row: -1 on two rows is a repeated id too
    if repeats:
        ridx[::8] = -1  # context rows
    return ridx, torch.randn(N, DP, generator=g), torch.randn(DP, width, generator=g), T


def dense_from_rows(uniq, count, rows, T):
    out = torch.zeros(T, rows.size(1), dtype=rows.dtype, device=rows.device)
    ops.kernels().rows_scatter(rows, uniq, count, out)
    return out


def check_row_gradient(ridx, dpre, Wc, T, dense, what=''):
    """the dense gradient against float64 under the header's bound for the whole gradient (segment sum + product)"""
    live = (ridx >= 0) & (ridx < T)
    X, W = dpre.double().cpu(), Wc.double().cpu()
    ref = torch.zeros(T, W.size(1), dtype=torch.float64).index_add_(0, ridx.cpu()[live.cpu()], (X @ W)[live.cpu()])
    S = torch.zeros(T, X.size(1), dtype=torch.float64).index_add_(0, ridx.cpu()[live.cpu()], X.abs()[live.cpu()])
    lens = torch.bincount(ridx.cpu()[live.cpu()], minlength=T).double()
    c = (CHUNK + torch.ceil(lens / CHUNK)).unsqueeze(1) * U32
    bound = ((c * S) + 12 * EPS32 * (1 + c) * S) @ W.abs()
    err = (dense.double().cpu() - ref).abs()
    assert bool((err <= bound + 1e-300).all()), f'{what}: {int((err > bound).sum())} elements over the bound, worst {float((err / (bound + 1e-300)).max()):.2f} of it'
    return float((err / (bound + 1e-300)).max())


@pytest.mark.parametrize('name', sorted(STAND_INS))
def test_the_comparison_rejects_a_stand_in_that_is_right_without_repeated_ids(name, monkeypatch):
    old = ops.set_kernels(STAND_INS[name]())
    try:
        for repeats in (False, True):
            ridx, dpre, Wc, T = _row_gradient_case(repeats)
            dense = dense_from_rows(*ops.table_row_gradient(ridx, dpre, Wc, T), T)
            if not repeats:
                check_row_gradient(ridx, dpre, Wc, T, dense, name)
            else:
                with pytest.raises(AssertionError, match='over the bound'):
                    check_row_gradient(ridx, dpre, Wc, T, dense, name)
    finally:
        ops.set_kernels(old)
    old = ops.set_kernels(EmuRowKernels())
    try:
        ridx, dpre, Wc, T = _row_gradient_case(True)
        check_row_gradient(ridx, dpre, Wc, T, dense_from_rows(*ops.table_row_gradient(ridx, dpre, Wc, T), T), 'emulation')
    finally:
        ops.set_kernels(old)


def test_training_step_one_on_the_emulation_meets_the_oracle_and_radam(monkeypatch):
    """the harness of the GPU training test without a GPU: step 1 with the table trainable, parameters and table held to radam_oracle"""
    import test_training_loop as TL
    monkeypatch.setitem(TL.SHAPES, 'S', trainable_case(TL.SHAPES['S']))
    old = ops.set_kernels(EmuRowKernels())
    try:
        loop = _table_loop(TL, 'cpu', replay=False)
        fig = TL.oracle_step(loop, 1)
        assert TABLE in {k for k, p in loop.model.named_parameters() if p in loop.opt.state}
        note('FIGURE entity table emulation step 1: fraction of each bar ' + ', '.join(f'{k} {v:.3g}' for k, v in fig.items()))
    finally:
        ops.set_kernels(old)


STEP_BATCH = (0, 1, 2, 4)  # batches of test_training_loop.BATCHES['S'] in ONE capacity bucket: a new capture is a new trainable set


def _table_loop(TL, dev, replay):
    class TableLoop(TL.Loop):
        def batch(self, t):
            hb = TL.host_batch(self.shape, STEP_BATCH[t - 1])
            return TL.on(hb, self.dev, None if self.replay else TL.capacity(hb['E']))
    loop = TableLoop('S', 'cross_entropy', dev=dev, replay=replay)
    loop.model.concept_emb.emb.weight.requires_grad_(True)
    loop.opt = TL.make_opt(loop.model)
    if replay:
        loop.step_fn = TL.graphed.GraphedStep(loop.model, loop.nc, capacity=TL.capacity, loss='cross_entropy')
    return loop


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------------------------
def hip():
    ops.set_kernels(None)
    return ops.kernels()


def np_groups(ridx, T):
    """(order, seg, uniq, U) of include/qagnn_hip_rows.h at capacity N, by a stable numpy sort"""
    N = ridx.size
    live = np.nonzero((ridx >= 0) & (ridx < T))[0]
    pos = live[np.argsort(ridx[live], kind='stable')]
    ids = ridx[pos]
    M = pos.size
    head = np.ones(M, dtype=bool)
    head[1:] = ids[1:] != ids[:-1]
    starts = np.nonzero(head)[0]
    U = starts.size
    order, seg, uniq = np.full(N, -1, np.int32), np.full(N + 1, M, np.int32), np.full(N, -1, np.int64)
    order[:M], seg[:U], uniq[:U] = pos, starts, ids[starts]
    return order, seg, uniq, U


def gpu_groups(K, ridx, T, fill=None):
    N = ridx.numel()
    dev = ridx.device

    def buf(n, dt):
        return torch.empty(n, dtype=dt, device=dev) if fill is None else torch.full((n,), fill, dtype=dt, device=dev)
    order, seg, uniq, count = buf(N, torch.int32), buf(N + 1, torch.int32), buf(N, torch.int64), buf(1, torch.int32)
    ws = buf(K.row_groups_workspace_elems(N), torch.int32)
    K.row_groups(ridx, T, order, seg, uniq, count, ws)
    return order, seg, uniq, count


def _group_cases():
    g = np.random.default_rng(7)
    top = MAX_TABLE - 1
    digit = 1 << RG_BITS
    cases = {
        'one': (np.array([3]), 10), 'one_dead': (np.array([-1]), 10), 'none_live': (np.full(300, -1), 50), 'all_equal': (np.full(777, 5), 9),
        'all_distinct': (g.permutation(3000), 3000), 'ends': (np.array([0, 99, 0, 99, -1, 99]), 100), 'table_of_one': (np.array([0, -1, 0, 0, 5, 1]), 1),
        'digit_edges': (g.permutation(np.repeat(np.array([0, digit - 1, digit, digit + 1, 2 * digit - 1, 2 * digit, top - digit, top - 1, top, -1]), 37)), MAX_TABLE),
        'outside': (np.array([4, 7, 8, 2 ** 40, -5, 7, 4]), 8),
    }
    sizes = sorted({s + d for s in (CHUNK, CHUNK * RS_WAVES, RG_BLK, 2 * RG_BLK, 1024 * RG_SCAN_ITEMS) for d in (-1, 0, 1)})
    for N in sizes:
        cases[f'N{N}'] = (g.integers(-1, 600, N), 600)
    z = np.minimum(g.zipf(1.3, 9000), 4000) - 1
    z[g.random(9000) < 0.35] = 17  # one id on more than 40 chunks' worth of positions
    z[::50] = -1
    cases['zipf'] = (z, 4000)
    return cases


GROUP_CASES = _group_cases()


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(GROUP_CASES))
def test_row_groups_equal_a_numpy_sort_bit_for_bit(name):
    K = hip()
    ridx, T = GROUP_CASES[name]
    ridx = np.asarray(ridx, dtype=np.int64)
    if name == 'zipf':
        assert np.bincount(ridx[ridx >= 0]).max() > 40 * CHUNK
    order, seg, uniq, count = gpu_groups(K, torch.from_numpy(ridx).cuda(), T)
    worder, wseg, wuniq, U = np_groups(ridx, T)
    assert int(count[0]) == U
    assert np.array_equal(order.cpu().numpy(), worder) and np.array_equal(seg.cpu().numpy(), wseg) and np.array_equal(uniq.cpu().numpy(), wuniq)
    assert bool((uniq[U:] == -1).all())


@pytest.mark.gpu
def test_refused_row_calls_leave_their_outputs_untouched():
    K = hip()
    canary = 0x5A5A5A5
    for what, N, T, short in (('N beyond the range', MAX_N + 1, 100, 0), ('table_rows beyond the range', 100, MAX_TABLE + 1, 0),
                              ('table_rows 0', 100, 0, 0), ('a short workspace', 5000, 100, 1)):
        ridx = torch.zeros(N, dtype=torch.long, device='cuda')
        order, seg, uniq, count = (torch.full((n,), canary, dtype=dt, device='cuda') for n, dt in
                                   ((N, torch.int32), (N + 1, torch.int32), (N, torch.int64), (1, torch.int32)))
        need = K.row_groups_workspace_elems(min(N, MAX_N))
        ws = torch.full((need - short,), canary, dtype=torch.int32, device='cuda')
        with pytest.raises(RuntimeError, match='qagnn_row_groups failed'):
            K.row_groups(ridx, T, order, seg, uniq, count, ws)
        torch.cuda.synchronize()
        for t in (order, seg, uniq, count, ws):
            assert bool((t == canary).all()), what
    X, G = torch.zeros(64, 16, device='cuda'), torch.full((64, 16), 7.0, device='cuda')
    order, seg, count = (torch.zeros(n, dtype=torch.int32, device='cuda') for n in (64, 65, 1))
    ws = torch.full((K.row_segment_sum_workspace_elems(64, 16) - 1,), 7.0, device='cuda')
    with pytest.raises(RuntimeError, match='qagnn_row_segment_sum_f32 failed'):
        K.row_segment_sum(X, order, seg, count, G, ws)
    with pytest.raises(RuntimeError, match='qagnn_row_segment_sum_f32 failed'):  # cols beyond 256
        K.row_segment_sum(torch.zeros(64, 260, device='cuda'), order, seg, count, torch.full((64, 260), 7.0, device='cuda'), torch.zeros(4096, device='cuda'))
    torch.cuda.synchronize()
    assert bool((G == 7.0).all()) and bool((ws == 7.0).all())


@pytest.mark.gpu
def test_row_gradient_ignores_what_its_fresh_buffers_held():
    hip()
    ridx, T = GROUP_CASES['zipf']
    ridx = torch.from_numpy(np.asarray(ridx, dtype=np.int64)).cuda()
    g = torch.Generator().manual_seed(3)
    dpre, Wc = torch.randn(ridx.numel(), 208, generator=g).cuda(), torch.randn(208, 64, generator=g).cuda()
    helpers.check_history_free(lambda: ops.table_row_gradient(ridx, dpre, Wc, T, Wc_t=Wc.t().contiguous()), what='table_row_gradient')
    K, N = ops.kernels(), ridx.numel()

    def groups():  # (allocated through the package's `torch`, so that the fill policy reaches them)
        t = ops.torch
        order, seg, uniq, count = (t.empty(n, dtype=dt, device='cuda') for n, dt in
                                   ((N, torch.int32), (N + 1, torch.int32), (N, torch.int64), (1, torch.int32)))
        return K.row_groups(ridx, T, order, seg, uniq, count, t.empty(K.row_groups_workspace_elems(N), dtype=torch.int32, device='cuda'))
    helpers.check_history_free(groups, what='row_groups')


def twin_segment_sum(X, order, seg, U, rows):
    """numpy twin: fp32 additions in the order include/qagnn_hip_rows.h states"""
    G = np.zeros((rows, X.shape[1]), np.float32)
    for u in range(min(U, rows)):
        idx = order[seg[u]:seg[u + 1]]
        parts = []
        for k in range(0, idx.size, CHUNK):
            p = X[idx[k]].copy()
            for j in idx[k + 1:k + CHUNK]:
                p = p + X[j]
            parts.append(p)
        t = parts[0]
        for p in parts[1:]:
            t = t + p
        G[u] = t
    return G


def _segment_case(cols, seed):
    g = np.random.default_rng(seed)
    N, T = 5000, 700
    ridx = np.minimum(g.zipf(1.4, N), T) - 1
    ridx[g.random(N) < 0.55] = 3  # the heavy hitter: more than 40 chunks
    ridx[::41] = -1
    X = (g.standard_normal((N, cols)) * np.exp(g.standard_normal((N, 1)))).astype(np.float32)
    return ridx.astype(np.int64), T, X


@pytest.mark.gpu
@pytest.mark.parametrize('cols', [12, 16, 208, 256])
def test_segment_sum_and_scatter_on_pitched_operands(cols):
    from test_pitched_operands import BIG, CANARY, check_guard, pitched, same_bits
    K = hip()
    ridx, T, X = _segment_case(cols, cols)
    N = ridx.size
    assert np.bincount(ridx[ridx >= 0]).max() > 40 * CHUNK
    order, seg, uniq, count = gpu_groups(K, torch.from_numpy(ridx).cuda(), T)
    U = int(count[0])
    worder, wseg, wuniq, wU = np_groups(ridx, T)
    assert U == wU
    rows = min(N, T)
    ws_n = K.row_segment_sum_workspace_elems(N, cols)
    # contiguous, and pitched with 2^100 around the input and a canary around the output
    Gc = torch.full((rows, cols), float('nan'), device='cuda')
    K.row_segment_sum(torch.from_numpy(X).cuda(), order, seg, count, Gc, torch.full((ws_n,), float('nan'), device='cuda'))
    _, Xp = pitched(torch.from_numpy(X), cols + 20, 8, BIG, 'cuda')
    Gbuf, Gp = pitched(torch.zeros(rows, cols), cols + 12, 4, CANARY, 'cuda')
    K.row_segment_sum(Xp, order, seg, count, Gp, torch.full((ws_n,), float('nan'), device='cuda'))
    check_guard(Gbuf, Gp, 'G')
    assert same_bits(Gc, Gp), 'a pitch changed the arithmetic'
    # (a) bit for bit the numpy twin, (b) float64 under the header's bound (chunked for the heavy hitter), (c) zeros behind U
    twin = twin_segment_sum(X, worder, wseg, U, rows)
    assert np.array_equal(Gc.cpu().numpy().view(np.int32), twin.view(np.int32)), 'the additions are not in the stated order'
    lens = np.diff(wseg[:U + 1]).astype(np.float64)
    worst = 0.0
    for u in range(U):
        idx = worder[wseg[u]:wseg[u + 1]]
        exact, mag = X[idx].astype(np.float64).sum(0), np.abs(X[idx]).astype(np.float64).sum(0)
        bound = (CHUNK + math.ceil(lens[u] / CHUNK)) * U32 * mag
        err = np.abs(twin[u].astype(np.float64) - exact)
        assert (err <= bound).all(), (u, lens[u])
        worst = max(worst, float((err / (bound + 1e-300)).max()))
    assert bool((Gc[U:] == 0).all()) and U < rows
    note(f'FIGURE segment sum cols {cols}: U = {U}, longest segment {int(lens.max())} positions = {math.ceil(lens.max() / CHUNK)} chunks, worst {worst:.3f} of the bound')
    # scatter: accumulate 0 and 1 touch only the rows of uniq[:U]
    R = torch.randn(rows, cols, generator=torch.Generator().manual_seed(1))
    _, Rp = pitched(R, cols + 8, 4, BIG, 'cuda')
    base = torch.randn(T, cols, generator=torch.Generator().manual_seed(2))
    for acc in (False, True):
        obuf, out = pitched(base, cols + 16, 8, CANARY, 'cuda')
        K.rows_scatter(Rp, uniq, count, out, accumulate=acc)
        check_guard(obuf, out, 'out')
        want = base.clone()
        ids = torch.from_numpy(wuniq[:U])
        want[ids] = (base[ids] + R[:U]) if acc else R[:U]
        assert same_bits(out, want), f'accumulate={acc}'


@pytest.mark.gpu
def test_a_nan_row_reaches_exactly_its_group():
    K = hip()
    ridx, T, X = _segment_case(16, 99)
    N = ridx.size
    p = int(np.nonzero(ridx == 5)[0][0])
    X[p, 3] = np.nan
    ridx_t, Xt, Wc = torch.from_numpy(ridx), torch.from_numpy(X), torch.randn(16, 32, generator=torch.Generator().manual_seed(4))
    uniq, count, rows = ops.table_row_gradient(ridx_t.cuda(), Xt.cuda(), Wc.cuda(), T)
    got = dense_from_rows(uniq, count, rows, T).cpu()
    old = ops.set_kernels(EmuRowKernels())
    try:
        want = dense_from_rows(*ops.table_row_gradient(ridx_t, Xt, Wc, T), T)
    finally:
        ops.set_kernels(None)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert bool(torch.isnan(got[5]).all()) and not bool(torch.isnan(torch.cat([got[:5], got[6:]])).any())


@pytest.mark.gpu
@pytest.mark.parametrize('repeats', [False, True])
def test_row_gradient_meets_the_header_bound_on_the_gpu(repeats):
    hip()
    for seed, (N, DP, width, T) in enumerate([(40, 16, 32, 64), (2500, 208, 768, 3000)]):
        ridx, dpre, Wc, T = _row_gradient_case(repeats, N=N, DP=DP, width=width, T=T, seed=seed)
        ridx, dpre, Wc = ridx.cuda(), dpre.cuda(), Wc.cuda()
        for Wc_t in (None, Wc.t().contiguous()):
            dense = dense_from_rows(*ops.table_row_gradient(ridx, dpre, Wc, T, Wc_t=Wc_t), T)
            worst = check_row_gradient(ridx, dpre, Wc, T, dense, f'N={N}')
        note(f'FIGURE row gradient N={N} DP={DP} in={width} repeats={repeats}: worst {worst:.3f} of the bound')


@pytest.mark.gpu
@pytest.mark.parametrize('case', list(MODULE_CASES))
def test_module_with_a_trainable_table_meets_the_float64_oracle(case, monkeypatch):
    hip()
    report, model, args = module_vs_oracle(MODULE_CASES[case], 'cuda', monkeypatch)
    check_table_gradient(model, args, case if case == 'small_train' else None)
    note(f'FIGURE entity table {case}: {len(report)} gradient tensors, table {report[TABLE]:.2e} of scale, worst {max(report.values()):.2e}')


@pytest.mark.gpu
def test_module_with_a_trainable_table_under_the_run_scripts_dropout(monkeypatch):
    import test_hip_parity as T
    hip()
    report, model, args = module_vs_oracle(MODULE_CASES['config1_x2'], 'cuda', monkeypatch, dropout=T.RUN_SCRIPT_DROPOUT)
    check_table_gradient(model, args)
    note(f'FIGURE entity table config1_train dropout: table {report[TABLE]:.2e} of scale, worst {max(report.values()):.2e}')


@pytest.mark.gpu
def test_a_trainable_table_takes_the_fused_stage_on_the_gpu(monkeypatch):
    hip()
    check_path_taken('cuda', monkeypatch)


@pytest.mark.gpu
def test_the_stock_path_answers_with_the_switch_off(monkeypatch):
    hip()
    monkeypatch.setattr(ops, 'TRAINABLE_TABLE_FUSED', False)
    report, model, args = module_vs_oracle('config1_train', 'cuda', monkeypatch, min_share=0.2)
    check_table_gradient(model, args, 'config1_train')


@pytest.mark.gpu
def test_config1_table_gradient_meets_the_reference_fixture(monkeypatch):
    hip()
    report, model, args = module_vs_oracle('config1_train', 'cuda', monkeypatch, min_share=0.2)
    check_table_gradient(model, args, 'config1_train')


@pytest.mark.gpu
def test_two_backward_passes_over_one_forward_give_the_same_bits():
    import test_hip_parity as T
    hip()
    c = trainable_case('config1_train')
    args, _ = T._case_args(c)
    model = T._package_model(c, 'cuda')
    model.concept_emb.emb.weight.requires_grad_(True)
    dargs = [a.cuda() for a in args]
    logits, _ = model(*dargs[:5], (dargs[5], dargs[6]))
    params = [p for p in model.parameters() if p.requires_grad]
    g1 = torch.autograd.grad(logits.sum(), params, retain_graph=True)
    g2 = torch.autograd.grad(logits.sum(), params)
    for (k, _), a, b in zip([(k, p) for k, p in model.named_parameters() if p.requires_grad], g1, g2):
        assert torch.equal(a, b), k


@pytest.mark.gpu
def test_replayed_training_with_a_trainable_table_equals_the_eager_run(monkeypatch):
    """four steps at d = 32: GraphedStep(cross_entropy), clip_grad_norm_, RAdam in the reference's two groups, the table trainable; frozen
    for step 3, trainable again for step 4.  One capture per trainable set the run met (the batches share a capacity bucket): the frozen
    set adds one, and unfreezing returns to the capture of steps 1 and 2, whose key it shares."""
    import test_training_loop as TL
    hip()
    _lib.ERR_WATCH.poll(block=True)
    monkeypatch.setitem(TL.SHAPES, 'S', trainable_case(TL.SHAPES['S']))
    assert len({TL.capacity(TL.host_batch('S', i)['E']) for i in STEP_BATCH}) == 1
    eager, rep = _table_loop(TL, 'cuda', False), _table_loop(TL, 'cuda', True)
    twin = TL.make_model('S', 'cuda', fill=99)
    twin.concept_emb.emb.weight.requires_grad_(True)
    graphs = []
    for t in (1, 2, 3, 4):
        if t in (3, 4):
            for loop in (eager, rep):
                loop.model.concept_emb.emb.weight.requires_grad_(t == 4)
                loop.model.concept_emb.emb.weight.grad = None
        if t == 1:  # the replayed step against the float64 oracle and radam_oracle, the table among the parameters
            fig = TL.oracle_step(rep, 1, twin)
            note('FIGURE entity table step 1: fraction of each bar ' + ', '.join(f'{k} {v:.3g}' for k, v in fig.items()))
            a, b = eager.snapshot(*eager.step(1)), rep.snapshot()
            n = TL.same(b, {k: v for k, v in a.items() if k in b}, 'step 1')
        else:
            a, b = eager.snapshot(*eager.step(t)), rep.snapshot(*rep.step(t))
            n = TL.same(b, a, f'step {t}')
        assert ('grad ' + TABLE in b) == (t != 3) and 'exp_avg ' + TABLE in b
        graphs.append(rep.step_fn.n_graphs)
    assert graphs == [1, 1, 2, 2], graphs
    steps = {k: int(rep.opt.state[p]['step']) for k, p in rep.model.named_parameters() if p in rep.opt.state}
    assert steps[TABLE] == 3 and set(v for k, v in steps.items() if k != TABLE) == {4}
    torch.cuda.synchronize()
    _lib.ERR_WATCH.poll(block=True)
    note(f'FIGURE entity table training: {n} tensors x 4 steps bit-identical to the eager run, captures {graphs}')
