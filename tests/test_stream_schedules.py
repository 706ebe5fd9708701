"""Every two-stream schedule of the package against its one-stream bits, with the late stream CHOSEN.

Six places order two streams (or the host and a stream) by an event, a wait_stream or a keep-alive list instead of by stream order:

  S1  csrc/hop.hip: stack_bwd_impl / hop_bwd_one put a hop's weight-gradient products on qagnn_hop_args.side_stream
      (HipKernels._side_stream()): three forks per hop, a `done` event per workspace buffer set, one join per call.
  S2  ops._WgradQueue / ops._SIDE_STREAMS: the composed path's deferred weight gradients (FUSED_HOP = False), their joins and keep list.
  S3  ops.graph_prep_async / ops._PREP_STREAMS: the graph preparation next to the input stage.
  S4  data_utils.DeviceGraphStore._stage: a ring of STAGING pinned id buffers, each rewritten only behind its own event.
  S5  graphed.GraphedStep with optimizer=: what the host writes in front of a replay while earlier replays are pending.
  S6  _lib._ErrWatch: flag words copied to pinned memory plus an event.

On the small batches of a test the device waits for the host, so the second stream is never late and a missing wait passes.  Here one stream
is held by a bounded spin (helpers.hold_stream) while the whole call under test is enqueued, and the results are compared, bit for bit, with
the same call on ONE stream, synchronised after every step.  Every case asserts that its hold was still pending when its last launch had been
enqueued (helpers.check_under_hold): a hold that did not hold is a failure, not a pass.  Buffers the package allocates arrive NaN-filled
(helpers.fresh_buffers), so a premature read is a NaN; where index arrays are allocated they arrive zeroed, so that an unprepared array stays
in range.  Nothing here measures overlap.

`-m "not gpu"`: the inventory of every stream / event site of qagnn_amd/*.py and csrc/*.hip (a new or removed site fails), the constants the
GPU ladders are derived from, and the helpers' own controls.

Hold lengths (profiles/stream_schedule_gpu_tests.txt): the spin is calibrated once per process; the host enqueue time of the longest case of
each group was measured, each hold is at least four times that and at most helpers.HOLD_CAP_MS.
"""
import contextlib
import copy
import glob
import os
import re
import time

import numpy as np
import pytest
import torch

import helpers

PKG = os.path.join(helpers.ROOT, 'qagnn_amd')

# =================================================================================================================================
# CPU: inventory
# =================================================================================================================================
PY_FORMS = re.compile(r'torch\.cuda\.Stream\(|\.wait_stream\(|torch\.cuda\.Event\(|\.record\(|(?<!cuda)\.synchronize\(|non_blocking=True')
HIP_FORMS = re.compile(r'hipEventRecord|hipStreamWaitEvent|hipEventCreate')


def _enclosing(lines, i, py):
    if py:
        ind = len(lines[i]) - len(lines[i].lstrip())
        for j in range(i, -1, -1):
            m = re.match(r'(\s*)(?:def|class)\s+(\w+)', lines[j])
            if m and (len(m.group(1)) < ind or j == i):
                return m.group(2)
        return '<module>'
    for j in range(i, -1, -1):  # a function definition that starts in column 0 and opens its body on the same line
        m = re.match(r'(?:static |extern "C" |__global__ )*[\w:<>\*]+[\s\*]+(\w+)\(.*\)\s*(?:const\s*)?\{\s*(//.*)?$', lines[j])
        if m and not lines[j].startswith(' '):
            return m.group(1)
    return '<file>'


def collect_sites():
    """{(file, enclosing function, form): count} over qagnn_amd/*.py and qagnn_amd/csrc/*.hip, comments cut off (a form named in an error
    string counts: the table below says so where it happens)"""
    out = {}
    for pat, rx, py in (('*.py', PY_FORMS, True), (os.path.join('csrc', '*.hip'), HIP_FORMS, False)):
        for f in sorted(glob.glob(os.path.join(PKG, pat))):
            with open(f) as fh:
                lines = fh.read().split('\n')
            for i, line in enumerate(lines):
                code = line.split('#')[0] if py else line.split('//')[0]
                for m in rx.finditer(code):
                    key = (os.path.basename(f), _enclosing(lines, i, py), m.group(0))
                    out[key] = out.get(key, 0) + 1
    return out


# (file, enclosing function, form) -> (count, 'S1'..'S6' or 'exempt', why).  An exempt site is ordered by something other than an event of the
# package: the copy's own stream, a synchronisation, or memory nobody rewrites.
SITES = {
    ('_lib.py', '_side_stream', 'torch.cuda.Stream('): (1, 'S1', 'the stream handed to qagnn_hop_args.side_stream'),
    ('_lib.py', 'after_replay', 'torch.cuda.Event('): (1, 'S6', 'one event per watched flag block'),
    ('_lib.py', 'after_replay', '.record('): (1, 'S6', 'behind the copy of the flag words'),
    ('_lib.py', 'after_replay', 'non_blocking=True'): (1, 'S6', 'flag words -> a pinned buffer allocated per call'),
    ('_lib.py', 'poll', '.synchronize('): (1, 'S6', 'poll(block=True)'),
    ('data_utils.py', '_stage', 'torch.cuda.Event('): (1, 'S4', 'one event per ring slot'),
    ('data_utils.py', '_stage', '.record('): (1, 'S4', 'behind the copy out of the slot'),
    ('data_utils.py', '_stage', '.synchronize('): (1, 'S4', 'before the slot is rewritten'),
    ('data_utils.py', '_stage', 'non_blocking=True'): (1, 'S4', 'out of the reused pinned slot'),
    ('data_utils.py', 'refill', 'non_blocking=True'): (4, 'S5', "a capture's static twin refilled in front of a replay: device to device, on the replay's stream"),
    ('data_utils.py', '__init__', 'non_blocking=True'): (1, 'exempt', 'EdgeListBatch.count: out of a fresh one-element host tensor nobody rewrites'),
    ('data_utils.py', 'to_packed', 'non_blocking=True'): (1, 'exempt', 'out of a pinned buffer packed for this batch and never rewritten'),
    ('data_utils.py', '_graphs_to_device', 'non_blocking=True'): (1, 'exempt', "out of the generator's buffer of this batch, never rewritten"),
    ('data_utils.py', '__iter__', 'non_blocking=True'): (1, 'exempt', "out of the generator's buffer of this batch, never rewritten"),
    ('graphed.py', 'load_static_inputs', 'non_blocking=True'): (5, 'S5', "static inputs rewritten in front of a replay, on the replay's stream"),
    ('graphed.py', '_load', 'non_blocking=True'): (1, 'S5', "the labels' static buffer, on the replay's stream"),
    ('graphed.py', 'warm_up', 'torch.cuda.Stream('): (1, 'exempt', 'the warm-up runs on a stream of its own and ends behind a device synchronisation'),
    ('graphed.py', 'warm_up', '.wait_stream('): (2, 'exempt', 'the warm-up runs on a stream of its own and ends behind a device synchronisation'),
    ('inference.py', '_load', 'non_blocking=True'): (1, 'exempt', "the evaluation replay's label buffer: stream order, no optimiser state (out of scope: held by tests/test_inference_path.py)"),
    ('inference.py', 'evaluate_accuracy', 'non_blocking=True'): (1, 'exempt', "the caller's labels, read once"),
    ('inference.py', 'evaluate_detail', 'non_blocking=True'): (1, 'exempt', "the caller's labels, read once"),
    ('ops.py', 'flush_wgrads', 'torch.cuda.Stream('): (1, 'S2', 'ops._SIDE_STREAMS'),
    ('ops.py', 'flush_wgrads', '.wait_stream('): (2, 'S2', 'the fork, and the join of work left on another main stream'),
    ('ops.py', 'join_wgrads', '.wait_stream('): (1, 'S2', 'the join'),
    ('ops.py', 'reset_wgrad_queue', '.wait_stream('): (1, 'S2', 'the join behind a backward that raised'),
    ('ops.py', 'graph_prep_async', 'torch.cuda.Stream('): (1, 'S3', 'ops._PREP_STREAMS'),
    ('ops.py', 'graph_prep_async', '.wait_stream('): (2, 'S3', 'the fork behind the last readers of the recycled storage, and join()'),
    ('hop.hip', 'side_sync_init', 'hipEventCreate'): (2, 'S1', 'the event pool (hipEventCreateWithFlags, and its name in the error text)'),
    ('hop.hip', 'stream_after', 'hipEventRecord'): (1, 'S1', 'a fork'),
    ('hop.hip', 'stream_after', 'hipStreamWaitEvent'): (1, 'S1', 'a fork'),
    ('hop.hip', 'hop_bwd_one', 'hipEventRecord'): (2, 'S1', "the buffer set's `done` event (and its name in the error text)"),
    ('hop.hip', 'stack_bwd_impl', 'hipStreamWaitEvent'): (3, 'S1', 'the wait for `done[set]` (and its name in the error text), the join'),
    ('hop.hip', 'stack_bwd_impl', 'hipEventRecord'): (1, 'S1', 'the join'),
    ('timing.hip', '<file>', 'hipEventCreate'): (2, 'exempt', 'a timing pair on ONE stream: orders nothing'),
    ('timing.hip', '<file>', 'hipEventRecord'): (2, 'exempt', 'a timing pair on ONE stream: orders nothing'),
}


def test_every_stream_and_event_site_is_listed():
    """A new or removed stream, event, wait or non-blocking copy in the package fails here until the table says which schedule test holds it
    (or why none has to)."""
    found = collect_sites()
    want = {k: v[0] for k, v in SITES.items()}
    new = {k: n for k, n in found.items() if want.get(k) != n}
    gone = {k: n for k, n in want.items() if k not in found}
    assert not new and not gone, f'sites not in the table (or with another count): {new}; sites of the table that are gone: {gone}'
    assert {v[1] for v in SITES.values()} == {'S1', 'S2', 'S3', 'S4', 'S5', 'S6', 'exempt'}
    assert all(v[2] for v in SITES.values())
    # the collector sees what it is meant to see
    assert _enclosing(['def f():', '    x = 1', '    y.record()'], 2, True) == 'f'
    assert PY_FORMS.findall('ev.synchronize(); torch.cuda.synchronize(); a.to(d, non_blocking=True)') == ['.synchronize(', 'non_blocking=True']


# =================================================================================================================================
# CPU: the constants the ladders are derived from
# =================================================================================================================================
def _function_body(src, name):
    """the text of the column-0 function `name` of a .hip file, up to the next closing brace in column 0"""
    m = re.search(r'^(?:static |extern "C" )*\w[\w\s\*]*\b' + name + r'\(.*?^\}', src, re.S | re.M)
    assert m, name
    return m.group(0)


def schedule_constants():
    with open(os.path.join(PKG, 'csrc', 'hop.hip')) as f:
        hop = f.read()
    with open(os.path.join(PKG, 'data_utils.py')) as f:
        du = f.read()
    pool = int(re.search(r'HOP_EV_POOL\s*=\s*(\d+)', hop).group(1))
    staging = int(re.search(r'^\s+STAGING\s*=\s*(\d+)', du, re.M).group(1))
    per_hop = _function_body(hop, 'hop_bwd_one').count('ss->take()')
    per_stack = _function_body(hop, 'stack_bwd_impl').count('ss.take()')
    k_wrap = next(k for k in range(1, 10 * pool) if per_hop * k + per_stack > pool)
    return dict(HOP_EV_POOL=pool, STAGING=staging, events_per_hop=per_hop, events_per_stack=per_stack, k_wrap=k_wrap)


CONST = schedule_constants()
K_LADDER = (1, 2, 3, 4, 5, CONST['k_wrap'])  # no buffer set reused; reuse at both parities; the event pool wraps around


def test_constants_the_ladders_are_derived_from():
    from qagnn_amd import data_utils
    assert CONST == dict(HOP_EV_POOL=64, STAGING=8, events_per_hop=4, events_per_stack=1, k_wrap=16), CONST
    assert data_utils.DeviceGraphStore.STAGING == CONST['STAGING']
    with open(os.path.join(PKG, 'csrc', 'hop.hip')) as f:
        body = _function_body(f.read(), 'hop_bwd_one')
    assert body.count('stream_after(ss->side, ss->main, ss->take())') == 3 and body.count('*done = ss->take()') == 1  # three forks and `done`
    assert K_LADDER == (1, 2, 3, 4, 5, 16) and CONST['events_per_hop'] * (CONST['k_wrap'] - 1) + 1 <= CONST['HOP_EV_POOL']
    with open(os.path.join(PKG, 'data_utils.py')) as f:
        assert re.search(r'max\(ids32\.size, 512\)', f.read()), 'the minimum ring buffer of 512 words'
    assert STAGE_LENGTHS.count(600) == 1 and max(STAGE_LENGTHS) > 512 > min(STAGE_LENGTHS) and len(STAGE_LENGTHS) == 3 * CONST['STAGING'] + 1


# =================================================================================================================================
# CPU: the helpers' own controls
# =================================================================================================================================
def test_hold_stream_refuses_a_cpu_device_and_a_hold_above_the_cap():
    for bad in (torch.device('cpu'), torch.zeros(2), 'cpu', None):
        with pytest.raises(ValueError, match='stream of a GPU'):
            helpers.hold_stream(bad, 10.0)
    for ms in (helpers.HOLD_CAP_MS + 1.0, 1e9, 0.0, -5.0):
        with pytest.raises(ValueError, match='bounded'):
            helpers.hold_stream(torch.device('cpu'), ms)
    assert helpers.HOLD_CAP_MS == 250.0 and all(h <= helpers.HOLD_CAP_MS for h in HOLD_MS.values())

    class _Pending:
        def __init__(self, done):
            self.done = done

        def query(self):
            return self.done
    helpers.check_under_hold(helpers.StreamHold(_Pending(False), 5.0))
    for holds in ((), (helpers.StreamHold(_Pending(True), 5.0),), (helpers.StreamHold(_Pending(False), 5.0), helpers.StreamHold(_Pending(True), 5.0))):
        with pytest.raises(AssertionError, match='hold too short: the schedule was not adverse'):
            helpers.check_under_hold(*holds)


def _two_set_backward(fill, stand_in=None, k=3):
    """The buffer-set discipline of the stack backward in miniature, float64 on the host -- a model written for this control, not the
    emulated kernel provider (whose stack backward has one workspace per call and no second stream): what it shows is that same_bits
    tells a premature read under the NaN fill from a right answer, not that the emulation keeps the discipline. hop `it` writes its d out into buffer set it & 1 of a
    workspace that starts as `fill`, and its weight gradient dW = h1^T d out into an output that starts as `fill`.
    stand_in 'poison': the product of hop 1 is added to what its output held (right from zeros; from the NaN fill, the fill);
    'other_set': hop 0's product reads its own set PLUS the other set, which nothing has written yet (right from zeros)."""
    g = torch.Generator().manual_seed(3)
    h1 = [torch.randn(6, 4, generator=g, dtype=torch.float64) for _ in range(k)]
    dy = torch.randn(6, 4, generator=g, dtype=torch.float64)
    sets = torch.full((2, 6, 4), fill, dtype=torch.float64)
    out = {}
    for it in range(k):
        s = it & 1
        sets[s] = dy * (it + 1.0)
        dW = torch.full((4, 4), fill, dtype=torch.float64)
        operand = sets[s] + sets[1 - s] if (stand_in == 'other_set' and it == 0) else sets[s]
        prod = h1[it].t() @ operand
        dW = dW + prod if (stand_in == 'poison' and it == 1) else prod
        out[f'dW{it}'] = dW
    return out


@pytest.mark.parametrize('stand_in', ['poison', 'other_set'])
def test_the_comparison_rejects_a_stand_in_that_is_right_on_zeros(stand_in):
    want = _two_set_backward(float('nan'))
    assert all(bool(torch.isfinite(t).all()) for t in want.values())
    assert helpers.same_bits(_two_set_backward(0.0), want, 'zeros against the NaN fill') == 3 * 16
    assert helpers.same_bits(_two_set_backward(0.0, stand_in), want, f'{stand_in} from zeros') == 3 * 16, 'the stand-in is right on zeros'
    with pytest.raises(AssertionError, match=r'dW[01]\[0\]: 16 of 16 elements differ \(16 NaN\)'):
        helpers.same_bits(_two_set_backward(float('nan'), stand_in), want, f'{stand_in} under the NaN fill')
    with pytest.raises(AssertionError):  # a NaN equals only the same NaN; a missing tensor is no match
        helpers.same_bits({'a': torch.tensor([float('nan')])}, {'a': torch.tensor([0.0])})
    with pytest.raises(AssertionError):
        helpers.same_bits({'a': [torch.zeros(2), None]}, {'a': [torch.zeros(2), torch.zeros(2)]})


# =================================================================================================================================
# GPU: common
# =================================================================================================================================
# hold lengths in ms per group: >= 4 x the measured host enqueue time of the group's longest case (profiles/stream_schedule_gpu_tests.txt)
HOLD_MS = {'S1': 80.0, 'S2': 200.0, 'S3': 200.0, 'S4': 40.0, 'S5': 120.0, 'S6': 40.0}
LONGER = 1.5   # schedule (c): the side hold against the main hold
_INSTALLED = []  # (dict, key, previous entry or None) of every stream a test installed: put back behind the test


def hip():
    from qagnn_amd import ops
    ops.set_kernels(None)
    return ops.kernels()


def _main():
    return torch.cuda.current_stream()


def _hold(which, group, side=None):
    """which: 'a' side held, 'b' main held, 'c' both with the side hold the longer one -> the holds, in the order they were enqueued"""
    ms = HOLD_MS[group]
    holds = []
    if which in ('b', 'c'):
        holds.append(helpers.hold_stream(_main(), ms))
    if which in ('a', 'c'):
        holds.append(helpers.hold_stream(side, min(helpers.HOLD_CAP_MS, ms * (LONGER if which == 'c' else 1.0))))
    return holds


def _enqueued(holds, t0, what):
    """right behind the last launch of the call under test: the holds must still be pending"""
    ms = (time.perf_counter() - t0) * 1e3
    helpers.check_under_hold(*holds)
    print(f'FIGURE enqueue {what}: {ms:.2f} ms on the host under holds of {[h.ms for h in holds]} ms')
    for h in holds:
        h.release_wait()
    torch.cuda.synchronize()
    return ms


@pytest.fixture(autouse=True)
def _wall_and_streams(request):
    """the case's wall time; and the package's stream tables as the test found them (install_side_stream)"""
    t0 = time.perf_counter()
    yield
    while _INSTALLED:
        table, key, old = _INSTALLED.pop()
        if old is None:
            table.pop(key, None)
        else:
            table[key] = old
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        print(f'FIGURE wall {request.node.name}: {time.perf_counter() - t0:.2f} s')


# =================================================================================================================================
# S1: the native hop and stack backward
# =================================================================================================================================
S1_WIDTHS = {100: (28, 25, 50), 200: (52, 50, 100)}  # d -> (HP, ones_col, tab_col) as ops.HeadLayout and the stack place them (test_hip_parity.WIDTH_BRANCHES)
# (d, k, form, batch_stats, tab_col >= 0, ones_col >= 0).  form: 'split1' gemm_split = 1; 'split2' the default below the row threshold of the
# packed forms; 'everywhere' the three-MFMA form (helpers.form_everywhere); 'dual' that form with the dX | dS launch forced on (mode 2, d = 200)
S1_CASES = [(200, k, 'everywhere', True, True, True) for k in K_LADDER] + [
    (100, 3, 'split1', True, False, False), (100, 4, 'everywhere', False, True, False), (100, 2, 'split2', True, False, True),
    (100, 5, 'everywhere', True, True, True), (200, 3, 'split1', False, False, True), (200, 4, 'dual', True, True, False),
    (200, 5, 'split2', True, False, False), (200, 2, 'dual', True, False, True)]
S1_ENTRIES = ('hop', 'stack', 'deferred')
S1_N, S1_E = 337, 1300  # node rows (no multiple of a 32-row k-tile or a 128-row tile), edges


class _S1:
    """k chained hops after HipKernels.stack_fwd; run(): the backward through hop_bwd (hop 0) / stack_bwd (defer off / on)"""

    def __init__(self, K, d, k, batch_stats, tab, ones):
        import test_deferred_reductions as TD
        from test_hip_kernels import side_width
        self.K = K
        HP, oc, tc = S1_WIDTHS[d]
        DP, SP = 4 * HP, side_width(HP)
        ei, et, nt, R, T = TD._graph(40 + k, S1_N, S1_E, 3, 2)
        self.g, self.nt = K.graph_prep(ei.cuda(), et.cuda(), nt.cuda(), R, T), nt.cuda()
        N = S1_N
        gen = torch.Generator().manual_seed(900 + k)
        rnd = lambda *shape, s=0.1: (torch.randn(*shape, generator=gen) * s).cuda()  # noqa: E731
        self.prms = []
        for _ in range(k):
            Wx_t, Ws_t, W1t, W2t = rnd(DP, 3 * DP), rnd(SP, 3 * DP), rnd(DP, DP), rnd(DP, DP)
            self.prms.append((Wx_t, Wx_t.t().contiguous(), Ws_t, Ws_t.t().contiguous(), rnd(T, 3 * DP), rnd(self.g.C, 2 * DP), W1t, W1t.t().contiguous(),
                              rnd(DP), 1 + rnd(DP), rnd(DP), W2t, W2t.t().contiguous(), rnd(DP), rnd(DP), 0.5 + rnd(DP).abs()))
        S = torch.randn(N, SP, generator=gen)
        if tab:  # the type indicators ride in S's padding columns
            S[:, tc:tc + T] = torch.nn.functional.one_hot(nt, T).float()
        self.X, self.S = rnd(N, DP, s=1.0), S.cuda()
        self.dys = [rnd(N, DP, s=1.0), rnd(N, DP, s=0.37)]
        self.k, self.HP, self.cols, self.bs = k, HP, (tc if tab else -1, oc if ones else -1), batch_stats
        self.p, self.seeds = 0.2, [4321 + l for l in range(k)]
        _, self.saved = K.stack_fwd(self.g, HP, 0.25, self.X, self.S, self.nt, self.prms, batch_stats, 1e-5, self.p, self.seeds, [None] * k, cols=self.cols)
        torch.cuda.synchronize()

    def run(self, entry, overlap, sync, behind_first=None):
        """-> clones of everything the calls wrote, taken on the main stream behind each call.  behind_first(dW2t of the hop that runs first):
        called right after the first call has returned (a second call's buffers are filled behind the first call's join)"""
        K, sv, out = self.K, self.saved, {}
        for i, dy in enumerate(self.dys[:1] if entry == 'hop' else self.dys):
            if entry == 'hop':
                hop_saved = (sv[0][0], sv[1][0], sv[2][0, 0], sv[2][0, 1], sv[2][0, 2], sv[3][0], sv[4][0])
                r = K.hop_bwd(self.g, self.HP, 0.25, self.X, self.S, self.nt, self.prms[0], self.bs, 1e-5, self.p, self.seeds[0], True, hop_saved, dy, True,
                              True, tab_col=self.cols, overlap=overlap)
                dX, dS, grads = r[0], r[1], list(r[2:])
            else:
                dX, dS, per_layer = K.stack_bwd(self.g, self.HP, 0.25, self.X, self.S, self.nt, self.prms, self.bs, 1e-5, self.p, self.seeds, sv, dy, True,
                                                True, tab_col=self.cols, overlap=overlap, defer=entry == 'deferred')
                grads = [t for layer in per_layer for t in layer]
                for layer in per_layer:  # dWs_t lies right behind dWx_t: the hop takes them as ONE [DP + SP, 3 DP] product, with the graph's live k-tiles
                    assert layer[1].data_ptr() == layer[0].data_ptr() + layer[0].numel() * 4 and K.tn_live
            out[f'call {i}'] = [dX.clone(), dS.clone(), sv[4].clone()] + [t.clone() for t in grads]
            if i == 0 and behind_first is not None:
                behind_first(grads[-2])  # dW2t of the last layer: the first product the side stream is given
            if sync:
                torch.cuda.synchronize()
        return out


@contextlib.contextmanager
def _s1_form(K, form, monkeypatch):
    import test_dual_product as TDP
    with contextlib.ExitStack() as st:
        if form == 'split1':
            monkeypatch.setattr(K, 'gemm_split', 1)
        elif form == 'everywhere':
            st.enter_context(helpers.form_everywhere())
        elif form == 'dual':
            st.enter_context(TDP._small_rows(K, 128))
        else:
            assert form == 'split2' and K.gemm_split == 2
        yield


_STREAMS = []


def _runs_during(stream, *held):
    """a marker enqueued on `stream` completes while every stream of `held` is held"""
    torch.cuda.synchronize()
    holds = [helpers.hold_stream(s, 20.0) for s in held]
    with torch.cuda.stream(stream):
        torch.zeros(4, device='cuda').add_(1.0)
        ev = torch.cuda.Event()
        ev.record(stream)
    ev.synchronize()
    free = all(h.still_held() for h in holds)
    for h in holds:
        h.release_wait()
    return free


def independent_streams():
    """(side, third), chosen once per process.  Streams share a few hardware queues, and two streams on one queue run in the order of their
    launches: a hold on one of them holds the other, the schedule "side held, main running ahead" would be "both held", and a witness stream
    would read behind the hold.  So the streams of this file are probed: `side` and the main stream each run while the other is held, `third`
    runs while both are.  `side` is what the tests install as the package's side stream (HipKernels._side_streams, ops._SIDE_STREAMS,
    ops._PREP_STREAMS: the package takes whatever stream it finds there)."""
    if not _STREAMS:
        main = _main()
        cands = [torch.cuda.Stream() for _ in range(8)]
        side = next((c for c in cands if _runs_during(main, c) and _runs_during(c, main)), None)
        assert side is not None, 'no stream runs independently of the main stream: no schedule with ONE stream held can be forced'
        third = next((c for c in cands if c is not side and _runs_during(c, main, side)), None)
        assert third is not None, 'no stream runs while the main and the side stream are held: the lag witness cannot be taken'
        _STREAMS.extend([side, third])
        print(f'FIGURE streams: candidates {cands.index(side)} (side) and {cands.index(third)} (third) of 8 run independently')
    return tuple(_STREAMS)


def install_side_stream(which, K=None):
    """which: 'hop' (of the provider K) / 'wgrad' / 'prep' -> the probed side stream, installed where the package looks for that stream"""
    from qagnn_amd import ops
    side, _ = independent_streams()
    dev = torch.cuda.current_device()
    table = {'hop': K._side_streams if K is not None else None, 'wgrad': ops._SIDE_STREAMS, 'prep': ops._PREP_STREAMS}[which]
    if table.get(dev) is not side:
        _INSTALLED.append((table, dev, table.get(dev)))  # (_wall_and_streams puts the entry back behind the test)
        table[dev] = side
    return side


@pytest.mark.gpu
@pytest.mark.parametrize('d,k,form,batch_stats,tab,ones', S1_CASES,
                         ids=[f'd{d}-k{k}-{form}-{"batch" if bs else "running"}-tab{int(t)}-ones{int(o)}' for d, k, form, bs, t, o in S1_CASES])
def test_native_backward_under_held_streams_equals_one_stream(d, k, form, batch_stats, tab, ones, monkeypatch):
    """hop_bwd, stack_bwd and the deferred stack; side held, main held, both held.  The stack entries run TWO backwards (another dy) back to
    back under one hold.  Every output -- dX, dS, every weight, table, class and bias gradient, the maximum words -- is cloned on the main
    stream without a host synchronisation and equals the one-stream call.  Side held: a clone of a weight gradient taken on a third stream
    that waits for nothing still holds the 0xFF fill (the products really were late)."""
    from qagnn_amd import _lib
    K = hip()
    with _s1_form(K, form, monkeypatch):
        st = _S1(K, d, k, batch_stats, tab, ones)
        side, third = install_side_stream('hop', K), independent_streams()[1]
        assert K._side_stream() == side.cuda_stream
        n = 0
        for entry in S1_ENTRIES:
            n_dual = K.dual_launches()
            with helpers.fresh_buffers('nan'):
                want = st.run(entry, False, True)
            if form == 'dual':
                assert K.dual_launches() - n_dual == (1 if entry == 'hop' else 2 * k), 'the two-output launch was to run in every hop'
            if form in ('everywhere', 'dual') and batch_stats and d == 200:  # (DP = 208: the width whose backward runs the form)
                words = want['call 0'][2][:, _lib.HOP_AM_DKMQ].tolist()
                assert all(0 < w < 0x7F000000 for w in (words[:1] if entry == 'hop' else words)), f'the three-MFMA form did not run: {words}'
            assert all(bool(torch.isfinite(t).all()) for t in want['call 0'][:2]), 'dX / dS of the one-stream call'
            for which in ('a', 'b', 'c'):
                torch.cuda.synchronize()
                with helpers.fresh_buffers('nan'):
                    holds = _hold(which, 'S1', side)
                    t0 = time.perf_counter()
                    seen = {}

                    def take(late):
                        with torch.cuda.stream(third):
                            seen['late'], seen['witness'] = late, late.view(torch.int32).add(0)  # (an elementwise launch, not a copy)
                            seen['taken'] = torch.cuda.Event()
                            seen['taken'].record(third)
                    got = st.run(entry, True, False, take if which == 'a' else None)
                    if which == 'a':
                        helpers.check_under_hold(*holds)
                        seen['taken'].synchronize()
                        in_time = holds[0].still_held()  # the witness was read while the side stream was still held
                    _enqueued(holds, t0, f'S1 {entry} k={k} d={d} {form} ({which})')
                what = f'{entry}, k = {k}, d = {d}, {form}, schedule ({which})'
                if which == 'a':
                    witness = seen['witness']
                    n_fill, n_prod = int((witness == helpers.fill_word('nan')).sum()), int((witness.cpu() == helpers._bits(seen['late'])).sum())
                    assert in_time and n_fill == witness.numel(), \
                        (f'{what}: the weight gradients were not late -- the witness was read {"inside" if in_time else "behind"} the hold; '
                         f'{n_fill} of {witness.numel()} of its elements hold the fill, {n_prod} the product')
                n += helpers.same_bits(got, want, what)
    print(f'FIGURE S1 d={d} k={k} {form}: {n} elements equal under three schedules x {len(S1_ENTRIES)} entry points')


# =================================================================================================================================
# S2: the composed path's deferred weight gradients
# =================================================================================================================================
S2_PS = dict(p_emb=0.2, p_gnn=0.2, p_fc=0.2, p_attn=0.1, p_pool=0.1)


def _s2_case(name, seed=None):
    import test_hip_parity as HPAR
    c = dict(HPAR.tiny_case(100, True) if name == 'tiny100' else helpers.GOLDEN_CASES['small_train'])
    if seed is not None:
        c['seed'] = seed
    return c


def _s2_args(case):
    import test_hip_parity as HPAR
    args, _ = HPAR._case_args(case)
    return [a.cuda() for a in args]


def _s2_model(case):
    import test_hip_parity as HPAR
    return HPAR._package_model(case, 'cuda', S2_PS)


def _s2_step(model, args, hook=None):
    for p in model.parameters():
        p.grad = None
    logits, _ = model(*args[:5], (args[5], args[6]))
    B = logits.numel()
    (logits.view(-1) * torch.linspace(0.5, 1.5, B, device=logits.device)).sum().backward()
    out = {'logits': logits.detach().clone()}
    out.update({'grad ' + k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    out.update({'buffer ' + k: b.clone() for k, b in model.named_buffers()})
    return out


@contextlib.contextmanager
def _s2_mode(monkeypatch, overlap):
    from qagnn_amd import ops
    monkeypatch.setattr(ops, 'FUSED_HOP', False)
    monkeypatch.setattr(ops, 'FUSED_STACK', False)
    monkeypatch.setattr(ops, 'WGRAD_POISON', True)
    monkeypatch.setattr(ops, 'WGRAD_OVERLAP', overlap)
    torch.manual_seed(5)
    ops._seed_counter[0] = 0
    yield ops


def _s2_warm(model, args, ops):
    """one synchronised step: a model's first forward builds its packing plans with host-synchronous copies, which would end a main hold"""
    _s2_step(model, args)
    torch.cuda.synchronize()
    torch.manual_seed(5)
    ops._seed_counter[0] = 0
    return model


def _s2_side(monkeypatch, case):
    """one warm-up step on a model of its own, on the probed side stream"""
    side = install_side_stream('wgrad')
    with _s2_mode(monkeypatch, True) as ops:
        _s2_step(_s2_model(case), _s2_args(case))
        torch.cuda.synchronize()
        assert ops._SIDE_STREAMS[torch.cuda.current_device()] is side
    return side


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['tiny100', 'small_train'])
@pytest.mark.parametrize('which', ['a', 'b'])
def test_composed_path_under_held_streams_equals_one_stream(name, which, monkeypatch):
    """FUSED_HOP = False, WGRAD_POISON = True, dropout on: logits, every gradient and every buffer of a step equal the WGRAD_OVERLAP = False
    step.  A second forward + backward on another batch inside the same hold allocates, on the main stream, what the first step freed while
    (side held) the first step's weight-gradient products are still pending: the keep list's job."""
    hip()
    case, other = _s2_case(name), _s2_case(name, seed=57)
    args, args2 = _s2_args(case), _s2_args(other)
    side = _s2_side(monkeypatch, case)
    with _s2_mode(monkeypatch, False) as ops, helpers.fresh_buffers('nan'):
        model = _s2_warm(_s2_model(case), args2, ops)
        want = []
        for a in (args, args2):
            want.append(_s2_step(model, a))
            torch.cuda.synchronize()
    with _s2_mode(monkeypatch, True) as ops, helpers.fresh_buffers('nan'):
        model = _s2_warm(_s2_model(case), args2, ops)
        n0 = ops._WgradQueue.n_deferred
        holds = _hold(which, 'S2', side)
        t0 = time.perf_counter()
        got = [_s2_step(model, a) for a in (args, args2)]
        _enqueued(holds, t0, f'S2 {name} two steps ({which})')
        assert ops._WgradQueue.n_deferred > n0, 'nothing was deferred'
    for i in range(2):
        n = helpers.same_bits(got[i], want[i], f'{name}, schedule ({which}), step {i + 1}')
    assert not torch.equal(want[0]['logits'], want[1]['logits'])
    print(f'FIGURE S2 {name} ({which}): {n} elements per step equal')


@pytest.mark.gpu
def test_a_backward_that_raised_behind_its_deferrals_is_followed_by_a_good_step(monkeypatch):
    """A gradient hook raises after the stack's backward has queued its weight gradients; the next step, with the side stream held, equals
    its one-stream twin: reset_wgrad_queue's job."""
    hip()
    case = _s2_case('tiny100')
    args = _s2_args(case)
    side = _s2_side(monkeypatch, case)

    def sequence(ops, hold):
        model = _s2_model(case)
        torch.cuda.synchronize()
        target = next(p for k, p in model.named_parameters() if k.startswith('svec2nvec') and p.dim() == 2)
        n0 = ops._WgradQueue.n_deferred

        def boom(g):
            raise RuntimeError('injected')
        handle = target.register_hook(boom)
        holds = _hold('a', 'S2', side) if hold else []
        t0 = time.perf_counter()
        with pytest.raises(RuntimeError, match='injected'):
            _s2_step(model, args)
        handle.remove()
        deferred = ops._WgradQueue.n_deferred - n0
        out = _s2_step(model, args)
        if hold:
            _enqueued(holds, t0, 'S2 a raised backward, then a good step (a)')
        torch.cuda.synchronize()
        return out, deferred
    with _s2_mode(monkeypatch, False) as ops, helpers.fresh_buffers('nan'):
        want, _ = sequence(ops, False)
    with _s2_mode(monkeypatch, True) as ops, helpers.fresh_buffers('nan'):
        got, deferred = sequence(ops, True)
    assert deferred > 0, 'the hook raised before anything was deferred'
    helpers.same_bits(got, want, 'the step behind a backward that raised')


@pytest.mark.gpu
def test_negative_control_a_join_that_does_not_wait_reads_the_poison(monkeypatch):
    """Once, float data only: ops.join_wgrads flushes but does not wait.  With the side stream held the main stream then reads the deferred
    gradients before their products ran -- the NaN poison out of allocated memory, a wrong number and never an address -- and the comparison
    fails on them.  The same comparison passes everywhere else in this file."""
    hip()
    case = _s2_case('tiny100')
    args = _s2_args(case)
    side = _s2_side(monkeypatch, case)
    with _s2_mode(monkeypatch, False) as ops, helpers.fresh_buffers('nan'):
        want = _s2_step(_s2_model(case), args)
        torch.cuda.synchronize()
    with _s2_mode(monkeypatch, True) as ops, helpers.fresh_buffers('nan'):
        model = _s2_model(case)
        torch.cuda.synchronize()
        real_join = ops.join_wgrads
        monkeypatch.setattr(ops, 'join_wgrads', lambda ref=None: ops.flush_wgrads(ref))  # (unjoined and the keep list stay as flush left them)
        holds = _hold('a', 'S2', side)
        t0 = time.perf_counter()
        got = _s2_step(model, args)
        _enqueued(holds, t0, 'S2 negative control (a)')
        monkeypatch.setattr(ops, 'join_wgrads', real_join)
        ops.join_wgrads()
        torch.cuda.synchronize()
    with pytest.raises(AssertionError, match=r'\([1-9]\d* NaN\)'):
        helpers.same_bits(got, want, 'a join that does not wait')
    poisoned = [k for k in got if k.startswith('grad ') and bool(torch.isnan(got[k]).any())]
    assert poisoned and torch.equal(got['logits'], want['logits']), poisoned
    print(f'FIGURE S2 negative control: {len(poisoned)} gradients read the poison, e.g. {poisoned[:3]}')


# =================================================================================================================================
# S3: the preparation stream
# =================================================================================================================================
HOLDERS = ('pair', 'edge lists', 'blobs', 'store')
S3_IDS = ([3, 9, 0, 4, 7, 3, 8, 1, 6, 2], [10, 5, 1, 7, 2, 9, 0, 6, 8, 5])  # two batches of ten with different edge counts


def _s3_holder(kind, h, d, ids):
    import test_device_store as DS
    from qagnn_amd import data_utils
    if kind == 'store':
        return d.batch(ids, DS.NC)
    packed = DS._packed(h, ids, DS.NC, 'cuda')
    if kind == 'blobs':
        return packed
    E = int(h.store.edge_count[ids].sum())
    cap = None if kind == 'pair' else -(-E // 256) * 256 + 256
    el = data_utils.EdgeListBatch.from_lists(*packed.nested_lists(), h.n, e_cap=cap).to('cuda')
    return el.pair() if kind == 'pair' else el


def _s3_run(kind, overlap, hold, monkeypatch):
    import test_device_store as DS
    from qagnn_amd import ops
    monkeypatch.setattr(ops, 'PREP_OVERLAP', overlap)
    h = DS._train_store()
    d = h.device('cuda')
    torch.manual_seed(5)
    ops._seed_counter[0] = 0
    model = DS._small_model(h.R, p=0.2).cuda().train()
    xs = [DS._inputs(h, ids, DS.NC, 'cuda') for ids in S3_IDS]
    adjs = [_s3_holder(kind, h, d, ids) for ids in S3_IDS]
    assert int(h.store.edge_count[S3_IDS[0]].sum()) != int(h.store.edge_count[S3_IDS[1]].sum())
    DS._eager(model, xs[1], adjs[1], xs[1]['fields'])  # (a model's first forward builds its packing plans with host-synchronous copies)
    torch.cuda.synchronize()
    torch.manual_seed(5)
    ops._seed_counter[0] = 0
    out = []
    with helpers.fresh_buffers('zero'):
        holds = []
        if hold == 'a':
            holds = _hold('a', 'S3', install_side_stream('prep'))
        elif hold == 'b':
            holds = _hold('b', 'S3')
        t0 = time.perf_counter()
        for x, adj in list(zip(xs, adjs))[:1 if hold == 'a' else 2]:
            out.append(DS._eager(model, x, adj, x['fields']))
            if not holds:
                torch.cuda.synchronize()
        if holds:
            _enqueued(holds, t0, f'S3 {kind} ({hold})')
    return [dict(logits=o[0], loss=o[1].reshape(-1), **{'grad ' + k: v for k, v in o[2].items()}, **{'buffer ' + k: v for k, v in o[3].items()}) for o in out]


@pytest.mark.gpu
@pytest.mark.parametrize('kind', HOLDERS)
def test_preparation_stream_under_held_streams_equals_one_stream(kind, monkeypatch):
    """All four graph holders.  (a) the preparation stream is held: the stack waits for the graph.  (b) the main stream is held and two eager
    steps on batches of different edge counts are enqueued without a synchronisation: step 2's preparation recycles step 1's graph storage
    while step 1's backward is pending.  Both equal PREP_OVERLAP = False, synchronised after every step.  No negative control: a stack that
    read unprepared index arrays could address outside its buffers -- the still-pending hold is the proof that the schedule was adverse."""
    from qagnn_amd import _lib
    hip()
    _lib.ERR_WATCH.poll(block=True)
    want = _s3_run(kind, False, None, monkeypatch)
    install_side_stream('prep')
    got_a = _s3_run(kind, True, 'a', monkeypatch)
    got_b = _s3_run(kind, True, 'b', monkeypatch)
    helpers.same_bits(got_a[0], want[0], f'{kind}: the preparation stream held')
    for i in range(2):
        n = helpers.same_bits(got_b[i], want[i], f'{kind}: the main stream held, step {i + 1}')
    assert not torch.equal(want[0]['logits'], want[1]['logits'])
    torch.cuda.synchronize()
    _lib.ERR_WATCH.poll(block=True)
    print(f'FIGURE S3 {kind}: {n} elements per step equal')


# =================================================================================================================================
# S4: the staging ring
# =================================================================================================================================
# lengths of 3 * STAGING + 1 id lists: below the 512-word minimum buffer, and ONE of 600 words, which re-allocates its slot in the second round
STAGE_LENGTHS = [5 + 3 * i for i in range(3 * CONST['STAGING'] + 1)]
STAGE_LENGTHS[CONST['STAGING'] + 2] = 600


@pytest.mark.gpu
def test_staging_ring_under_a_held_stream_keeps_every_id_list():
    """3 * STAGING + 1 batches of distinct ids while the copies are pending.  The (STAGING + 1)-th call waits on the host for the first slot's
    event BY DESIGN, which ends the hold: so the hold is asserted pending behind the STAGING-th call, not at the end.  Every batch's device
    ids equal the ids it was given; the first and the last batch gather and build the graph of the host-packed batch."""
    import test_device_store as DS
    K = hip()
    S = CONST['STAGING']
    h = DS._special(20)
    d = h.device('cuda')
    rng = np.random.RandomState(4)
    lists = [rng.randint(0, len(d), size=n) for n in STAGE_LENGTHS]
    lists[0], lists[-1] = np.array([6, 0, 8, 2, 5]), np.array([3, 7, 1, 3, 8, 0, 4])
    torch.cuda.synchronize()
    holds = _hold('b', 'S4')
    t0 = time.perf_counter()
    batches = [d.batch(ids, 1) for ids in lists[:S]]
    ms = (time.perf_counter() - t0) * 1e3
    helpers.check_under_hold(*holds)
    print(f'FIGURE enqueue S4 {S} batches: {ms:.2f} ms on the host under a hold of {holds[0].ms} ms')
    batches += [d.batch(ids, 1) for ids in lists[S:]]
    holds[0].release_wait()
    torch.cuda.synchronize()
    for i, (sb, ids) in enumerate(zip(batches, lists)):
        assert sb.ids.dtype == torch.int32 and np.array_equal(sb.ids.cpu().numpy(), ids.astype(np.int32)), f'batch {i} of {len(lists)}: its ids on the device'
    assert d._ring[(S + 2) % S][0].numel() == 600 and d._ring[0][0].numel() == 512
    for sb, ids in ((batches[0], lists[0]), (batches[-1], lists[-1])):
        ids = ids.tolist()
        for got, want in zip(sb.fields(), h.fields()):
            assert torch.equal(got.cpu(), want[ids])
        DS._both_graphs(K, h, d, ids, int(h.store.edge_count[ids].sum()), f'ids {ids}')


# =================================================================================================================================
# S5: the replayed update
# =================================================================================================================================
# The runtime's launch of a captured graph waits ON THE HOST once about ten replays are pending behind a busy stream (measured: under one
# main hold the first ten launches of the window form took 0.8 .. 1.8 ms each, the eleventh 109 ms -- the rest of the hold -- inside
# CUDAGraph.replay(); no call of the package waits, and one mini-batch per update, four replays, never gets there).  That is a queue depth,
# not an ordering: so no hold of S5 covers more than REPLAYS_PER_HOLD replays, and the window form's twelve go under two consecutive holds
# of two optimiser steps each.  The second hold is enqueued behind the first one's pending replays without a synchronisation of the device:
# only the first hold's own event is waited for.
REPLAYS_PER_HOLD = 8


def _s5_run(window, held, reload):
    """steps 1 .. 3 (4 with a reload) capture and are synchronised; then four optimiser steps (two, a reload of the checkpoint, two) on new
    batches, under main holds or synchronised one by one -> (snapshots behind each step, captures before and after)"""
    import test_graphed_update as GU
    run = GU.Run(True, window)
    tiny = [i for i, (shape, _) in enumerate(GU.TL.BATCHES['U']) if shape == 'tiny']
    caps = {GU.TL.capacity(GU.TL.host_batch('U', i)['E']) for i in tiny}
    assert len(caps) == 1, f'the mini-batches lie in the capacity buckets {caps}: a capture would fall inside the hold'
    run.minis = {t: [tiny[(window * (t - 1) + j) % len(tiny)] for j in range(window)] for t in range(1, 9)}
    for t in range(1, 9):
        for mb in run.minis[t]:
            run.batch(mb)
    first = 5 if reload else 4
    for t in range(1, first):
        run.opt_step(t)
        torch.cuda.synchronize()
    ckpt = copy.deepcopy({'model': run.model.state_dict(), 'opt': run.opt.state_dict()})
    torch.cuda.synchronize()
    n_graphs = run.step_fn.n_graphs
    steps = [first, first + 1, first, first + 1] if reload else list(range(first, first + 4))
    assert 6 in steps
    per_hold = 4 if 4 * window <= REPLAYS_PER_HOLD else 2  # optimiser steps under one hold
    assert per_hold * window <= REPLAYS_PER_HOLD
    snaps, holds, t0 = [], [], 0.0
    for i, t in enumerate(steps):
        if held and i % per_hold == 0:
            holds, t0 = _hold('b', 'S5'), time.perf_counter()
        if reload and i == 2:
            run.model.load_state_dict(ckpt['model'])
            run.opt.load_state_dict(copy.deepcopy(ckpt['opt']))
        snaps.append(run.snapshot(run.opt_step(t)))
        if not held:
            torch.cuda.synchronize()
        elif (i + 1) % per_hold == 0:  # the last launch under this hold has been enqueued
            ms = (time.perf_counter() - t0) * 1e3
            assert run.step_fn.n_graphs == n_graphs, f'{run.step_fn.n_graphs - n_graphs} captures inside the hold'
            helpers.check_under_hold(*holds)
            print(f'FIGURE enqueue S5 window {window}{", reload" if reload else ""} (b), steps {steps[i + 1 - per_hold:i + 1]}: {ms:.2f} ms on the '
                  f'host, {per_hold * window} replays under a hold of {holds[0].ms} ms')
            holds[0].release_wait()  # (the hold's own event: the replays behind it stay pending)
    torch.cuda.synchronize()
    return snaps, n_graphs, run.step_fn.n_graphs


@pytest.mark.gpu
@pytest.mark.parametrize('window', [1, 3])
@pytest.mark.parametrize('reload', [False, True], ids=['straight', 'reload'])
def test_replayed_updates_enqueued_under_a_held_stream_equal_the_synchronised_run(window, reload):
    """GraphedStep(model, nc, optimizer=opt, max_grad_norm=...) at d = 32, a learning rate that changes at every step; one mini-batch per
    update, and accumulate=True for three mini-batches of which the last has update=True.  Four optimiser steps across RAdam's change of
    branch at step 6 are enqueued while the main stream is held (the window form under two consecutive holds: REPLAYS_PER_HOLD):
    parameters, moments, buffers, logits, losses and the norm cloned behind each step equal the run that synchronises after every step.
    reload: load_state_dict of the model and the optimiser between the second and the third of them, inside a hold."""
    import test_graphed_update as GU
    GU.begin()
    want, _, _ = _s5_run(window, False, reload)
    got, before, after = _s5_run(window, True, reload)
    assert before == after, f'{after - before} captures inside the hold'
    for i, (g, w) in enumerate(zip(got, want)):
        n = GU.TL.same(g, w, f'window {window}, step {i + 1} of four inside the hold')
    assert not torch.equal(want[0]['loss 0'], want[1]['loss 0'])
    GU.end()
    print(f'FIGURE S5 window {window} reload {reload}: {n} tensors per step equal, {after} captures')


# =================================================================================================================================
# S6: the flag watch
# =================================================================================================================================
def _s6_graphs():
    import test_deferred_reductions as TD
    ei, et, nt, R, T = TD._graph(71, 60, 200, 3, 2)
    bad = ei.clone()
    bad[1, 17] = 60 + 5  # one edge endpoint outside the node rows: the device clamps it and raises the flag
    return (ei[:, :180].contiguous().cuda(), bad.cuda(), et.cuda(), nt.cuda(), R, T)  # (the good batch: 180 edges, the bad one 200)


@pytest.mark.gpu
def test_flag_watch_under_a_held_stream_neither_reads_early_nor_loses_a_flag():
    from qagnn_amd import _lib
    K = hip()
    W = _lib.ERR_WATCH
    W.poll(block=True)
    ei, bad, et, nt, R, T = _s6_graphs()
    torch.cuda.synchronize()
    assert not W.pending
    holds = _hold('b', 'S6')
    t0 = time.perf_counter()
    K.graph_prep(bad, et, nt, R, T)
    K.graph_prep(ei, et[:180].contiguous(), nt, R, T)
    W.poll()  # inside the hold: nothing has landed, nothing is read, nothing is dropped
    assert len(W.pending) == 2
    _enqueued(holds, t0, 'S6 eager (b)')
    assert [('E=200' in e[2], 'E=180' in e[2], int(e[1][0]) != 0) for e in W.pending] == [(True, False, True), (False, True, False)], \
        'the flag words in pinned memory: the bad batch\'s raised, the good batch\'s clear, in the order of the calls'
    with pytest.raises(RuntimeError, match=r'out-of-range input in the graph of the batch with N=60 node rows, E=200 edges') as err:
        W.poll(block=True)
    assert 'E=180' not in str(err.value)
    assert not W.pending
    W.poll(block=True)


@pytest.mark.gpu
def test_flag_watch_behind_replays_under_a_held_stream():
    """the same through GraphedStep: the flag words the replayed launches wrote are copied behind every replay (after_replay)"""
    import test_device_store as DS
    from qagnn_amd import _lib, data_utils, graphed
    hip()
    W = _lib.ERR_WATCH
    W.poll(block=True)
    h = DS._train_store()
    ids_good, ids_bad = DS.TRAIN_IDS['captured'], DS.TRAIN_IDS['same bucket']
    step = graphed.GraphedStep(DS._small_model(h.R).cuda().train(), DS.NC)

    def batch(ids, spoil):
        x = DS._inputs(h, ids, DS.NC, 'cuda')
        packed = DS._packed(h, ids, DS.NC)
        el = data_utils.EdgeListBatch.from_lists(*packed.nested_lists(), h.n)
        if spoil:
            el.edge_index[1, 3] = len(ids) * h.n + 9
        return x, el.to('cuda')
    (xg, g), (xb, b) = batch(ids_good, False), batch(ids_bad, True)
    step(xg['sent'], *xg['fields'], g, xg['labels'])  # the capture
    torch.cuda.synchronize()
    W.poll(block=True)
    n_graphs = step.n_graphs
    holds = _hold('b', 'S6')
    t0 = time.perf_counter()
    step(xb['sent'], *xb['fields'], b, xb['labels'])
    step(xg['sent'], *xg['fields'], g, xg['labels'])
    W.poll()
    pending = len(W.pending)
    _enqueued(holds, t0, 'S6 replays (b)')
    watched = len(next(iter(step._captured.values())).watched)  # flag blocks the captured launches write: one entry each behind every replay
    assert step.n_graphs == n_graphs and watched >= 1 and pending == 2 * watched, (step.n_graphs, watched, pending)
    # a replayed entry is named as the capture named it, so the name tells the flag block, not the batch: the batch is told by the position
    raised = [(e[2], int(e[1][0]) != 0) for e in W.pending]
    assert [r for _, r in raised[watched:]] == [False] * watched, f'the good batch, replayed second, raised a flag: {raised[watched:]}'
    assert [w for w, r in raised[:watched] if r] and all('the graph of the edge-list batch' in w for w, r in raised[:watched] if r), raised[:watched]
    with pytest.raises(RuntimeError, match='out-of-range input in the graph of the edge-list batch'):
        W.poll(block=True)
    assert not W.pending
    W.poll(block=True)
