"""One training step of the QA-GNN decoder as ONE hipGraph launch.

Why: a step is ~400-500 kernel launches.  At the reference's own operating point (mbs = 2 questions = 10 subgraphs,
run_qagnn__csqa.sh:16-17; qagnn.py:252-266) the GPU work is < 2 ms while Python + autograd + launch overhead is 5.5-6.6 ms
(DESIGN.md 6a): every batch below ~190 subgraphs is bound by the host, not by the kernels.  A captured graph replays the whole
forward + loss + backward with one host call.

What makes it legitimate for TRAINING (a new batch every step, not a replay of one batch):
  * shapes  -- every launch shape of the step depends on (B, n, edge CAPACITY) only: the graph arrives in static buffers laid out for
    `e_cap` >= E edges -- load-time blobs (qagnn_graph_from_blobs), the reference's int64 edge lists (qagnn_graph_prep_cap,
    include/qagnn_hip.h) or sample ids into a device-resident store (qagnn_store_gather + qagnn_graph_from_store INSIDE the captured
    graph: the static input is the id list) -- and the kernels read the batch's true edge count on the device.  One capture per capacity bucket (8 buckets
    per octave of E: <= 12.5 % slack) and kind of graph input;
  * inputs  -- static device buffers, refilled by `copy_` before each replay (the one host-to-device copy per tensor the eager path
    makes too);
  * dropout -- seeds are launch arguments, which a graph replays verbatim; the kernels mix in a device-side epoch word that the
    captured step advances as its last launch (qagnn_seed_epoch_advance), torch's own nn.Dropout registers its philox state with
    the graph: replay k draws masks no other replay draws;
  * BatchNorm running statistics and batch counters are updated by the captured kernels in place, once per replay;
  * gradients land in static `.grad` tensors (re-attached after every replay), ready for any optimiser; `accumulate=True` adds them
    into the parameters' running `.grad` instead (the reference accumulates `loss.backward()` over mini-batches of 2 questions before
    each `optimizer.step()`, qagnn.py:252-266), and `sent_vecs.requires_grad` makes the step return d loss / d sent_vecs for the LM
    encoder's backward (the reference backpropagates into the encoder after `unfreeze_epoch`);
  * input validation -- the flag words the captured preparation kernels write (out-of-range edge endpoint / relation / node type /
    concept id, clamped on the device) are copied to the host behind every replay and looked at before the next one
    (_lib.ERR_WATCH): a corrupt batch raises one step late, as on the eager path.

The captured work is exactly the eager step's launch sequence (same kernels, same order, side streams included): results are
bit-identical to the eager path on the same capacity-laid-out batch (tests/test_graphed.py).
"""
import math

import torch

from . import ops
from .data_utils import GRAPH_HOLDERS, EdgeListBatch


def edge_capacity(E, floor=1024):
    """Capacity bucket of an edge count: the next multiple of 2^(floor(log2 E) - 3), i.e. 8 buckets per octave."""
    E = max(int(E), floor)
    step = 1 << max(int(math.floor(math.log2(E))) - 3, 0)
    return (E + step - 1) // step * step


# ---- what a captured training step (GraphedStep) and a captured eval forward (inference.GraphedForward) share ----------------------
def as_holder(packed, who):
    """the graph input as one of data_utils.GRAPH_HOLDERS (the plain int64 pair becomes an EdgeListBatch without a count word of its own:
    the capture's static one is written)"""
    if isinstance(packed, GRAPH_HOLDERS):
        return packed
    assert isinstance(packed, (tuple, list)) and len(packed) == 2 and all(isinstance(t, torch.Tensor) for t in packed), \
        f'{who} takes the graph as a PackedGraphBatch, an EdgeListBatch, a StoreBatch or an (edge_index [2, E], edge_type [E]) pair'
    return EdgeListBatch(packed[0], packed[1], count=False)


def capture_dims(cids, packed):
    """(B, n) of a batch: the holder's own where it carries the node fields, else the caller's tensors'"""
    return (packed.B, packed.n) if packed.own_fields else (cids.size(0), cids.size(1))


def alloc_static_fields(c, packed, B, n, dev):
    """c.cids / nt / ns / al: static buffers of the four node tensors -- None for a holder with fields of its own (outputs of the captured
    gather)"""
    c.cids = c.nt = c.ns = c.al = None
    if not packed.own_fields:
        c.cids = torch.empty((B, n), dtype=torch.long, device=dev)
        c.nt = torch.empty((B, n), dtype=torch.long, device=dev)
        c.ns = torch.empty((B, n, 1), dtype=torch.float32, device=dev)
        c.al = torch.empty((B,), dtype=torch.long, device=dev)


def load_static_inputs(c, sent, cids, nt, ns, al, packed):
    """one non-blocking copy per tensor into the capture's static buffers, the graph through its holder's refill"""
    with torch.no_grad():
        c.sent.copy_(sent, non_blocking=True)
    if not c.packed.own_fields:
        c.cids.copy_(cids, non_blocking=True)
        c.nt.copy_(nt, non_blocking=True)
        c.ns.copy_(ns.reshape(c.ns.shape), non_blocking=True)
        c.al.copy_(al, non_blocking=True)
    c.packed.refill(packed)


def fetch_own_fields(c):
    """a holder with fields of its own: the gather is part of the captured work, it reads the static id buffer and the model consumes its
    outputs in place"""
    if c.packed.own_fields:
        c.packed.reset()
        c.cids, c.nt, c.ns, c.al = c.packed.fields()


def warm_up(dev, times, fn):
    """`times` runs of fn outside the capture (lazy initialisation: operand-packing plans, LDS attribute raises, allocator pools), on a side
    stream as torch's capture recipe asks"""
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(times):
            fn()
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize(dev)


def capture_graph(pool, watched, fn, tables):
    """-> (graph, fn's result) with fn's launches captured; the flag tensors of the captured preparation kernels land in `watched` (kept
    alive, read behind every replay), the (frozen table, maximum word) pairs whose word the graph reads (ops.table_amax) in `tables`
    (brought up to date in front of every replay)"""
    from ._lib import ERR_WATCH
    graph = torch.cuda.CUDAGraph()
    ERR_WATCH.sink = watched
    try:
        with ops.table_words(tables), torch.cuda.graph(graph, pool=pool):
            out = fn()
    finally:
        ERR_WATCH.sink = None
    return graph, out


def capture_or_fall_back(owner, who, capture):
    """capture(); a capture that rejects the forked side streams is taken again on one stream (owner.overlap off: same launches, no overlap
    inside the graph)"""
    try:
        return capture()
    except RuntimeError as e:
        if not owner.overlap:
            raise
        import warnings
        warnings.warn(f'{who}: capture with side streams failed ({str(e)[:300]}); capturing on one stream')
        owner.overlap = False
        torch.cuda.synchronize(owner.dev)
        return capture()


def replay(c, load):
    """the previous replays' validation flags that have landed (a corrupt batch raises here, one call late), the refill, the maxima of
    frozen tables that were loaded anew since the last replay, the launch"""
    from ._lib import ERR_WATCH
    ERR_WATCH.poll()
    load()
    ops.refresh_table_words(c.tables)
    c.graph.replay()
    c.replays += 1
    ERR_WATCH.after_replay(c.watched)


class _Captured:
    # packed: the static twin of the graph input (data_utils: static_twin / refill), the holder the captured step reads
    __slots__ = ('graph', 'sent', 'cids', 'nt', 'ns', 'al', 'labels', 'lw', 'packed', 'logits', 'attn', 'loss', 'grads', 'replays', 'params', 'watched', 'sent_grad', 'tables')


# ---- the optimiser step inside the capture (GraphedStep(optimizer=...)) -----------------------------------------------------------------
EAGER_TAIL = 'clip_grad_norm_(..., defer_to=opt) then opt.step()'


def in_graph_update_plan(model, optimizer):
    """[(parameter, its group of the optimiser)] over the trainable parameters of `model`, in model.parameters() order (the order the norm's
    partial sums are taken in: that of clip_grad_norm_(model.parameters(), ...)) -- or the refusal.  Host only, nothing is enqueued; works on
    CPU tensors, which is how the refusals are tested."""
    from .optimization_utils import RAdam
    if not isinstance(optimizer, RAdam):
        raise TypeError(f'GraphedStep(optimizer=...) takes a {RAdam.__module__}.RAdam, whose update has a capturable form; got '
                        f'{type(optimizer).__name__} (run every other optimiser behind the step: {EAGER_TAIL})')
    if optimizer._grad_scale is not None:
        raise ValueError('the optimiser holds a pending defer_grad_scale (clip_grad_norm_(..., defer_to=opt) without its opt.step()): the '
                         'captured update computes its own coefficient and would leave that one to a later step')
    own = {id(p) for p in model.parameters()}
    group_of = {}
    for group in optimizer.param_groups:
        for p in group['params']:
            if p.requires_grad and id(p) not in own:
                raise ValueError(f'the optimiser holds a trainable parameter {tuple(p.shape)} that is no parameter of the captured model (the '
                                 f'unfrozen encoder: its gradient is produced outside the capture); use the eager tail: {EAGER_TAIL}')
            group_of[id(p)] = group
    plan = []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if id(p) not in group_of:
            raise ValueError(f'{name} is trainable and the optimiser does not hold it: the captured update would leave it behind')
        tensors = [(name, p)]
        st = optimizer.state.get(p)
        if st:
            tensors += [(f'{k} of {name}', st[k]) for k in ('exp_avg', 'exp_avg_sq')]
        for what, t in tensors:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != p.shape:
                raise ValueError(f'{what}: the captured update takes contiguous fp32 tensors of the parameter\'s shape, got {t.dtype} '
                                 f'{tuple(t.shape)} with strides {t.stride()}; use the eager tail: {EAGER_TAIL}')
        plan.append((p, group_of[id(p)]))
    return plan


class _Tail:
    """The static state of the captured tail for ONE set of trainable parameters, shared by the captures of every capacity bucket (a window
    spans buckets): params / groups (the plan; a group by its INDEX, load_state_dict() replaces the dicts), m / v (the optimiser's own moment
    tensors), records (device, one qagnn_step_record per
    tensor), first (device word: the next accumulation opens a window) and the value it was last given, window (the running sum; None
    until the first accumulate=True call), ws / out2 (workspace and result of the norm)."""
    __slots__ = ('params', 'groups', 'm', 'v', 'records', 'first', 'first_host', 'window', 'ws', 'out2')


class GraphedStep:
    """step = GraphedStep(model, num_choice);  logits, loss = step(sent_vecs, concept_ids, node_type_ids, node_scores, adj_lengths,
    packed, labels, loss_weight)  -- the flattened [B, ...] decoder inputs of QAGNN.forward (reference modeling_qagnn.py:141-189), the
    graph as a data_utils.PackedGraphBatch (device or host buffer), a data_utils.EdgeListBatch, the reference's plain
    (edge_index [2, E], edge_type [E]) int64 pair (device or host, pinned or not) or a data_utils.StoreBatch (the four node tensors may
    then be None: the captured graph gathers them from the store itself), labels [B / num_choice].

    loss = cross_entropy(logits.view(-1, nc), labels) * loss_weight  (the reference's mini-batch loss, qagnn.py:257-261);
    GraphedStep(..., loss='cross_entropy' | 'margin_rank', margin=0.1) computes it with ops.choice_loss instead -- one launch for the loss,
    the weight and the gradient, either of the reference's --loss kinds -- and adds every replayed loss to `step.meter` (losses.LossMeter:
    `step.meter.read()` -> (sum, count) with one synchronisation; the reference's total_loss without an .item() per mini-batch);
    after the call every trainable parameter's .grad holds this step's gradient (zero_grad implicit), or -- accumulate=True -- the
    running sum of the window's steps (the first step of a window is the one that finds .grad None, e.g. after
    optimizer.zero_grad(set_to_none=True)).  sent_vecs.requires_grad: `step.sent_grad` holds d loss / d sent_vecs afterwards.
    The set of trainable parameters is read at every call (freeze_net / unfreeze_net change it): one capture per set."""

    def __init__(self, model, num_choice, capacity=edge_capacity, warmup=2, loss=None, margin=0.1, optimizer=None, max_grad_norm=None):
        from .losses import LossMeter, check_loss_name
        if optimizer is not None:
            from .optimization_utils import RAdam
            if not isinstance(optimizer, RAdam):
                raise TypeError(f'GraphedStep(optimizer=...) takes a {RAdam.__module__}.RAdam, whose update has a capturable form; got '
                                f'{type(optimizer).__name__} (run every other optimiser behind the step: {EAGER_TAIL})')
        # the tail of the reference's loop inside the capture (qagnn.py:267-278): max_grad_norm None or <= 0 is no clipping (:267)
        self.optimizer = optimizer
        self.max_grad_norm = float(max_grad_norm) if max_grad_norm is not None and max_grad_norm > 0 else None
        self.grad_norm = None    # behind an update=True call: the window's total norm, a 0-dim device tensor (None without clipping)
        self._tails = {}         # trainable set -> _Tail
        self._window = None      # the _Tail whose window is open (the host knows the window state)
        self._outside = None     # (the optimiser's parameters that are none of the model's, how many it held when they were listed)
        self.loss, self.margin = (None if loss is None else check_loss_name(loss)), float(margin)
        self.model, self.nc, self.capacity, self.warmup = model, int(num_choice), capacity, int(warmup)
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.sent_grad = None
        self.dev = self.params[0].device
        assert self.dev.type == 'cuda', 'GraphedStep captures a HIP graph: the model must live on the GPU'
        self.meter = LossMeter(self.dev) if self.loss is not None else None  # (sum, count) of the replayed losses, on the device
        self._captured = {}
        self._pool = None
        # Side streams inside the capture.  Graph preparation under the input GEMM pays (-2 % at 65 subgraphs, more below); the
        # weight-gradient products on a stream of their own do NOT pay in a replayed graph: every fork / join is a cross-queue
        # dependency of the graph, and at 10 / 65 / 150 subgraphs the step is 6 % slower / equal / 2 % slower with them
        # (profiles/r3_run13_graph_overlap_ab.txt) -- so the captured step keeps them in the chain.
        self.overlap = True            # graph preparation on its side stream inside the capture; switched off if a capture rejects it
        self.wgrad_overlap = False     # (see above: measured, not taken)

    # -- the eager step that gets captured -------------------------------------------------------------------------------------------
    def _step(self, c):
        fetch_own_fields(c)
        logits, attn = self.model(c.sent, c.cids, c.nt, c.ns, c.al, c.packed)
        if self.loss is None:
            loss = torch.nn.functional.cross_entropy(logits.view(-1, self.nc), c.labels) * c.lw
        else:  # one launch: the loss times the weight word, its gradient, the meter's two doubles
            loss = ops.choice_loss(logits.view(-1, self.nc), c.labels, self.loss, self.margin, c.lw, self.meter.stats)
        loss.backward()
        return logits, attn, loss

    def _key(self, sent, cids, packed, trainable=None):
        if trainable is None:
            trainable = tuple(i for i, p in enumerate(self.model.parameters()) if p.requires_grad)
        B, n = capture_dims(cids, packed)
        return (B, n, sent.size(1), int(self.capacity(packed.E)), bool(self.model.training), bool(sent.requires_grad), hash(trainable), packed.capture_kind())

    # -- the optimiser step inside the capture ------------------------------------------------------------------------------------------
    def _tail(self, trainable):
        """the _Tail of the current trainable set -- or a refusal, on the host with nothing enqueued"""
        opt = self.optimizer
        if opt._grad_scale is not None:
            raise ValueError('the optimiser holds a pending defer_grad_scale (clip_grad_norm_(..., defer_to=opt) without its opt.step()): the '
                             'captured update computes its own coefficient and would leave that one to a later step')
        held = sum(len(g['params']) for g in opt.param_groups)
        if self._outside is None or self._outside[1] != held:
            own = {id(p) for p in self.model.parameters()}
            self._outside = [p for g in opt.param_groups for p in g['params'] if id(p) not in own], held
        tail = self._tails.get(trainable)
        if tail is not None and not any(p.requires_grad for p in self._outside[0]):
            return tail
        plan = in_graph_update_plan(self.model, opt)  # (raises what the line above saw)
        from . import _step
        S, dev = _step.kernels(), self.dev
        tail = _Tail()
        index = {id(g): i for i, g in enumerate(opt.param_groups)}
        tail.params, tail.groups = [p for p, _ in plan], [index[id(g)] for _, g in plan]
        for p in tail.params:  # the moments as RAdam.step() creates them, now: their addresses go into the captures
            st = opt.state[p]
            if len(st) == 0:
                st['step'] = 0
                st['exp_avg'] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                st['exp_avg_sq'] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
        tail.m = [opt.state[p]['exp_avg'] for p in tail.params]
        tail.v = [opt.state[p]['exp_avg_sq'] for p in tail.params]
        tail.records = torch.zeros(len(plan) * _step.RECORD_WORDS, dtype=torch.float32, device=dev)
        tail.first = torch.zeros(1, dtype=torch.int32, device=dev)
        tail.first_host = 0
        tail.window = None
        tail.ws = torch.zeros(S.grad_norm_workspace_elems(tail.params), dtype=torch.float32, device=dev)
        tail.out2 = torch.zeros(2, dtype=torch.float32, device=dev)
        if not self._tails:
            # every kernel of the tail once on scratch words, outside any capture: the warm-up runs of a capture stop behind the backward
            # (an update that ran there would stay), so no launch of the tail is the first of its kind inside a capture
            w = [torch.zeros(1, dtype=torch.float32, device=dev) for _ in range(4)]
            rec = torch.zeros(_step.RECORD_WORDS, dtype=torch.float32, device=dev)
            S.records_write(rec, [dict(decay=0.0, s=0.0, mode=0, beta1=0.0, beta2=0.0, ob1=0.0, ob2=0.0, eps=0.0)])
            S.window_accumulate(w[:1], w[1:2], tail.first)
            S.grad_norm_into(w[1:2], 1.0, tail.ws, tail.out2)
            S.radam_step_records(w[:1], w[1:2], w[2:3], w[3:4], [0], rec)
            S.radam_step_records(w[:1], w[1:2], w[2:3], w[3:4], [0], rec, grad_scale=tail.out2[1:2])
            tail.out2.zero_()
        self._tails[trainable] = tail
        return tail

    def _tail_launches(self, kind, tail, c):
        """behind the backward, inside the capture: the window, the norm and its coefficient, the update (the seed epoch follows)"""
        from . import _step
        S = _step.kernels()
        src = [p.grad for p in c.params]
        assert all(g is not None and g.dtype == torch.float32 and g.is_contiguous() for g in src), 'a trainable parameter received no fp32 gradient during capture'
        if kind != 'update':
            S.window_accumulate(tail.window, src, tail.first)
            src = tail.window
        if kind == 'accumulate':
            return
        scale = None
        if self.max_grad_norm is not None:
            S.grad_norm_into(src, self.max_grad_norm, tail.ws, tail.out2)
            scale = tail.out2[1:2]
        S.radam_step_records(tail.params, src, tail.m, tail.v, list(range(len(tail.params))), tail.records, grad_scale=scale)

    def _before_replay(self, kind, tail):
        """what the replay reads and a replay cannot carry: the first-of-window word and, for an update, every tensor's record.  Both are
        written by launches on the replay's stream whose values travel in their own arguments: a replay that is still pending keeps what
        was written in front of it.  The step counts advance here, on the host, as Python ints."""
        if kind != 'update':
            first = 1 if self._window is None else 0
            if tail.first_host != first:
                tail.first.fill_(first)
                tail.first_host = first
        if kind == 'accumulate':
            return
        from . import _step
        from .optimization_utils import radam_record
        opt, values, seen = self.optimizer, [], {}
        with torch.no_grad():
            for i, (p, gi) in enumerate(zip(tail.params, tail.groups)):
                st = opt.state[p]
                if len(st) == 0:  # (the state was dropped: start over, in the static moments)
                    st['step'] = 0
                    st['exp_avg'], st['exp_avg_sq'] = tail.m[i].zero_(), tail.v[i].zero_()
                elif st['exp_avg'] is not tail.m[i] or st['exp_avg_sq'] is not tail.v[i]:
                    # load_state_dict() under live captures: the captured update holds the addresses of the moments it was given, so the
                    # loaded ones are copied into those (stream-ordered, behind every pending replay) and the state points at them again
                    st['exp_avg'], st['exp_avg_sq'] = tail.m[i].copy_(st['exp_avg']), tail.v[i].copy_(st['exp_avg_sq'])
                st['step'] = int(st['step']) + 1
                at = (gi, st['step'])
                if at not in seen:
                    seen[at] = radam_record(opt.param_groups[gi], st['step'], opt.degenerated_to_sgd)
                values.append(seen[at])
        _step.kernels().records_write(tail.records, values)

    def _capture(self, key, args, kind='plain', tail=None):
        B, n, sent_dim, e_cap, _, sent_rg = key[:6]
        sent, cids, nt, ns, al, packed, labels, lw = args
        dev, K = self.dev, ops.kernels()
        c = _Captured()
        c.params = [p for p in self.model.parameters() if p.requires_grad]
        c.watched, c.tables, c.sent_grad = [], [], None
        c.sent = torch.empty((B, sent_dim), dtype=torch.float32, device=dev, requires_grad=sent_rg)
        alloc_static_fields(c, packed, B, n, dev)
        c.labels = torch.empty((B // self.nc,), dtype=torch.long, device=dev)
        c.lw = torch.ones((), dtype=torch.float32, device=dev)
        c.packed = packed.static_twin(B, n, e_cap, dev)  # the graph input in static buffers laid out for the bucket's capacity
        c.replays = 0
        self._load(c, args)
        # warm-up outside the capture; module buffers (BatchNorm running statistics, batch counters) are put back afterwards
        saved = [(b, b.detach().clone()) for b in self.model.buffers()]
        held = [p.grad for p in c.params]  # a capture in the middle of an accumulation window must not lose the window's gradients
        metered = self.meter.stats.clone() if self.meter is not None else None  # (the warm-up steps add their losses: put back)
        old = ops.WGRAD_OVERLAP, ops.PREP_OVERLAP
        ops.WGRAD_OVERLAP = ops.WGRAD_OVERLAP and self.wgrad_overlap and self.overlap
        ops.PREP_OVERLAP = ops.PREP_OVERLAP and self.overlap

        def fresh_step():
            for p in c.params:
                p.grad = None
            c.sent.grad = None
            return self._step(c)

        def step_and_advance():
            out = self._step(c)
            if kind != 'plain':
                self._tail_launches(kind, tail, c)
            K.seed_epoch_advance(1)  # the next replay draws different dropout masks
            return out

        try:
            warm_up(dev, self.warmup, fresh_step)
            with torch.no_grad():
                for b, v in saved:
                    b.copy_(v)
                if metered is not None:
                    self.meter.stats.copy_(metered)
            for p in c.params:
                p.grad = None
            c.sent.grad = None
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            c.graph, (c.logits, c.attn, c.loss) = capture_graph(self._pool, c.watched, step_and_advance, c.tables)
        finally:
            ops.WGRAD_OVERLAP, ops.PREP_OVERLAP = old
        c.grads = [p.grad for p in c.params]
        c.sent_grad = c.sent.grad if sent_rg else None
        for p, g in zip(c.params, held):
            p.grad = g
        assert all(g is not None for g in c.grads), 'a trainable parameter received no gradient during capture'
        self._captured[key] = c
        return c

    def _load(self, c, args):
        sent, cids, nt, ns, al, packed, labels, lw = args
        c.labels.copy_(labels, non_blocking=True)
        c.lw.fill_(float(lw))
        load_static_inputs(c, sent, cids, nt, ns, al, packed)

    def __call__(self, sent_vecs, concept_ids, node_type_ids, node_scores, adj_lengths, packed, labels, loss_weight=1.0, accumulate=False,
                 update=False):
        if update and self.optimizer is None:
            raise ValueError('GraphedStep(update=True) needs the optimiser the captured step is to run: GraphedStep(model, nc, optimizer=opt)')
        packed = as_holder(packed, 'GraphedStep')
        args = (sent_vecs, concept_ids, node_type_ids, node_scores, adj_lengths, packed, labels, loss_weight)
        if self.optimizer is not None and (accumulate or update):
            return self._call_with_tail(args, update)
        key = self._key(sent_vecs, concept_ids, packed)
        with torch.cuda.device(self.dev):
            c = self._captured.get(key)
            if c is None:
                c = capture_or_fall_back(self, 'GraphedStep', lambda: self._capture(key, args))
            replay(c, lambda: self._load(c, args))
            self.params, self.sent_grad = c.params, c.sent_grad
            if accumulate:
                # the static gradients are overwritten by the next replay: the window's sum lives in tensors of its own
                dst, src = [], []
                static = {id(g) for cc in self._captured.values() for g in cc.grads}  # a .grad that IS one of these holds one step
                for p, g in zip(c.params, c.grads):
                    if p.grad is None or id(p.grad) in static:
                        p.grad = g.clone()
                    else:
                        dst.append(p.grad)
                        src.append(g)
                if dst:
                    torch._foreach_add_(dst, src)
                return c.logits, c.loss
        for p, g in zip(c.params, c.grads):
            p.grad = g
        return c.logits, c.loss

    def _call_with_tail(self, args, update):
        """A mini-batch whose captured graph goes on behind the backward.  Three kinds of capture per bucket:
          'accumulate'     window = first ? gradient : window + gradient                          (accumulate=True, update=False)
          'update_window'  the same (a window is open), then norm, coefficient and update on the WINDOW   (update=True)
          'update'         norm, coefficient and update on the capture's own static gradients: no window buffer is touched (update=True and
                           no window open -- one mini-batch per optimiser step)"""
        sent_vecs, concept_ids, packed = args[0], args[1], args[5]
        trainable = tuple(i for i, p in enumerate(self.model.parameters()) if p.requires_grad)
        with torch.cuda.device(self.dev):
            tail = self._tail(trainable)
            if self._window is not None and self._window is not tail:
                raise ValueError('the set of trainable parameters changed inside an accumulation window: close the window (update=True) first')
            kind = 'accumulate' if not update else ('update' if self._window is None else 'update_window')
            key = self._key(sent_vecs, concept_ids, packed, trainable) + (kind,)
            if tail.window is None and kind == 'accumulate':
                tail.window = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in tail.params]
            c = self._captured.get(key)
            if c is None:
                c = capture_or_fall_back(self, 'GraphedStep', lambda: self._capture(key, args, kind, tail))

            def load():
                self._load(c, args)
                self._before_replay(kind, tail)

            replay(c, load)
            self.params, self.sent_grad = c.params, c.sent_grad
            self._window = tail if kind == 'accumulate' else None
            for p, g in zip(c.params, c.grads if kind == 'update' else tail.window):
                p.grad = g  # the window's unclipped gradient (as with defer_to=): the next call opens a new window, zero_grad is implicit
            if update:
                self.grad_norm = tail.out2[0] if self.max_grad_norm is not None else None
        return c.logits, c.loss

    @property
    def n_graphs(self):
        return len(self._captured)
