"""The model TOGETHER with its optimiser: a short training run, step by step.

The loop is the reference's (qagnn.py:252-278): GraphedStep(model, nc, loss=kind) on a fresh batch (loss weight 1.0 on odd steps, 0.5 on
even ones), optimization_utils.clip_grad_norm_, the warm-up learning rate lr min(1, t / 3), RAdam.step() with the reference's two
parameter groups (weight decay 0.01; none for biases and BatchNorm weights), T = 7 steps: RAdam takes its SGD-with-momentum branch at
steps 1 .. 5 and the rectified one from step 6.

Shapes: S = GOLDEN_CASES['small_train'] (d = 32, k = 2, 6 subgraphs of 20 nodes), M = config1_train with two questions (d = 200 -> padded
width 208, k = 5, 10 subgraphs of 100 nodes).  Every step has its own seeded batch; the record shape changes at step 4, so that under the
256-edge capacity buckets a second bucket -- a capture in the middle of the run -- first appears there.

  1. `-m gpu`  the replayed loop == the eager loop on the same capacity layout, bit for bit, after every step: logits, loss, norm, every
     gradient, parameter, moment, step count and buffer; a parameter frozen at step 4 and unfrozen at step 6.
  2. each step against the float64 oracle, TEACHER-FORCED: the oracle gets the run's state before the step, then that one step is held
     to the project's bars (FWD for the logits, the loss kernel's bound, F64Ref.check_all with aligned ReLU kinks, the norm bar of
     test_grad_clip, the RAdam tolerances of test_grad_clip against oracle.radam_oracle, the buffer bar of test_hip_parity).  A free-running
     fp32 trajectory cannot be compared with a float64 one beyond step 5: the rectified branch normalises rounding-noise gradients to
     +-lr.  The same harness runs without a GPU at S on the eager loop over the emulation provider.
  3. `-m gpu`  one GraphedForward for the whole run, captured after step 2 and replayed after step 7.
  4. `-m gpu`  checkpoint after step 4, resume in fresh objects and fresh captures: steps 5 .. 7 bit for bit.
  5. `-m gpu`  load_state_dict under live captures (a 64 times larger frozen entity table: ops.table_amax).
  6. `-m gpu`  the run with the run scripts' dropout is reproducible.

QAGNN_LOOP_TEST_LOG names a file that collects the figures (the worst fraction of every bar, per step and case).
"""
import math
import os
import re
import time

import numpy as np
import pytest
import torch

import helpers
from emu_loss import EmuLossKernels
from oracle import radam_oracle as RO
from qagnn_amd import _lib, data_utils, graphed, inference, losses, ops, synthetic
from qagnn_amd import modeling_qagnn as MQ
from qagnn_amd import optimization_utils as OU
from test_grad_clip import norm_bar, torch_clip_f64
from test_hip_parity import RUN_SCRIPT_DROPOUT
from test_host_logic_emu import FWD

T_STEPS, LR, WD, MARGIN, BUCKET = 7, 1e-3, 0.01, 0.1, 256
LOG = os.environ.get('QAGNN_LOOP_TEST_LOG')

SHAPES = {'S': dict(helpers.GOLDEN_CASES['small_train']), 'M': dict(helpers.GOLDEN_CASES['config1_train'], nq=2)}
# (record shape, seed) of the batch of step 1 .. 7, then of the evaluation batch.  Edge counts: S 138 142 130 | 352 | 136 | 414 | 156 (buckets
# 256 256 256 512 256 512 256), M 8000 8000 7948 | 6060 | 8000 | 6004 | 8000 (8192 8192 8192 6144 8192 6144 8192): the second bucket first
# appears at step 4, and step 3 of M is another edge count in the first bucket.  (Every step of both shapes under either loss has active
# margin pairs and a gradient norm of 1.6 .. 8: max_norm = 1 clips at every step.)
BATCHES = {'S': [('tiny', 100), ('tiny', 101), ('tiny', 102), ('csqa', 103), ('tiny', 104), ('csqa', 102), ('tiny', 105), ('tiny', 106)],
           'M': [('config1', 100), ('config1', 101), ('csqa', 102), ('csqa', 103), ('config1', 104), ('csqa', 104), ('config1', 105), ('config1', 106)]}
SECOND_BUCKET_AT = 4
ORACLE_STEPS = {'S': tuple(range(1, T_STEPS + 1)), 'M': (1, 6, 7)}  # (the oracle costs ~0.4 s a pass at M)
# besides helpers.has_null_gradient: both losses depend on differences of a question's logits only, which is all the head's two output
# biases move -- their exact gradient is 0 (tests/test_hip_parity.py, bench_size_step_vs_oracle)
SHIFT_ONLY = ('fc.layers.0-Linear.bias', 'pooler.w_vs.bias')
NO_DECAY = re.compile(r'bias$|(edge_encoder|mlp)\.1\.weight$')  # biases and BatchNorm weights
ZERO_P = dict(p_emb=0.0, p_gnn=0.0, p_fc=0.0, p_attn=0.0, p_pool=0.0)


def capacity(E):
    return max(BUCKET, -(-int(E) // BUCKET) * BUCKET)


def note(line):
    print(line)
    if LOG:
        with open(LOG, 'a') as f:
            f.write(line + '\n')


def hip():
    ops.set_kernels(None)
    return ops.kernels()


@pytest.fixture
def form(request):
    yield from helpers.apply_form(request.param)


# ---- batches, models, the loop -----------------------------------------------------------------------------------------------------------
_HOST = {}


def host_batch(shape, i):
    """batch i (0-based; T_STEPS = the evaluation batch) of a shape as host tensors; built once"""
    if (shape, i) in _HOST:
        return _HOST[shape, i]
    c, (rshape, seed) = SHAPES[shape], BATCHES[shape][i]
    cfg, nq, nc, n = c['cfg'], c['nq'], c['nc'], c['n']
    B = nq * nc
    recs = synthetic.make_records(B, seed=seed, shape=rshape, n_rel=c['n_rel'], n_concept_vocab=cfg['n_concept'])
    _, cids, nt, ns, al, ei, et, _ = data_utils.records_to_tensors(recs, n, nc)
    store = data_utils.GraphBlobStore.build(ei, et, nt, cfg['n_etype'], cfg['n_ntype'])
    buf, Bb, E = store.pack(list(range(B)))
    bei, bet = data_utils.batch_graph(ei, et, n)
    assert Bb == B and bei.size(1) == E
    g = torch.Generator().manual_seed(seed + 1000)
    _HOST[shape, i] = dict(sent=torch.randn(B, cfg['sent_dim'], generator=g), labels=torch.randint(0, nc, (nq,), generator=g),
                           cids=cids.view(B, n), nt=nt.view(B, n), ns=ns.view(B, n, 1), al=al.view(B), ei=bei, et=bet, buf=buf, B=B, E=E,
                           store=store, nc=nc)
    return _HOST[shape, i]


def on(hb, dev, e_cap=None):
    """a host batch on a device; 'graph' = the blobs (e_cap: in a buffer laid out for e_cap edges, as a capture's static twin is) on the GPU,
    the reference's (edge_index, edge_type) pair on the CPU"""
    b = {k: hb[k].to(dev) for k in ('sent', 'labels', 'cids', 'nt', 'ns', 'al')}
    b['E'], b['host'] = hb['E'], hb
    if torch.device(dev).type == 'cpu':
        b['graph'] = (hb['ei'], hb['et'])
        return b
    buf = hb['buf'].to(dev)
    packed = data_utils.PackedGraphBatch(buf, hb['B'], hb['E'], hb['store'], list(range(hb['B'])), hb['nc'])
    if e_cap is not None:
        blob = torch.zeros(packed.head + 2 * packed.n * packed.B + 3 * e_cap, dtype=torch.int32, device=dev)
        blob[:buf.numel()] = buf
        packed = data_utils.PackedGraphBatch(blob, hb['B'], hb['E'], hb['store'], list(range(hb['B'])), hb['nc'])
        packed.e_cap = e_cap
    b['graph'] = packed
    return b


def make_model(shape, dev, fill=None, ps=ZERO_P):
    c = SHAPES[shape]
    cfg = c['cfg']
    torch.manual_seed(0)
    m = MQ.QAGNN(None, cfg['k'], cfg['n_ntype'], cfg['n_etype'], cfg['sent_dim'], cfg['n_concept'], cfg['concept_dim'], cfg['concept_in_dim'],
                 cfg['n_attention_head'], cfg['fc_dim'], cfg['n_fc_layer'], ps['p_emb'], ps['p_gnn'], ps['p_fc'], pretrained_concept_emb=None,
                 freeze_ent_emb=True, init_range=cfg['init_range'])
    helpers.det_fill_(m, c['seed'] if fill is None else fill, c['std'])
    m.pooler.dropout.p, m.pooler.attention.dropout.p = ps['p_pool'], ps['p_attn']
    return m.to(dev).train()


def make_opt(model):
    named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    return OU.RAdam([dict(params=[p for k, p in named if not NO_DECAY.search(k)], weight_decay=WD),
                     dict(params=[p for k, p in named if NO_DECAY.search(k)], weight_decay=0.0)], lr=LR)


def loss_weight(t):
    return 1.0 if t % 2 else 0.5


def lr_at(t):
    return LR * min(1.0, t / 3.0)


class Loop:
    """model + RAdam + (replay) a GraphedStep; step t = forward_backward, clip, update"""

    def __init__(self, shape, kind, dev='cuda', replay=True, defer=True, max_norm=1.0, fill=None, ps=ZERO_P):
        self.shape, self.kind, self.dev, self.replay, self.defer, self.max_norm = shape, kind, dev, replay, defer, max_norm
        self.nc, self.d = SHAPES[shape]['nc'], SHAPES[shape]['cfg']['concept_dim']
        self.model = make_model(shape, dev, fill, ps)
        self.opt = make_opt(self.model)
        self.step_fn = graphed.GraphedStep(self.model, self.nc, capacity=capacity, loss=kind) if replay else None
        self.caps = []

    def batch(self, t):
        hb = host_batch(self.shape, t - 1)
        return on(hb, self.dev, None if self.replay else capacity(hb['E']))

    def forward_backward(self, b, t, rec=False):
        """-> (logits, loss[, the ReLU inputs of the forward: eager only])"""
        lw, self.t = loss_weight(t), t
        self.caps.append(capacity(b['E']))
        if self.replay:
            assert not rec
            return self.step_fn(b['sent'], b['cids'], b['nt'], b['ns'], b['al'], b['graph'], b['labels'], lw)
        for p in self.model.parameters():
            p.grad = None
        pre = None
        if rec:
            with helpers.recorded_forward(self.d) as pre:
                logits, _ = self.model(b['sent'], b['cids'], b['nt'], b['ns'], b['al'], b['graph'])
        else:
            logits, _ = self.model(b['sent'], b['cids'], b['nt'], b['ns'], b['al'], b['graph'])
        loss = losses.compute_loss(logits.view(-1, self.nc), b['labels'], self.kind, MARGIN, weight=lw)
        loss.backward()
        return (logits, loss, pre) if rec else (logits, loss)

    def clip(self):
        defer = self.t % 2 == 1 if self.defer == 'alternate' else self.defer  # 'alternate': deferred on odd steps, in place on even ones
        return OU.clip_grad_norm_(list(self.model.parameters()), self.max_norm, defer_to=self.opt if defer else None)

    def update(self, t):
        for g in self.opt.param_groups:
            g['lr'] = lr_at(t)
        self.opt.step()

    def step(self, t):
        logits, loss = self.forward_backward(self.batch(t), t)
        norm = self.clip()
        self.update(t)
        return logits, loss, norm

    def snapshot(self, logits=None, loss=None, norm=None):
        out = {}
        if logits is not None:
            out.update({'logits': logits.detach().clone(), 'loss': loss.detach().clone().reshape(-1), 'norm': norm.detach().clone()})
        for k, p in self.model.named_parameters():
            out['param ' + k] = p.detach().clone()
            if p.grad is not None:
                out['grad ' + k] = p.grad.detach().clone()
            st = self.opt.state.get(p)
            if st:
                out['exp_avg ' + k], out['exp_avg_sq ' + k] = st['exp_avg'].clone(), st['exp_avg_sq'].clone()
                out['step ' + k] = torch.tensor(int(st['step']))
        for k, v in self.model.named_buffers():
            out['buffer ' + k] = v.detach().clone()
        return out


def same(a, b, what, only=None):
    if only is not None:
        a, b = ({k: v for k, v in d.items() if k.split(' ')[0] in only} for d in (a, b))
    assert set(a) == set(b), f'{what}: {sorted(set(a) ^ set(b))[:6]}'
    keys = list(a)
    bad = [k for k in keys if not torch.equal(a[k].cpu(), b[k].cpu())]
    assert not bad, (f'{what}: {len(bad)} of {len(keys)} tensors differ, e.g. ' +
                     ', '.join(f'{k} ({(a[k].double().cpu() - b[k].double().cpu()).abs().max().item():.3e})' for k in bad[:4]))
    return len(keys)


def check_buckets(loop, n_extra=0):
    """the capacity buckets the run met, in order: a second one, first at SECOND_BUCKET_AT; one capture per bucket (+ n_extra)"""
    caps = loop.caps
    first_other = next(i + 1 for i, c in enumerate(caps) if c != caps[0])
    assert first_other == SECOND_BUCKET_AT >= 3, caps
    if loop.replay:
        assert loop.step_fn.n_graphs >= 2 and loop.step_fn.n_graphs == len(set(caps)) + n_extra, (loop.step_fn.n_graphs, caps)
    return first_other


# ---- 1. the replayed loop == the eager loop -----------------------------------------------------------------------------------------------
# (shape, loss, composed path, clip deferred, max_norm): every axis with each shape; max_norm 1 always clips (norms 4 .. 27), 1e9 never
GRID = [(s,) + g for s in ('S', 'M') for g in (('cross_entropy', False, True, 1.0), ('margin_rank', True, False, 1.0),
                                               ('margin_rank', False, True, 1e9))]


def _paired_run(shape, kind, composed, defer, max_norm, monkeypatch, freeze=None):
    hip()
    _lib.ERR_WATCH.poll(block=True)
    if composed:
        monkeypatch.setattr(ops, 'FUSED_HOP', False)
    eager = Loop(shape, kind, replay=False, defer=defer, max_norm=max_norm)
    rep = Loop(shape, kind, replay=True, defer=defer, max_norm=max_norm)
    n = 0
    for t in range(1, T_STEPS + 1):
        if freeze and t in freeze:  # (frozen at freeze[0], trainable again at freeze[1])
            for loop in (eager, rep):
                for p in loop.model.svec2nvec.parameters():
                    p.requires_grad_(t == freeze[1])
                    p.grad = None
        a, b = eager.snapshot(*eager.step(t)), rep.snapshot(*rep.step(t))
        n = same(b, a, f'step {t} ({shape} {kind}, E = {host_batch(shape, t - 1)["E"]}, capacity {rep.caps[-1]})')
        if max_norm == 1.0:
            assert float(a['norm']) > 1.0, 'max_norm = 1 was to clip at every step'
        assert eager.opt._grad_scale is None and rep.opt._grad_scale is None  # (the deferred coefficient is consumed by its one step)
    torch.cuda.synchronize()
    _lib.ERR_WATCH.poll(block=True)
    return eager, rep, n


@pytest.mark.gpu
@pytest.mark.parametrize('shape,kind,composed,defer,max_norm,form', helpers.with_forms(GRID), indirect=['form'])
def test_replayed_loop_equals_the_eager_loop(shape, kind, composed, defer, max_norm, form, monkeypatch):
    """7 steps of model + clip + RAdam, replayed and eager on the same capacity layout: bit-identical after every step.  A replay reads the
    weights the fused RAdam kernel wrote through raw pointers a step earlier; the second bucket's capture is taken at step 4 and its warm-up
    steps must leave weights, moments and buffers where training had them."""
    t0 = time.time()
    eager, rep, n = _paired_run(shape, kind, composed, defer, max_norm, monkeypatch)
    at = check_buckets(rep)
    steps = {int(st['step']) for st in rep.opt.state.values()}
    assert steps == {T_STEPS}
    note(f'LOOP replay==eager {shape} {kind} {"composed" if composed else "native"} {"deferred" if defer else "in place"} max_norm {max_norm:g} '
         f'[{form}]: {n} tensors x {T_STEPS} steps bit-identical, {rep.step_fn.n_graphs} captures, second bucket at step {at}, {time.time() - t0:.1f} s')


@pytest.mark.gpu
@pytest.mark.parametrize('shape,form', helpers.with_forms(['S']), indirect=['form'])
def test_replayed_loop_with_a_parameter_frozen_at_step_4_and_unfrozen_at_step_6(shape, form, monkeypatch):
    """svec2nvec frozen for steps 4 and 5: a capture of its own (per bucket met meanwhile) and step counts that lag by two afterwards, i.e.
    two (step, branch) buckets per parameter group inside one RAdam.step()."""
    eager, rep, n = _paired_run(shape, 'cross_entropy', False, True, 1.0, monkeypatch, freeze=(4, 6))
    frozen_caps = len(set(rep.caps[3:5]))
    check_buckets(rep, n_extra=frozen_caps)
    lag = {k: int(rep.opt.state[p]['step']) for k, p in rep.model.named_parameters() if p in rep.opt.state}
    assert {v for k, v in lag.items() if k.startswith('svec2nvec.')} == {T_STEPS - 2} and {v for k, v in lag.items() if not k.startswith('svec2nvec.')} == {T_STEPS}
    note(f'LOOP frozen 4..5 {shape} [{form}]: {n} tensors x {T_STEPS} steps bit-identical, {rep.step_fn.n_graphs} captures')


# ---- 2. each step against the float64 oracle, teacher-forced -------------------------------------------------------------------------------
def _state_before(loop):
    sd = {k: v.detach().cpu().clone() for k, v in loop.model.state_dict().items()}
    opt0 = {}
    for k, p in loop.model.named_parameters():
        st = loop.opt.state.get(p)
        opt0[k] = ((st['exp_avg'].cpu().numpy().astype(np.float64), st['exp_avg_sq'].cpu().numpy().astype(np.float64), int(st['step'])) if st
                   else (np.zeros(tuple(p.shape)), np.zeros(tuple(p.shape)), 0))
    return sd, opt0


def oracle_step(loop, t, twin=None):
    """step t of `loop` with everything held to the float64 oracle that starts from the run's own state -> {bar: worst fraction of it}"""
    shape, kind, dev, c = loop.shape, loop.kind, loop.dev, SHAPES[loop.shape]
    cfg, nc, lw, k_hops = c['cfg'], c['nc'], loss_weight(t), c['cfg']['k']
    hb = host_batch(shape, t - 1)
    b = loop.batch(t)
    sd0, opt0 = _state_before(loop)
    p0 = {k: p.detach().cpu().numpy().astype(np.float64) for k, p in loop.model.named_parameters()}
    if loop.replay:  # the ReLU inputs of the step: those of its eager twin (bit-identical: part 1) from the same state on the same layout
        logits, loss = loop.forward_backward(b, t)
        twin.load_state_dict(sd0)
        with helpers.recorded_forward(loop.d) as pre:
            tb = on(hb, dev, capacity(hb['E']))
            tl, _ = twin.train()(tb['sent'], tb['cids'], tb['nt'], tb['ns'], tb['al'], tb['graph'])
        assert torch.equal(tl, logits), 'the eager twin of the replayed step has other logits'
    else:
        logits, loss, pre = loop.forward_backward(b, t, rec=True)
    logits, loss = logits.detach().cpu().clone(), float(loss.detach())
    named = dict(loop.model.named_parameters())
    grads = {k: p.grad.detach().cpu().clone() for k, p in named.items() if p.grad is not None}
    word = ops.kernels().grad_norm([p.grad for p in named.values() if p.grad is not None], loop.max_norm).cpu() if dev != 'cpu' else None
    norm = loop.clip()
    if dev == 'cpu':  # (torch's own clip: its fp32 coefficient)
        coef = float(torch.clamp(loop.max_norm / (norm + 1e-6), max=1.0))
    else:
        assert torch.equal(norm.cpu(), word[0]), 'clip_grad_norm_ returned another norm than qagnn_grad_norm_f32 on the same gradients'
        coef = float(word[1])
    loop.update(t)
    fig = {}

    # -- the oracle from the same state
    case = dict(c, labels=hb['labels'], loss=kind, margin=MARGIN, loss_weight=lw, train=True)
    inputs = (hb['sent'], hb['cids'], hb['nt'], hb['ns'], hb['al'], hb['ei'], hb['et'])
    ref = helpers.F64Ref(case, 'train', inputs=inputs, prepare=lambda m: m.load_state_dict(sd0))
    ref.compute_yard()
    what = f'{shape} {kind} step {t}: '
    # logits: FWD against the fp32 oracle
    ref_logits = ref.forward32['::logits']
    admitted = FWD['atol'] + FWD['rtol'] * float(ref_logits.abs().max())
    fig['logits'] = helpers._close(logits, ref_logits, what=what + 'logits', **FWD) / admitted
    # loss: the kernel's bound on ITS logits + the loss of the admitted logit error (both losses move by at most 2 max|dx|)
    Q = hb['labels'].numel()
    want_loss = float(helpers.train_loss(ref_logits.double().view(Q, nc), hb['labels'], kind, MARGIN, lw))
    lb, _ = _lib.choice_loss_bound(kind, nc, Q, float(logits.abs().max()), MARGIN, lw)
    fig['loss'] = abs(loss - want_loss) / (lb + 2 * admitted)
    assert fig['loss'] <= 1.0, f'{what}loss {loss!r} vs {want_loss!r} (bound {lb:.3e} + 2 x {admitted:.3e})'
    # gradients: F64Ref.check_all, the run's ReLU masks at the kinks
    held = {k: g for k, g in grads.items() if k not in SHIFT_ONLY}
    report = ref.check_all(held, what=what + 'grad::', min_checked=math.ceil(0.8 * len(grads)), **helpers.kink_args(pre, cfg, hb['ei'], hb['et'], hb['nt']))
    fig['grad'] = max(r / (helpers.YARD_MULT * max(ref.yard[k][0] / (ref.yard[k][1] + 1e-300), ref.median_rel) + helpers.ABS_FLOOR) for k, r in report.items())
    fig['grad of scale'] = max(report.values())
    # total norm and clip coefficient against float64 on the run's own gradients
    want_norm, want_coef = torch_clip_f64(list(grads.values()), loop.max_norm)
    bar = norm_bar()
    assert abs(float(norm) - want_norm) <= bar * want_norm, f'{what}norm {float(norm)!r} vs {want_norm!r}'
    fig['norm'] = abs(float(norm) - want_norm) / (bar * want_norm) if want_norm > 0 else 0.0
    if loop.max_norm >= 1e9:
        assert want_coef == 1.0 and coef == 1.0, f'{what}coefficient {coef!r} where nothing is clipped'
        fig['coef'] = 0.0
    else:
        assert want_coef < 1.0, f'{what}max_norm = {loop.max_norm} was to clip (norm {want_norm})'
        fig['coef'] = abs(coef - want_coef) / ((bar + 2.0 ** -24) * want_coef)
        assert fig['coef'] <= 1.0, f'{what}coefficient {coef!r} vs {want_coef!r}'
    # the update: oracle.radam_oracle on the run's fp32 gradients times the float64 coefficient, at the group's learning rate of this step
    worst = dict(m=0.0, v=0.0, p=0.0)
    for group in loop.opt.param_groups:
        assert group['lr'] == lr_at(t)
        for p in group['params']:
            k = next(kk for kk, q in named.items() if q is p)
            if k not in grads:
                continue
            m0, v0, s0 = opt0[k]
            st = loop.opt.state[p]
            assert st['step'] == s0 + 1
            rp, rm, rv = RO.radam_step(p0[k], grads[k].numpy().astype(np.float64) * want_coef, m0, v0, s0 + 1, lr_at(t), weight_decay=group['weight_decay'])
            for key, got, want, atol in (('m', st['exp_avg'], rm, 3e-8), ('v', st['exp_avg_sq'], rv, 1e-10), ('p', p.detach(), rp, 1e-7)):
                got = got.cpu().numpy().astype(np.float64)
                assert np.isfinite(got).all(), f'{what}{key} of {k}'
                worst[key] = max(worst[key], float(np.max(np.abs(got - want) / (atol + 2e-6 * np.abs(want)))) if got.size else 0.0)
    fig.update({'exp_avg': worst['m'], 'exp_avg_sq': worst['v'], 'param': worst['p']})
    assert max(worst.values()) <= 1.0, f'{what}update |got - ref| / (atol + 2e-6 |ref|), atol 3e-8 / 1e-10 / 1e-7 for m / v / p: {worst}'
    # buffers: the oracle's after its own forward from the same previous buffers
    obuf = dict(ref.model.named_buffers())
    fig['buffer'] = 0.0
    for k, v in loop.model.named_buffers():
        if k.endswith('num_batches_tracked'):
            want_n = (k_hops if 'edge_encoder' in k else 1) * t
            assert int(v) == want_n == int(obuf[k]), f'{what}{k} = {int(v)}, oracle {int(obuf[k])}, expected {want_n}'
            continue
        o = obuf[k].float()
        err = helpers._close(v.detach().cpu().float(), o, rtol=1e-4, atol=1e-6, what=what + 'buffer ' + k)
        fig['buffer'] = max(fig['buffer'], err / (1e-6 + 1e-4 * float(o.abs().max())))
    return fig


def oracle_run(shape, kind, dev, replay, defer, max_norm, label):
    loop = Loop(shape, kind, dev=dev, replay=replay, defer=defer, max_norm=max_norm)
    twin = make_model(shape, dev, fill=99) if replay else None
    worst = {}
    for t in range(1, T_STEPS + 1):
        if t not in ORACLE_STEPS[shape]:
            loop.step(t)
            continue
        fig = oracle_step(loop, t, twin)
        note(f'LOOP oracle {label} step {t}: fraction of each bar ' + ', '.join(f'{k} {v:.3g}' for k, v in fig.items()))
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
    check_buckets(loop)
    note(f'LOOP oracle {label} worst over steps {ORACLE_STEPS[shape]}: ' + ', '.join(f'{k} {v:.3g}' for k, v in worst.items()))
    return worst


# (shape, loss, composed path, clip deferred, max_norm).  'alternate': the clip deferred on odd steps and in place on even ones -- a deferred
# coefficient that outlived its step would be applied a second time, on top of the in-place clip of the next one
ORACLE_GRID = [('S', 'cross_entropy', False, True, 1.0), ('S', 'margin_rank', True, False, 1.0), ('S', 'cross_entropy', False, False, 1e9),
               ('S', 'cross_entropy', False, 'alternate', 1.0), ('M', 'cross_entropy', False, True, 1.0)]


@pytest.mark.gpu
@pytest.mark.parametrize('shape,kind,composed,defer,max_norm,form', helpers.with_forms(ORACLE_GRID), indirect=['form'])
def test_each_replayed_step_matches_the_float64_oracle(shape, kind, composed, defer, max_norm, form, monkeypatch):
    hip()
    _lib.ERR_WATCH.poll(block=True)
    if composed:
        monkeypatch.setattr(ops, 'FUSED_HOP', False)
    t0 = time.time()
    oracle_run(shape, kind, 'cuda', True, defer, max_norm,
               f'{shape} {kind} {"composed" if composed else "native"} {"deferred" if defer is True else "in place" if defer is False else defer} max_norm {max_norm:g} [{form}]')
    torch.cuda.synchronize()
    _lib.ERR_WATCH.poll(block=True)
    note(f'LOOP oracle {shape} {kind} [{form}]: {time.time() - t0:.1f} s')


@pytest.mark.parametrize('kind,max_norm', [('cross_entropy', 1.0), ('margin_rank', 1e9)])
def test_oracle_harness_on_the_emulation(kind, max_norm):
    """the harness of the test above without a GPU: the eager loop at S on the emulation provider (torch's clip, RAdam's CPU loop)"""
    old = ops.set_kernels(EmuLossKernels())
    try:
        oracle_run('S', kind, 'cpu', False, True, max_norm, f'S {kind} emulation max_norm {max_norm:g}')
    finally:
        ops.set_kernels(old)


# ---- 3. evaluation in the middle of training ------------------------------------------------------------------------------------------------
def _oracle_eval_logits(shape, sd, hb):
    o = helpers.build_oracle(SHAPES[shape])
    o.load_state_dict(sd)
    o.eval()
    with torch.no_grad():
        return o(hb['sent'], hb['cids'], hb['nt'], hb['ns'], hb['al'], (hb['ei'], hb['et']))[0]


@pytest.mark.gpu
@pytest.mark.parametrize('shape,form', helpers.with_forms(['S', 'M']), indirect=['form'])
def test_evaluation_replay_in_the_middle_of_training(shape, form):
    """ONE GraphedForward for the run, captured after step 2 and replayed after step 7, when weights and running statistics have moved"""
    hip()
    _lib.ERR_WATCH.poll(block=True)
    loop = Loop(shape, 'cross_entropy')
    nc, hb = loop.nc, host_batch(shape, T_STEPS)
    eb = on(hb, 'cuda')
    fwd = inference.GraphedForward(loop.model, nc, capacity=capacity)
    fields = (eb['sent'], eb['cids'], eb['nt'], eb['ns'], eb['al'], eb['graph'])
    seen = []
    for t in range(1, T_STEPS + 1):
        loop.step(t)
        if t not in (2, T_STEPS):
            continue
        loop.model.eval()
        got = fwd(*fields, labels=eb['labels']).clone()
        with torch.no_grad(), ops.inference_path():
            want, _ = loop.model(*fields)
        assert torch.equal(got, want), f'after step {t}: replayed eval logits differ from the eager inference forward by {(got - want).abs().max().item():.3e}'
        sd = {k: v.detach().cpu().clone() for k, v in loop.model.state_dict().items()}
        ref = _oracle_eval_logits(shape, sd, hb)
        frac = helpers._close(got.cpu(), ref, what=f'{shape} eval logits after step {t}', **FWD) / (FWD['atol'] + FWD['rtol'] * float(ref.abs().max()))
        hits = int((want.view(-1, nc).argmax(1) == eb['labels']).sum())
        acc = inference.evaluate_accuracy([(None, eb['labels']) + fields], loop.model, graphed=fwd)
        assert acc == hits / eb['labels'].numel()
        seen.append(got)
        note(f'LOOP eval {shape} [{form}] after step {t}: replay == eager, {frac:.3g} of the FWD bar from the fp32 oracle, accuracy {acc:.3f}')
        loop.model.train()
    assert fwd.n_graphs == 1, 'the evaluation after step 7 was to REPLAY the capture of step 2'
    assert not torch.equal(seen[0], seen[1]), 'five training steps left the eval logits where they were'
    torch.cuda.synchronize()
    _lib.ERR_WATCH.poll(block=True)


# ---- 4. resume from a checkpoint -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('shape,form', helpers.with_forms(['S', 'M']), indirect=['form'])
def test_resume_from_a_checkpoint_after_step_4(shape, form, tmp_path):
    """both state dicts through torch.save into a model with another fill, a new RAdam and a new GraphedStep: steps 5 .. 7 (RAdam changes
    its branch at 6) equal the uninterrupted run's bit for bit"""
    hip()
    _lib.ERR_WATCH.poll(block=True)
    run = Loop(shape, 'cross_entropy')
    want = {}
    for t in range(1, T_STEPS + 1):
        out = run.step(t)
        if t == 4:
            torch.save({'model': run.model.state_dict(), 'opt': run.opt.state_dict()}, tmp_path / 'step4.pt')
        if t > 4:
            want[t] = run.snapshot(*out)
    ckpt = torch.load(tmp_path / 'step4.pt', map_location='cuda')
    res = Loop(shape, 'cross_entropy', fill=77)
    assert not torch.equal(res.model.fc.layers[0].weight, run.model.fc.layers[0].weight)
    res.model.load_state_dict(ckpt['model'])
    res.opt.load_state_dict(ckpt['opt'])
    n = 0
    for t in range(5, T_STEPS + 1):
        n = same(res.snapshot(*res.step(t)), want[t], f'{shape} resumed step {t}')
    assert {int(st['step']) for st in res.opt.state.values()} == {T_STEPS} and res.step_fn.n_graphs == len(set(res.caps)) == 2
    torch.cuda.synchronize()
    _lib.ERR_WATCH.poll(block=True)
    note(f'LOOP resume {shape} [{form}]: steps 5 .. 7 bit-identical ({n} tensors each), {res.step_fn.n_graphs} fresh captures')


# ---- 5. load_state_dict under live captures -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('shape,form', helpers.with_forms(['S', 'M']), indirect=['form'])
def test_load_state_dict_under_live_captures(shape, form):
    """A GraphedStep and a GraphedForward are captured; then every weight and buffer is replaced in place and the frozen entity table
    grows 64-fold (ops.table_amax notes max|table| per tensor version, and the three-MFMA form maps it onto the fp16 range: a stale word
    overflows).  The next training replay and the next eval replay equal an eager run, on the same capacity layout, of a fresh model
    holding that state -- bit for bit."""
    hip()
    _lib.ERR_WATCH.poll(block=True)
    nc = SHAPES[shape]['nc']
    loop = Loop(shape, 'cross_entropy')
    hb_eval = host_batch(shape, T_STEPS)
    eb = on(hb_eval, 'cuda')
    efields = (eb['sent'], eb['cids'], eb['nt'], eb['ns'], eb['al'], eb['graph'])
    fwd = inference.GraphedForward(loop.model, nc, capacity=capacity)
    loop.step(1)
    loop.model.eval()
    fwd(*efields, labels=eb['labels'])
    loop.model.train()
    # the new state
    sd = {k: v.detach().clone() for k, v in make_model(shape, 'cuda', fill=55).state_dict().items()}
    table = [k for k in sd if k.endswith('concept_emb.emb.weight')]
    assert len(table) == 1
    sd[table[0]] *= 64.0
    for k in sd:
        if k.endswith('num_batches_tracked'):
            sd[k] += 3
    old = loop.model.state_dict()
    assert all(not torch.equal(old[k], sd[k]) for k in sd), [k for k in sd if torch.equal(old[k], sd[k])][:4]
    loop.model.load_state_dict(sd)
    fresh = Loop(shape, 'cross_entropy', replay=False, fill=66)
    fresh.model.load_state_dict(sd)
    # the next training replay (same bucket as the capture: step 2's batch)
    assert capacity(host_batch(shape, 1)['E']) == capacity(host_batch(shape, 0)['E'])
    lg, ls = loop.forward_backward(loop.batch(2), 2)
    le, lse = fresh.forward_backward(fresh.batch(2), 2)
    assert torch.isfinite(le).all() and all(torch.isfinite(p.grad).all() for p in fresh.model.parameters() if p.grad is not None)
    n = same(loop.snapshot(lg, ls, ls), fresh.snapshot(le, lse, lse), f'{shape} training replay behind load_state_dict', only=('logits', 'loss', 'grad', 'buffer', 'param'))
    assert loop.step_fn.n_graphs == 1
    # the next eval replay
    loop.model.eval()
    fresh.model.eval()
    got = fwd(*efields, labels=eb['labels']).clone()
    with torch.no_grad(), ops.inference_path():
        want, _ = fresh.model(*efields)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), f'eval replay behind load_state_dict: logits differ by {(got - want).abs().max().item():.3e}'
    assert fwd.n_graphs == 1
    ref = _oracle_eval_logits(shape, {k: v.cpu() for k, v in fresh.model.state_dict().items()}, hb_eval)
    frac = helpers._close(got.cpu(), ref, what=f'{shape} eval logits behind load_state_dict', **FWD) / (FWD['atol'] + FWD['rtol'] * float(ref.abs().max()))
    torch.cuda.synchronize()
    _lib.ERR_WATCH.poll(block=True)
    note(f'LOOP load_state_dict under captures {shape} [{form}]: training replay ({n} tensors) and eval replay bit-identical to the eager run of a '
         f'fresh model, eval logits {frac:.3g} of the FWD bar from the fp32 oracle')


# ---- 6. the dropout run is reproducible --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('shape,form', helpers.with_forms(['S', 'M']), indirect=['form'])
def test_dropout_run_is_reproducible(shape, form):
    """the run scripts' dropout rates, ops.manual_seed(5) (seed epoch 0), the replayed loop twice in fresh objects: the same final bits"""
    hip()
    _lib.ERR_WATCH.poll(block=True)
    finals, all_losses = [], []
    for _ in range(2):
        loop = Loop(shape, 'cross_entropy', ps=RUN_SCRIPT_DROPOUT)
        ops.manual_seed(5)  # (behind the model's construction, which seeds torch for its own initialisation)
        run_losses = [float(loop.step(t)[1].detach()) for t in range(1, T_STEPS + 1)]
        assert all(math.isfinite(x) for x in run_losses), run_losses
        all_losses.append(run_losses)
        finals.append({k: v for k, v in loop.snapshot().items() if k.split(' ')[0] in ('param', 'buffer')})
    n = same(finals[0], finals[1], f'{shape} dropout run, final state')
    assert all_losses[0] == all_losses[1] and len(set(all_losses[0])) == T_STEPS
    undropped = Loop(shape, 'cross_entropy')
    assert float(undropped.step(1)[1].detach()) != all_losses[0][0], 'the dropout run drew no masks'
    torch.cuda.synchronize()
    _lib.ERR_WATCH.poll(block=True)
    note(f'LOOP dropout {shape} [{form}]: two runs, {n} final tensors bit-identical, losses {["%.4f" % x for x in all_losses[0]]}')


def test_a_reloaded_table_keeps_its_maximum_word_and_a_capture_refreshes_it():
    """The host logic behind test 5, without a GPU (a stub provider whose absmax is torch's): the word of a live table keeps its identity
    across versions, so the address a captured graph holds stays valid; a capture is handed the (table, word) pairs it read
    (ops.table_words); ops.refresh_table_words -- what graphed.replay runs in front of every launch -- reduces a reloaded table into that
    same word and costs no reduction when nothing moved."""
    class Stub:
        name, gemm_split, calls = 'hip', 2, 0

        def absmax(self, x):
            self.calls += 1
            return x.abs().max().reshape(1).view(torch.int32).repeat(4)

    def as_float(word):
        return word[:1].view(torch.float32).item()

    K = Stub()
    old = ops.set_kernels(K)
    try:
        raw = torch.zeros(64 * 8 + 4)
        off = (-raw.data_ptr() % 16) // 4
        table = raw[off:off + 64 * 8].view(64, 8)
        table.copy_(torch.linspace(-1.0, 0.5, 64 * 8).view(64, 8))
        assert table.data_ptr() % 16 == 0 and table.is_contiguous()
        pairs = []
        with ops.table_words(pairs):
            w = ops.table_amax(K, table)
            assert ops.table_amax(K, table) is w  # (the capture itself: a second lookup, no second entry)
        assert len(pairs) == 1 and pairs[0][0] is table and pairs[0][1] is w and as_float(w) == 1.0 and K.calls == 1
        assert ops.table_amax(K, table) is w and len(pairs) == 1  # (outside the capture nothing is recorded)
        ops.refresh_table_words(pairs)
        assert K.calls == 1, 'a table that did not move cost a reduction'
        table.copy_(table * 64.0)  # what load_state_dict does: in place, the version moves
        ops.refresh_table_words(pairs)
        assert K.calls == 2 and as_float(w) == 64.0, 'the word a capture holds was not brought up to date'
        assert ops.table_amax(K, table) is w and K.calls == 2
        table.mul_(0.5)
        assert ops.table_amax(K, table) is w and as_float(w) == 32.0 and K.calls == 3  # (the eager path writes the same word)
        ops.refresh_table_words(pairs)
        assert K.calls == 3
    finally:
        ops.set_kernels(old)
