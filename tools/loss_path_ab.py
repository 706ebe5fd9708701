"""The decoder's training step with the loss two ways, in ONE process:

  torch     loss = F.cross_entropy(logits.view(-1, nc), labels) * weight -- what GraphedStep(loss=None), bench.py and every tool compute
  native    loss = ops.choice_loss(..., weight word, meter): qagnn_choice_loss_f32, one launch forward and one backward
            ('cross_entropy', and 'margin_rank', which has no replayed "torch" arm: its pairs need boolean-mask indexing)

each as the eager step and as the replayed step (graphed.GraphedStep), on bench.py's workload and model (CSQA-shaped: n = 200 node
slots, 38 relations, 5 choices) at 10 and 320 subgraphs per batch, over a fixed cycle of `--batches` different batches per size (blobs
already on the device).  Three rounds; in a round the arms run one after another; per arm the wall time of `--steps` steps, final
synchronisation included, divided by their number; the rounds, their median and their spread (max - min).

Then the reference's optimiser window (qagnn.py:252-266: 32 mini-batches of 2 questions, gradients accumulated): replayed steps with
`total_loss += loss.item()` behind every mini-batch against replayed native steps and ONE `step.meter.read()` per window.

The launch counts of the two routes are counted on the host: the ATen operators that the loss and its backward dispatch on a detached
logits leaf (operators that only make views are left out; each of the others is one launch), against the two launches of the native route.

    python tools/loss_path_ab.py [--steps 100] [--warmup 10] [--rounds 3] [--out profiles/loss_path_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workload and the model of the timed benchmark; nothing of it is run)
from qagnn_amd import _lib, data_utils, graphed, ops  # noqa: E402
from qagnn_amd import modeling_qagnn as MQ  # noqa: E402

ARMS = ('eager torch CE', 'eager native CE', 'eager native MR', 'replay torch CE', 'replay native CE', 'replay native MR')
VIEW_OPS = ('view', 'expand', 'detach', 'alias', 'reshape', 'unsqueeze', 'squeeze', 'as_strided', 't.', 'transpose', 'permute', 'select', 'slice',
            '_unsafe_view', 'empty', 'is_same_size', 'stride', 'size', 'lift_fresh')


def batches(wl, nq, count, n_concept, dev):
    out = []
    for i in range(count):
        b = bench.make_batch(wl, nq, 500 + i, n_concept)
        B, E, store, ids = b['blob_meta']
        out.append(dict(flat=[b[k].to(dev) for k in ('sent', 'cids', 'nt', 'ns', 'al')], labels=b['labels'].to(dev),
                        adj=data_utils.PackedGraphBatch(b['blobs'].to(dev), B, E, store, ids, wl['nc'])))
    return out


def launch_counts(nq, nc, dev):
    """{route: [operator names]} of the loss and its backward on a detached logits leaf"""
    from torch.utils._python_dispatch import TorchDispatchMode

    class Count(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = str(func).replace('aten.', '')
            on_device = any(isinstance(t, torch.Tensor) and t.is_cuda for t in list(args) + list((kwargs or {}).values()))
            if on_device and not any(name.startswith(v) for v in VIEW_OPS):  # (host-only operators: the flag words' bookkeeping in pinned memory)
                self.names.append(name)
            return func(*args, **(kwargs or {}))

    g = torch.Generator().manual_seed(0)
    x = torch.randn(nq, nc, generator=g).to(dev)
    labels = torch.randint(0, nc, (nq,), generator=g).to(dev)
    lw = torch.full((), 0.5, device=dev)
    out = {}
    for route, fn in (('torch CE', lambda t: torch.nn.functional.cross_entropy(t, labels) * lw),
                      ('native CE', lambda t: ops.choice_loss(t, labels, 'cross_entropy', 0.1, lw)),
                      ('native MR', lambda t: ops.choice_loss(t, labels, 'margin_rank', 0.1, lw))):
        leaf = x.clone().requires_grad_(True)
        fn(leaf).backward()  # (lazy initialisation outside the count)
        leaf = x.clone().requires_grad_(True)
        with Count() as c:
            fn(leaf).backward()
        out[route] = c.names
    torch.cuda.synchronize()
    return out


def measure(nq, wl, args, model):
    nc, dev = wl['nc'], torch.device('cuda', 0)
    bs = batches(wl, nq, args.batches, args.n_concept, dev)
    steps = {'torch CE': graphed.GraphedStep(model, nc), 'native CE': graphed.GraphedStep(model, nc, loss='cross_entropy'),
             'native MR': graphed.GraphedStep(model, nc, loss='margin_rank')}
    lw = 0.5

    def run(arm, b):
        how, route = arm.split(' ', 1)
        if how == 'replay':
            steps[route](*b['flat'], b['adj'], b['labels'], lw)
            return
        for p in model.parameters():
            p.grad = None
        logits, _ = model(*b['flat'], b['adj'])
        if route == 'torch CE':
            loss = torch.nn.functional.cross_entropy(logits.view(-1, nc), b['labels']) * lw
        else:
            loss = ops.choice_loss(logits.view(-1, nc), b['labels'], 'cross_entropy' if route == 'native CE' else 'margin_rank', 0.1, lw)
        loss.backward()

    for arm in ARMS:  # one walk over the cycle: lazy initialisation and every capture, outside every figure
        for b in bs:
            run(arm, b)
    torch.cuda.synchronize()
    ms = {a: [] for a in ARMS}
    it = {a: 0 for a in ARMS}
    for _ in range(args.rounds):
        for arm in ARMS:
            for _ in range(args.warmup):
                run(arm, bs[it[arm] % len(bs)])
                it[arm] += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run(arm, bs[it[arm] % len(bs)])
                it[arm] += 1
            torch.cuda.synchronize()
            ms[arm].append((time.perf_counter() - t0) * 1e3 / args.steps)
    _lib.ERR_WATCH.poll(block=True)
    med = {a: statistics.median(ms[a]) for a in ARMS}
    spr = {a: max(ms[a]) - min(ms[a]) for a in ARMS}
    head = f'  {"":18s} ' + ' '.join(f'{"round " + str(r + 1):>9s}' for r in range(args.rounds)) + f' {"median":>9s} {"spread":>9s}'
    lines = [f'{nq * nc} subgraphs per batch ({nq} questions x {nc}), {len(bs)} batches of {min(b["adj"].E for b in bs)}..{max(b["adj"].E for b in bs)} '
             f'edges; {args.steps} steps per round behind {args.warmup} untimed; ms per step', head]
    lines += [f'  {a:18s} ' + ' '.join(f'{t:9.3f}' for t in ms[a]) + f' {med[a]:9.3f} {spr[a]:9.3f}' for a in ARMS]
    for how in ('eager', 'replay'):
        a, b = f'{how} torch CE', f'{how} native CE'
        d, s = med[a] - med[b], max(spr[a], spr[b])
        lines.append(f'  {how}: torch CE - native CE = {d:+.3f} ms, larger spread of the two arms {s:.3f} ms: {"OUTSIDE" if abs(d) > s else "inside"} the spread')
    lines.append(f'  margin-rank (no replayed torch arm exists): replay {med["replay native MR"]:.3f} ms per step beside cross-entropy {med["replay native CE"]:.3f} ms')
    return lines, steps, bs


def window(wl, args, steps, bs):
    """32 mini-batches of 2 questions with accumulated gradients: .item() per mini-batch against one meter.read() per window, and two
    controls that separate the loss route from the host running ahead: the native step with .item() per mini-batch, the torch step with
    no logging at all.  Beside the times: the longest queue of validation-flag copies (_lib.ERR_WATCH.pending) a replay found waiting."""
    n_mb, lw = 32, 2 / 64
    torch_step, native = steps['torch CE'], steps['native CE']
    for p in native.model.parameters():  # (a window starts from no gradient, as after optimizer.zero_grad(set_to_none=True))
        p.grad = None
    arms = {'torch + item': (torch_step, True, 'replay torch CE + loss.item() x 32', n_mb),
            'native + item': (native, True, 'replay native CE + loss.item() x 32', n_mb),
            'torch, no log': (torch_step, False, 'replay torch CE, loss never read', 0),
            'native + meter': (native, False, 'replay native CE + meter.read() x 1', 1)}
    queue = {a: 0 for a in arms}

    def run(arm):
        step, item = arms[arm][:2]
        total = 0.0
        if arm == 'native + meter':
            native.meter.reset()
        for i in range(n_mb):
            b = bs[i % len(bs)]
            _, loss = step(*b['flat'], b['adj'], b['labels'], lw, accumulate=True)
            queue[arm] = max(queue[arm], len(_lib.ERR_WATCH.pending))
            if item:
                total += loss.item()
        return native.meter.read()[0] if arm == 'native + meter' else total

    totals = {a: run(a) for a in arms}
    torch.cuda.synchronize()
    ms = {a: [] for a in arms}
    for _ in range(args.rounds):
        for arm in arms:
            run(arm)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.windows):
                run(arm)
            torch.cuda.synchronize()
            ms[arm].append((time.perf_counter() - t0) * 1e3 / args.windows)
    med = {a: statistics.median(ms[a]) for a in arms}
    spr = {a: max(ms[a]) - min(ms[a]) for a in arms}
    lines = [f'one optimiser window of the reference: {n_mb} mini-batches of 2 questions (10 subgraphs), gradients accumulated, no optimiser step; '
             f'{args.windows} windows per round behind 1 untimed; ms per window',
             f'  {"":38s} ' + ' '.join(f'{"round " + str(r + 1):>9s}' for r in range(args.rounds)) + f' {"median":>9s} {"spread":>9s}   host waits   longest flag queue']
    lines += [f'  {arms[a][2]:38s} ' + ' '.join(f'{t:9.3f}' for t in ms[a]) + f' {med[a]:9.3f} {spr[a]:9.3f}   {arms[a][3]:10d}   {queue[a]:18d}' for a in arms]
    for x, y in (('torch + item', 'native + meter'), ('torch + item', 'native + item'), ('torch, no log', 'native + meter')):
        d, sp = med[x] - med[y], max(spr[x], spr[y])
        lines.append(f'  ({x}) - ({y}) = {d:+.3f} ms per window ({d / n_mb:+.4f} ms per mini-batch), larger spread of the two {sp:.3f} ms: '
                     f'{"OUTSIDE" if abs(d) > sp else "inside"} the spread')
    lines.append('  window losses (dropout on: every replay draws its own masks, the arms do not see the same numbers): '
                 + ', '.join(f'{a} {totals[a]:.6f}' for a in arms if a != 'torch, no log'))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--windows', type=int, default=10)
    ap.add_argument('--batches', type=int, default=4, help='different batches per size, cycled')
    ap.add_argument('--n-concept', type=int, default=100000)
    ap.add_argument('--dropout', type=float, default=0.2)
    ap.add_argument('--sizes', type=int, nargs='+', default=[2, 64], help='questions per batch (x 5 choices = subgraphs)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    wl = bench.WORKLOADS['configs[1]']
    dev = torch.device('cuda', 0)
    model = bench.build_model(MQ, wl, args.n_concept, p=args.dropout).to(dev).train()
    lines = [f'training step of the decoder, bench.py model ({bench.K_LAYERS} layers, d = {bench.D}), entity table {args.n_concept} x {wl["concept_in"]}; '
             f'{len(os.sched_getaffinity(0))} CPUs, {torch.get_num_threads()} torch threads', '']
    counts = launch_counts(2, wl['nc'], dev)
    lines.append('launches of the loss and its backward on a detached logits leaf, eager (library launches + ATen operators dispatched, view-only operators left out;')
    lines.append('copy_ on the native routes is the asynchronous copy of the label flag word to pinned memory, which a replay makes once per replay, not per loss):')
    for route, names in counts.items():
        own = 2 if route.startswith('native') else 0
        lines.append(f'  {route:10s} {own} + {len(names):2d} = {own + len(names):2d}: {", ".join(names) if names else "-"}')
    lines.append('')
    small = None
    for nq in args.sizes:
        got, steps, bs = measure(nq, wl, args, model)
        lines += got + ['']
        if nq == 2:
            small = (steps, bs)
    if small is not None:
        lines += window(wl, args, *small)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
