"""One optimiser step of the reference's loop with the tail behind the replayed step (a) and inside it (b) -- in ONE process.

  a  graphed.GraphedStep(model, nc) with accumulate=True per mini-batch, then optimization_utils.clip_grad_norm_(..., defer_to=opt),
     RAdam.step() and zero_grad(set_to_none=True): the sequence the package had before the captured tail, which remains in the tree
  b  graphed.GraphedStep(model, nc, optimizer=opt, max_grad_norm=...) with accumulate=True per mini-batch and update=True on the last one

at three points: 10 subgraphs with a window of 1 mini-batch, 10 subgraphs with a window of 32 (the reference's operating point: 64
questions as 32 mini-batches of 2, run_qagnn__csqa.sh:16-17) and 320 subgraphs with a window of 1 -- bench.py's CSQA workload and model,
inputs resident on the device as load-time blobs, the learning rate changed before every optimiser step as a scheduler does.
Three rounds; in a round the arms run one after another (a b), each `--steps` optimiser steps behind `--warmup` untimed ones.  A HIP event
is recorded on the launch stream behind every optimiser step and nothing synchronises inside a round (the host runs ahead as in a
training loop); a step's time is the interval between its event and the one before.  Reported: the median ms per optimiser step of each
round, and per arm the median of the rounds and their spread (max - min).  Captures are made before round 1.
The launch counts of the tail are COMPUTED from the pack arithmetic of csrc/optim.hip (for_each_pack over the model's tensor list), not
traced; torch's own launches in arm a (clone, _foreach_add_) are named, not counted.

    python tools/graphed_update_ab.py [--steps 100] [--warmup 10] [--rounds 3] [--out profiles/graphed_update_ab.txt]
"""
import argparse
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workload, the batch and the model of the timed benchmark; nothing of it is run)
from qagnn_amd import graphed  # noqa: E402
from qagnn_amd import modeling_qagnn as MQ  # noqa: E402
from qagnn_amd import optimization_utils as OU  # noqa: E402

NO_DECAY = re.compile(r'bias$|(edge_encoder|mlp)\.1\.weight$')  # biases and BatchNorm weights (the reference's no_decay list)
MAX_NORM, LR, WD = 1.0, 1e-3, 0.01


def make_opt(model):
    named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
    return OU.RAdam([dict(params=[p for k, p in named if not NO_DECAY.search(k)], weight_decay=WD),
                     dict(params=[p for k, p in named if NO_DECAY.search(k)], weight_decay=0.0)], lr=LR)


def constants():
    with open(os.path.join(ROOT, 'qagnn_amd', 'csrc', 'optim.hip')) as f:
        text = f.read()
    return {n: int(re.search(r'constexpr int %s = (\d+);' % n, text).group(1)) for n in ('MT_MAX_TENSORS', 'MT_MAX_BLOCKS', 'MT_CHUNK')}


def packs(numels, k):
    """launches of one multi-tensor call over tensors of these sizes (for_each_pack of csrc/optim.hip)"""
    nt = nb = launches = 0
    for numel in numels:
        chunks, c = -(-numel // k['MT_CHUNK']), 0
        while c < chunks:
            if nt == k['MT_MAX_TENSORS'] or nb == k['MT_MAX_BLOCKS']:
                launches += 1 if nb else 0
                nt = nb = 0
            nt += 1
            take = min(chunks - c, k['MT_MAX_BLOCKS'] - nb)
            nb, c = nb + take, c + take
    return launches + (1 if nb else 0)


def launch_counts(opt, window):
    k = constants()
    groups = [[p.numel() for p in g['params'] if p.requires_grad] for g in opt.param_groups]
    every = [n for g in groups for n in g]
    norm = packs(every, k) + 1
    a = f'{norm} norm + {sum(packs(g, k) for g in groups)} update (one call per group)'
    a += f'; torch: {len(every)} clone' + (f' + {window - 1} x _foreach_add_ over {len(every)} tensors' if window > 1 else '')
    acc = packs(every, k)
    b = f'{norm} norm + {packs(every, k)} update (one call, every group), all inside the graph; in front of the replay {-(-len(every) // 64)} record launches'
    if window > 1:
        b += f'; {acc} accumulation per mini-batch inside the graph (+ 1 fill of the first-of-window word where it changes)'
    return a, b


def arms(nq, window, n_concept, dropout):
    wl = bench.WORKLOADS['configs[1]']
    nc = wl['nc']
    dev = torch.device('cuda', 0)
    batches = [bench.to_device(bench.make_batch(wl, nq, seed=123 + i, n_concept=n_concept), dev, True, nc) for i in range(min(window, 4))]
    models = {v: bench.build_model(MQ, wl, n_concept, p=dropout).to(dev).train() for v in 'ab'}
    opts = {v: make_opt(models[v]) for v in 'ab'}
    steps = {'a': graphed.GraphedStep(models['a'], nc, loss='cross_entropy'),
             'b': graphed.GraphedStep(models['b'], nc, loss='cross_entropy', optimizer=opts['b'], max_grad_norm=MAX_NORM)}
    count = {'a': 0, 'b': 0}

    def fields(j):
        b = batches[j % len(batches)]
        return b['sent'], b['cids'], b['nt'], b['ns'], b['al'], b['adj'], b['labels'], 1.0 / window

    def set_lr(v):
        count[v] += 1
        for g in opts[v].param_groups:
            g['lr'] = LR * (1.0 + 0.001 * (count[v] % 100))

    def a():
        set_lr('a')
        for j in range(window):
            steps['a'](*fields(j), accumulate=True)
        OU.clip_grad_norm_(list(models['a'].parameters()), MAX_NORM, defer_to=opts['a'])
        opts['a'].step()
        opts['a'].zero_grad(set_to_none=True)

    def b():
        set_lr('b')
        for j in range(window):
            steps['b'](*fields(j), accumulate=True, update=(j == window - 1))

    E = sorted({int(graphed.edge_capacity(x['adj'].E)) for x in batches})
    return {'a': a, 'b': b}, steps, opts, nq * nc, E


def measure(nq, window, n_steps, args):
    run, steps, opts, B, caps = arms(nq, window, args.n_concept, args.dropout)
    ms = {v: [] for v in 'ab'}
    for v in 'ab':  # captures and lazy initialisation, outside every figure
        for _ in range(2):
            run[v]()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for v in 'ab':
            for _ in range(args.warmup):
                run[v]()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(n_steps + 1)]
            ev[0].record()
            for i in range(n_steps):
                run[v]()
                ev[i + 1].record()
            torch.cuda.synchronize()
            ms[v].append(statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(n_steps)))
    from qagnn_amd import _lib
    _lib.ERR_WATCH.poll(block=True)
    what = {'a': 'tail behind the replay', 'b': 'tail inside the graph'}
    lines = [f'{B} subgraphs ({nq} questions x 5), window of {window} mini-batch(es), capacities {caps}: median ms per OPTIMISER step (window x (forward + loss + '
             f'backward) + clip + RAdam), {n_steps} steps per round behind {args.warmup} untimed, HIP events between the steps, no synchronisation inside a round',
             f'  {"arm":27s} ' + ' '.join(f'{"round " + str(r + 1):>9s}' for r in range(args.rounds)) + f' {"median":>9s} {"spread":>9s}']
    for v in 'ab':
        x = ms[v]
        lines.append(f'  {v}  {what[v]:24s} ' + ' '.join(f'{t:9.3f}' for t in x) + f' {statistics.median(x):9.3f} {max(x) - min(x):9.3f}')
    med = {v: statistics.median(ms[v]) for v in 'ab'}
    spread = max(max(ms[v]) - min(ms[v]) for v in 'ab')
    verdict = 'outside' if abs(med['a'] - med['b']) > spread else 'INSIDE'
    lines.append(f'  a - b = {med["a"] - med["b"]:.3f} ms per optimiser step (a / b = {med["a"] / med["b"]:.3f}); largest spread between rounds {spread:.3f} ms: '
                 f'the difference lies {verdict} the spread;  captures: a {steps["a"].n_graphs}, b {steps["b"].n_graphs}')
    la, lb = launch_counts(opts['b'], window)
    lines += [f'  launches of the tail per optimiser step, a: {la}', f'  launches of the tail per optimiser step, b: {lb}']
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100, help='optimiser steps per round (a window of 32 runs a quarter of them)')
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--n-concept', type=int, default=100000)
    ap.add_argument('--dropout', type=float, default=0.2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    lines = []
    for nq, window in ((2, 1), (2, 32), (64, 1)):
        lines += measure(nq, window, args.steps if window == 1 else max(args.steps // 4, 10), args) + ['']
        print('\n'.join(lines[-7:]), flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines))


if __name__ == '__main__':
    main()
