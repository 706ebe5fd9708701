"""The decoder's training step on int64 edge lists, eager against replayed, and the replay on load-time blobs -- in ONE process.

  a  eager step, graph as (edge_index [2, E], edge_type [E]) on the device         qagnn_graph_prep_blocked, ~450 launches from Python
  b  graphed.GraphedStep, the same pair                                             qagnn_graph_prep_cap inside one hipGraph launch
  c  graphed.GraphedStep, the same graph as a PackedGraphBatch of load-time blobs   qagnn_graph_from_blobs inside one hipGraph launch

at 10 and 320 subgraphs (nq = 2 and 64 questions x 5 choices, n = 200 node slots: bench.py's CSQA workload and model, inputs resident on
the device).  Three rounds; in a round the variants run one after another (a b c), each `--steps` steps behind `--warmup` untimed ones.
A HIP event is recorded on the launch stream behind every step and nothing synchronises inside a round's steps (the host runs ahead as
in a training loop); a step's time is the interval between its event and the one before.  Reported: the median ms per step of each
round, and per variant the median of the rounds and their spread (max - min).
The captures of b and c are made once, before round 1 (their cost is not in any figure); `n_graphs` is printed to show nothing re-captures.

    python tools/graphed_edge_lists_ab.py [--steps 200] [--warmup 20] [--rounds 3] [--out profiles/graphed_edge_lists_ab.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workload, the batch and the model of the timed benchmark; nothing of it is run)
from qagnn_amd import graphed  # noqa: E402
from qagnn_amd import modeling_qagnn as MQ  # noqa: E402


def variants(nq, n_concept, dropout):
    wl = bench.WORKLOADS['configs[1]']
    nc = wl['nc']
    host = bench.make_batch(wl, nq, seed=123, n_concept=n_concept)
    dev = torch.device('cuda', 0)
    bl, be = bench.to_device(host, dev, True, nc), bench.to_device(host, dev, False, nc)
    models = {v: bench.build_model(MQ, wl, n_concept, p=dropout).to(dev).train() for v in 'abc'}
    steps = {v: graphed.GraphedStep(models[v], nc) for v in 'bc'}

    def eager():
        m = models['a']
        for p in m.parameters():
            p.grad = None
        logits, _ = m(be['sent'], be['cids'], be['nt'], be['ns'], be['al'], be['adj'])
        torch.nn.functional.cross_entropy(logits.view(-1, nc), be['labels']).backward()

    run = {'a': eager,
           'b': lambda: steps['b'](be['sent'], be['cids'], be['nt'], be['ns'], be['al'], be['adj'], be['labels']),
           'c': lambda: steps['c'](bl['sent'], bl['cids'], bl['nt'], bl['ns'], bl['al'], bl['adj'], bl['labels'])}
    E = int(be['ei'].size(1))
    return run, steps, nq * nc, E


def measure(nq, args):
    run, steps, B, E = variants(nq, args.n_concept, args.dropout)
    ms = {v: [] for v in 'abc'}
    for v in 'abc':  # captures and lazy initialisation, outside every figure
        for _ in range(3):
            run[v]()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for v in 'abc':
            for _ in range(args.warmup):
                run[v]()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
            ev[0].record()
            for i in range(args.steps):
                run[v]()
                ev[i + 1].record()
            torch.cuda.synchronize()
            ms[v].append(statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps)))
    from qagnn_amd import _lib
    _lib.ERR_WATCH.poll(block=True)
    what = {'a': 'eager, edge lists', 'b': 'replay, edge lists', 'c': 'replay, blobs'}
    lines = [f'{B} subgraphs ({nq} questions x 5), E = {E} edges, capacity {graphed.edge_capacity(E)}: median ms per step (forward + loss + backward), '
             f'{args.steps} steps per round behind {args.warmup} untimed, HIP events between the steps, no synchronisation inside a round',
             f'  {"variant":22s} ' + ' '.join(f'{"round " + str(r + 1):>9s}' for r in range(args.rounds)) + f' {"median":>9s} {"spread":>9s}']
    for v in 'abc':
        x = ms[v]
        lines.append(f'  {v}  {what[v]:19s} ' + ' '.join(f'{t:9.3f}' for t in x) + f' {statistics.median(x):9.3f} {max(x) - min(x):9.3f}')
    med = {v: statistics.median(ms[v]) for v in 'abc'}
    spread = max(max(ms[v]) - min(ms[v]) for v in 'ab')
    lines.append(f'  a - b = {med["a"] - med["b"]:.3f} ms (largest spread between rounds of a, b: {spread:.3f} ms);  b - c = {med["b"] - med["c"]:.3f} ms '
                 f'(b / c = {med["b"] / med["c"]:.3f});  captures: b {steps["b"].n_graphs}, c {steps["c"].n_graphs}')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--n-concept', type=int, default=100000)
    ap.add_argument('--dropout', type=float, default=0.2)
    ap.add_argument('--sizes', type=int, nargs='+', default=[2, 64], help='questions per batch (x 5 choices = subgraphs)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    lines = []
    for nq in args.sizes:
        lines += measure(nq, args) + ['']
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
