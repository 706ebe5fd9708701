"""What feeds the decoder's training step: batches assembled on the host from load-time blobs against batches named by sample ids into a
device-resident store -- in ONE process.

  blobs   MultiGPUSparseAdjDataBatchGenerator(graph_blobs=...): GraphBlobStore.pack(pin=True) + one copy of the packed buffer, the four
          node tensors indexed on the host and copied one by one                                        (the parent commit's path)
  store   MultiGPUSparseAdjDataBatchGenerator(device_store=...): DeviceGraphStore.batch() -- B int32 words -- and qagnn_store_gather
          (in front of GraphedStep with gather_fields=False: the captured graph gathers for itself, the generator only names the batch)

on a synthetic CSQA-shaped dataset (bench.py's workload and model: n = 200 node slots, 38 relations, 5 choices) at 10 and 320 subgraphs
per batch.  Two figures, three rounds each; in a round the variants run one after another:

  (a) HOST milliseconds per batch spent inside the generator (perf_counter around next(); nothing else runs, one synchronisation behind
      the round): per round the median over `--steps` batches.
  (b) milliseconds per training step with the generator INSIDE the loop, eager and graphed.GraphedStep, on both paths: per round the wall
      time of `--steps` steps, final synchronisation included, divided by their number.

Per variant: the rounds, their median and their spread (max - min).  The batches are the same fixed sequence on both paths (one fixed order
of the questions, cycled), and every variant walks the sequence once before round 1, so that every capacity bucket is captured outside
the figures; `n_graphs` is printed before and after to show nothing re-captures.

    python tools/store_batch_ab.py [--questions 320] [--steps 100] [--warmup 10] [--rounds 3] [--out profiles/device_store_ab.txt]
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
from qagnn_amd import data_utils, graphed, synthetic  # noqa: E402
from qagnn_amd import modeling_qagnn as MQ  # noqa: E402

PATHS = ('blobs', 'store')
HOST_PATHS = PATHS + ('store, ids only',)


def dataset(wl, questions, n_concept):
    nc, n = wl['nc'], wl['n']
    recs = synthetic.make_records(questions * nc, seed=123, shape=wl['shape'], n_rel=wl['n_rel'], n_concept_vocab=n_concept)
    _, cids, nt, ns, al, ei, et, _ = data_utils.records_to_tensors(recs, n, nc)
    store = data_utils.GraphBlobStore.build(ei, et, nt, wl['n_etype'], bench.N_NTYPE)
    g = torch.Generator().manual_seed(124)
    nested = [x.view(questions, nc, *x.shape[1:]) for x in (cids, nt, ns, al)]
    return dict(store=store, nested=nested, sent=torch.randn(questions, nc, wl['sent_dim'], generator=g),
                labels=torch.randint(0, nc, (questions,), generator=g), order=torch.randperm(questions, generator=g))


def loaders(ds, dstore, nq, nc, dev):
    """path -> an endless iterator over the generator's batches (the fixed question order, cycled), flattened for QAGNN.forward"""
    qids = list(range(ds['labels'].numel()))

    def stream(**kw):
        gen = data_utils.MultiGPUSparseAdjDataBatchGenerator(None, 'eval', dev, dev, nq, ds['order'], qids, ds['labels'], tensors0=[ds['sent']],
                                                             tensors1=ds['nested'], num_choice=nc, **kw)
        while True:
            for _, labels, sent, cids, nt, ns, al, adj, _ in gen:
                flat = [x if x is None else x.reshape(-1, *x.shape[2:]) for x in (sent, cids, nt, ns, al)]
                yield flat, adj, labels

    return {'blobs': stream(graph_blobs=ds['store']), 'store': stream(device_store=dstore),
            'store, ids only': stream(device_store=dstore, gather_fields=False)}, -(-len(qids) // nq)


def measure(nq, ds, dstore, wl, args):
    nc, dev = wl['nc'], torch.device('cuda', 0)
    variants = [(mode, path) for mode in ('eager', 'graphed') for path in PATHS]
    models = {v: bench.build_model(MQ, wl, args.n_concept, p=args.dropout).to(dev).train() for v in variants}
    steps = {v: graphed.GraphedStep(models[v], nc) for v in variants if v[0] == 'graphed'}

    def step(v, flat, adj, labels):
        if v[0] == 'graphed':
            steps[v](*flat, adj, labels)
            return
        for p in models[v].parameters():
            p.grad = None
        logits, _ = models[v](*flat, adj)
        torch.nn.functional.cross_entropy(logits.view(-1, nc), labels).backward()

    # ---- (a) the generator alone
    host = {p: [] for p in HOST_PATHS}
    its, per_epoch = loaders(ds, dstore, nq, nc, dev)
    for p in HOST_PATHS:
        for _ in range(args.warmup):
            next(its[p])
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for p in HOST_PATHS:
            t = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                batch = next(its[p])
                t.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            del batch
            host[p].append(statistics.median(t))
    # ---- (b) the training step with the generator in the loop
    its = {v: loaders(ds, dstore, nq, nc, dev)[0]['store, ids only' if v == ('graphed', 'store') else v[1]] for v in variants}
    for v in variants:  # one walk over the whole sequence: lazy initialisation and every capacity bucket's capture, outside every figure
        for _ in range(per_epoch + 3):
            step(v, *next(its[v]))
    torch.cuda.synchronize()
    captured = {v: s.n_graphs for v, s in steps.items()}
    ms = {v: [] for v in variants}
    for _ in range(args.rounds):
        for v in variants:
            for _ in range(args.warmup):
                step(v, *next(its[v]))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(v, *next(its[v]))
            torch.cuda.synchronize()
            ms[v].append((time.perf_counter() - t0) * 1e3 / args.steps)
    from qagnn_amd import _lib
    _lib.ERR_WATCH.poll(block=True)
    E = ds['store'].edge_count.reshape(-1, nc).sum(1)[ds['order'].numpy()]
    Eb = [int(E[a:a + nq].sum()) for a in range(0, E.size, nq)]
    row = lambda name, x: f'  {name:28s} ' + ' '.join(f'{t:9.3f}' for t in x) + f' {statistics.median(x):9.3f} {max(x) - min(x):9.3f}'  # noqa: E731
    head = f'  {"":28s} ' + ' '.join(f'{"round " + str(r + 1):>9s}' for r in range(args.rounds)) + f' {"median":>9s} {"spread":>9s}'
    lines = [f'{nq * nc} subgraphs per batch ({nq} questions x {nc}), {per_epoch} batches of {min(Eb)}..{max(Eb)} edges, '
             f'{len(set(graphed.edge_capacity(e) for e in Eb))} capacity buckets; {args.steps} batches per round behind {args.warmup} untimed',
             '(a) host ms per batch inside the generator (median over the round\'s batches)', head]
    lines += [row(p, host[p]) for p in HOST_PATHS]
    med = {p: statistics.median(host[p]) for p in HOST_PATHS}
    spread = max(max(host[p]) - min(host[p]) for p in HOST_PATHS)
    lines.append(f'  blobs - store = {med["blobs"] - med["store"]:.3f} ms, blobs - store, ids only = {med["blobs"] - med["store, ids only"]:.3f} ms '
                 f'(largest spread between rounds: {spread:.3f} ms)')
    lines += ['(b) ms per training step, generator in the loop (wall time of the round / steps)', head]
    lines += [row(f'{v[0]}, {v[1]}', ms[v]) for v in variants]
    for mode in ('eager', 'graphed'):
        m = {p: statistics.median(ms[(mode, p)]) for p in PATHS}
        spread = max(max(ms[(mode, p)]) - min(ms[(mode, p)]) for p in PATHS)
        lines.append(f'  {mode}: blobs - store = {m["blobs"] - m["store"]:.3f} ms (largest spread between rounds: {spread:.3f} ms)')
    lines.append('  captures before / after the rounds: ' + ', '.join(f'{v[1]} {captured[v]} / {s.n_graphs}' for v, s in steps.items()))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--questions', type=int, default=320, help='questions of the synthetic dataset (x 5 choices = samples)')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--n-concept', type=int, default=100000)
    ap.add_argument('--dropout', type=float, default=0.2)
    ap.add_argument('--sizes', type=int, nargs='+', default=[2, 64], help='questions per batch (x 5 choices = subgraphs)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    wl = bench.WORKLOADS['configs[1]']
    ds = dataset(wl, args.questions, args.n_concept)
    t0 = time.perf_counter()
    dstore = data_utils.DeviceGraphStore.from_host(ds['store'], *ds['nested'], torch.device('cuda', 0))
    torch.cuda.synchronize()
    lines = [f'dataset: {len(dstore)} samples, n = {dstore.n}, {int(ds["store"].edge_count.min())}..{int(ds["store"].edge_count.max())} edges per sample; '
             f'device store {dstore.nbytes / 2 ** 20:.1f} MiB, uploaded once in {(time.perf_counter() - t0) * 1e3:.0f} ms; '
             f'{len(os.sched_getaffinity(0))} CPUs, {torch.get_num_threads()} torch threads', '']
    for nq in args.sizes:
        lines += measure(nq, ds, dstore, wl, args) + ['']
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
