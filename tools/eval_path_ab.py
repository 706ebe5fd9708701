"""The decoder's eval forward three ways, in ONE process:

  parent    model.eval(), torch.no_grad(): the forward as it is without the inference path (the k-hop stack keeps every hop's
            buffers and runs the exact six-MFMA products under running statistics)
  infer     the same forward inside ops.inference_path(): the forward-only stack (one set of hop buffers, the three-MFMA form from
            8 192 node rows, one pass over h1 per hop for its operand maximum)
  graphed   inference.GraphedForward: the inference forward + qagnn_choice_eval_f32 as one hipGraph launch per batch

on bench.py's workload and model (CSQA-shaped: n = 200 node slots, 38 relations, 5 choices) at 10 and 320 subgraphs per batch, over a
fixed cycle of `--batches` different batches per size (blobs already on the device: the data layer is not in the figure).  Three
rounds; in a round the arms run one after another; per arm the wall time of `--steps` forwards, final synchronisation included,
divided by their number.  Per arm: the rounds, their median and their spread (max - min), and the peak of torch's allocator above what
was allocated before the arm's first timed round.  The three arms score the same batches: their (correct, seen) counts are printed.

    python tools/eval_path_ab.py [--steps 100] [--warmup 10] [--rounds 3] [--out profiles/inference_path_ab.txt]
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
from qagnn_amd import data_utils, inference, ops  # noqa: E402
from qagnn_amd import modeling_qagnn as MQ  # noqa: E402

ARMS = ('parent', 'infer', 'graphed')


def batches(wl, nq, count, n_concept, dev):
    out = []
    for i in range(count):
        b = bench.make_batch(wl, nq, 500 + i, n_concept)
        B, E, store, ids = b['blob_meta']
        out.append(dict(flat=[b[k].to(dev) for k in ('sent', 'cids', 'nt', 'ns', 'al')], labels=b['labels'].to(dev),
                        adj=data_utils.PackedGraphBatch(b['blobs'].to(dev), B, E, store, ids, wl['nc'])))
    return out


def measure(nq, wl, args):
    nc, dev = wl['nc'], torch.device('cuda', 0)
    model = bench.build_model(MQ, wl, args.n_concept, p=args.dropout).to(dev).eval()
    K = ops.kernels()
    bs = batches(wl, nq, args.batches, args.n_concept, dev)
    fwd = inference.GraphedForward(model, nc)
    counts = {a: torch.zeros(2, dtype=torch.long, device=dev) for a in ARMS[:2]}

    def run(arm, b):
        if arm == 'graphed':
            fwd(*b['flat'], b['adj'], labels=b['labels'])
            return
        with torch.no_grad(), ops.inference_path(arm == 'infer'):
            logits, _ = model(*b['flat'], b['adj'])
        K.choice_eval(logits.view(-1, nc), b['labels'], counts[arm])

    for arm in ARMS:  # one walk over the cycle: lazy initialisation and every capture, outside every figure
        for b in bs:
            run(arm, b)
    torch.cuda.synchronize()
    captured = fwd.n_graphs
    fwd.reset_counts()
    for c in counts.values():
        c.zero_()
    ms, peak = {a: [] for a in ARMS}, {}
    it = {a: 0 for a in ARMS}  # (every arm walks the same sequence of batches)
    for r in range(args.rounds):
        for arm in ARMS:
            for _ in range(args.warmup):
                run(arm, bs[it[arm] % len(bs)])
                it[arm] += 1
            torch.cuda.synchronize()
            if r == 0:
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run(arm, bs[it[arm] % len(bs)])
                it[arm] += 1
            torch.cuda.synchronize()
            ms[arm].append((time.perf_counter() - t0) * 1e3 / args.steps)
            if r == 0:
                peak[arm] = torch.cuda.max_memory_allocated() - base
    from qagnn_amd import _lib
    _lib.ERR_WATCH.poll(block=True)
    head = f'  {"":10s} ' + ' '.join(f'{"round " + str(r + 1):>9s}' for r in range(args.rounds)) + f' {"median":>9s} {"spread":>9s} {"peak MiB":>10s}'
    row = lambda a: (f'  {a:10s} ' + ' '.join(f'{t:9.3f}' for t in ms[a]) +  # noqa: E731
                     f' {statistics.median(ms[a]):9.3f} {max(ms[a]) - min(ms[a]):9.3f} {peak[a] / 2 ** 20:10.1f}')
    med = {a: statistics.median(ms[a]) for a in ARMS}
    spread = max(max(ms[a]) - min(ms[a]) for a in ARMS)
    got = {a: tuple(counts[a].tolist()) for a in ARMS[:2]}
    got['graphed'] = fwd.counts()
    lines = [f'{nq * nc} subgraphs per batch ({nq} questions x {nc}, {nq * nc * wl["n"]} node rows), {len(bs)} batches of '
             f'{min(b["adj"].E for b in bs)}..{max(b["adj"].E for b in bs)} edges; {args.steps} forwards per round behind {args.warmup} untimed; ms per forward',
             head] + [row(a) for a in ARMS]
    lines.append(f'  parent - infer = {med["parent"] - med["infer"]:.3f} ms, parent - graphed = {med["parent"] - med["graphed"]:.3f} ms, '
                 f'infer - graphed = {med["infer"] - med["graphed"]:.3f} ms (largest spread between rounds: {spread:.3f} ms)')
    lines.append('  (correct, seen): ' + ', '.join(f'{a} {got[a]}' for a in ARMS) + f'; captures before / after the rounds: {captured} / {fwd.n_graphs}')
    return lines


def pass_cost(rows=64000, cols=208, reps=200):
    """the one launch pair the inference stack adds per hop where it runs the form: qagnn_bn_relu_absmax_f32 over h1 (device events)"""
    K = ops.kernels()
    g = torch.Generator().manual_seed(1)
    H = torch.randn(rows, cols, generator=g).cuda()
    sc, sh = torch.randn(cols, generator=g).cuda(), torch.randn(cols, generator=g).cuda()
    word = torch.zeros(4, dtype=torch.int32, device='cuda')
    for _ in range(10):
        K.bn_relu_absmax(H, sc, sh, out=word)
    torch.cuda.synchronize()
    t = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            K.bn_relu_absmax(H, sc, sh, out=word)
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3 / reps)
    med = statistics.median(t)
    return [f'qagnn_bn_relu_absmax_f32 alone, {rows} x {cols} ({rows * cols * 4 / 1e6:.1f} MB read), {reps} calls back to back, three rounds: '
            + ' '.join(f'{x:.1f}' for x in t) + f' us per call (both launches and the scratch allocation of the binding), median {med:.1f} us = '
            f'{rows * cols * 4 / med / 1e3:.0f} GB/s']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batches', type=int, default=4, help='different batches per size, cycled')
    ap.add_argument('--n-concept', type=int, default=100000)
    ap.add_argument('--dropout', type=float, default=0.2)
    ap.add_argument('--sizes', type=int, nargs='+', default=[2, 64], help='questions per batch (x 5 choices = subgraphs)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    wl = bench.WORKLOADS['configs[1]']
    lines = [f'eval forward of the decoder, bench.py model ({bench.K_LAYERS} layers, d = {bench.D}), entity table {args.n_concept} x {wl["concept_in"]}; '
             f'{len(os.sched_getaffinity(0))} CPUs, {torch.get_num_threads()} torch threads', '']
    for nq in args.sizes:
        lines += measure(nq, wl, args) + ['']
    lines += pass_cost()
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
