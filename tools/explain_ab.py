"""What the detailed evaluation costs, four forms of one eval forward of the decoder in ONE process:

  plain     the inference-path forward (ops.inference_path), nothing traced, no host synchronisation per forward
  trace     explain.trace(model, ...): the same forward with an attention buffer per hop + qagnn_attn_trace_f32, one synchronisation
  edges     explain.trace(..., edges=True): additionally qagnn_attn_export_f32 and the edge list in the caller's order
  by hand   the way to the same numbers without the two kernels: the per-layer loop (every hop its own native call, its attention
            collected), the attention permuted into edge order and propagated by stock torch ops (explain.export_torch / trace_torch),
            one synchronisation

on bench.py's workload and model (CSQA-shaped: n = 200 node slots, 38 relations, 5 choices) at 10 and 320 subgraphs per batch, over a
fixed cycle of `--batches` different batches per size (blobs already on the device).  Three rounds; in a round the arms run one after
another; per arm the wall time of `--steps` calls, final synchronisation included, divided by their number.  Per arm: the rounds, their
median and their spread (max - min).  A difference is quoted only where it lies outside the larger spread of the two arms compared.

    python tools/explain_ab.py [--steps 50] [--warmup 5] [--rounds 3] [--out profiles/explain_ab.txt]
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
from qagnn_amd import data_utils, explain, ops  # noqa: E402
from qagnn_amd import modeling_qagnn as MQ  # noqa: E402

ARMS = ('plain', 'trace', 'edges', 'by hand')


def batches(wl, nq, count, n_concept, dev):
    out = []
    for i in range(count):
        b = bench.make_batch(wl, nq, 500 + i, n_concept)
        B, E, store, ids = b['blob_meta']
        out.append(dict(flat=[b[k].to(dev) for k in ('sent', 'cids', 'nt', 'ns', 'al')],
                        adj=data_utils.PackedGraphBatch(b['blobs'].to(dev), B, E, store, ids, wl['nc'])))
    return out


def by_hand(model, b, n):
    with ops.attention_capture() as cap:  # (outside the inference path: the per-layer loop)
        logits, _ = model(*b['flat'], b['adj'])
    graph, a = cap.graph, cap.a
    alpha = explain.export_torch(graph, a)
    flow, best, pred = explain.trace_torch(graph, a, graph.N // n, n)
    graph.array('err', 4).tolist()  # the synchronisation
    return logits, flow, best, pred, alpha


def measure(nq, wl, args):
    dev = torch.device('cuda', 0)
    model = bench.build_model(MQ, wl, args.n_concept, p=args.dropout).to(dev).eval()
    bs = batches(wl, nq, args.batches, args.n_concept, dev)
    n = wl['n']

    def run(arm, b):
        with torch.no_grad():
            if arm == 'plain':
                with ops.inference_path():
                    return model(*b['flat'], b['adj'])
            if arm == 'by hand':
                return by_hand(model, b, n)
            return explain.trace(model, *b['flat'], b['adj'], edges=arm == 'edges')

    for arm in ARMS:  # one walk over the cycle: lazy initialisation outside every figure
        for b in bs:
            run(arm, b)
    torch.cuda.synchronize()
    # the two kernels against the stock-torch forms on the SAME attention (that of the inference-path forward; the per-layer loop of the
    # `by hand` arm runs outside that path -- other GEMM forms from 8 192 node rows on -- so its attention differs in the last bits);
    # flow is summed in another order by index_add_: not bit for bit
    with torch.no_grad(), ops.inference_path(), ops.attention_capture() as cap:
        model(*bs[0]['flat'], bs[0]['adj'])
    K, B = ops.kernels(), cap.graph.N // n
    nat, ref = K.attn_trace(cap.graph, cap.a, B, n), explain.trace_torch(cap.graph, cap.a, B, n)
    agree = (f'on one attention: flow max |kernel - torch ops| = {(nat[0] - ref[0]).abs().max().item():.2e}, best {(nat[1] - ref[1]).abs().max().item():.2e}, '
             f'pred equal on {(nat[2] == ref[2]).float().mean().item() * 100:.2f} % of the nodes, alpha bit for bit: '
             f'{torch.equal(K.attn_export(cap.graph, cap.a), explain.export_torch(cap.graph, cap.a))}')
    ms = {a: [] for a in ARMS}
    it = {a: 0 for a in ARMS}
    for r in range(args.rounds):
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
    from qagnn_amd import _lib
    _lib.ERR_WATCH.poll(block=True)
    med = {a: statistics.median(ms[a]) for a in ARMS}
    spr = {a: max(ms[a]) - min(ms[a]) for a in ARMS}
    head = f'  {"":10s} ' + ' '.join(f'{"round " + str(r + 1):>9s}' for r in range(args.rounds)) + f' {"median":>9s} {"spread":>9s}'
    lines = [f'{nq * wl["nc"]} subgraphs per batch ({nq} questions x {wl["nc"]}, {nq * wl["nc"] * n} node rows), {len(bs)} batches of '
             f'{min(b["adj"].E for b in bs)}..{max(b["adj"].E for b in bs)} edges; {args.steps} calls per round behind {args.warmup} untimed; ms per call',
             head] + [f'  {a:10s} ' + ' '.join(f'{t:9.3f}' for t in ms[a]) + f' {med[a]:9.3f} {spr[a]:9.3f}' for a in ARMS]
    for x, y in (('trace', 'plain'), ('edges', 'trace'), ('by hand', 'trace'), ('by hand', 'edges')):
        s = max(spr[x], spr[y])
        d = med[x] - med[y]
        lines.append(f'  {x} - {y} = {d:+.3f} ms, larger spread of the two arms {s:.3f} ms: ' + ('OUTSIDE the spread' if abs(d) > s else 'inside the spread'))
    lines.append('  ' + agree)
    return lines


def kernels_alone(wl, args, nq=64, reps=100):
    """the two launches by themselves at the large size (device events): qagnn_attn_trace_f32 and qagnn_attn_export_f32 on one batch's graph"""
    dev = torch.device('cuda', 0)
    model = bench.build_model(MQ, wl, args.n_concept, p=args.dropout).to(dev).eval()
    b = batches(wl, nq, 1, args.n_concept, dev)[0]
    K = ops.kernels()
    with torch.no_grad(), ops.inference_path(), ops.attention_capture() as cap:
        model(*b['flat'], b['adj'])
    graph, a, n = cap.graph, cap.a, wl['n']
    lines = []
    for name, fn in (('qagnn_attn_trace_f32', lambda: K.attn_trace(graph, a, graph.N // n, n)), ('qagnn_attn_export_f32', lambda: K.attn_export(graph, a))):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3 / reps)
        lines.append(f'{name} alone, {graph.N // n} subgraphs x {n} node rows, k = {a.size(0)}, {graph.Ep} edge positions, {reps} calls back to back, three rounds: '
                     + ' '.join(f'{x:.1f}' for x in t) + f' us per call (the launch and the output allocation of the binding), median {statistics.median(t):.1f} us')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batches', type=int, default=4, help='different batches per size, cycled')
    ap.add_argument('--n-concept', type=int, default=100000)
    ap.add_argument('--dropout', type=float, default=0.2)
    ap.add_argument('--sizes', type=int, nargs='+', default=[2, 64], help='questions per batch (x 5 choices = subgraphs)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    wl = bench.WORKLOADS['configs[1]']
    lines = [f'eval forward of the decoder with its attention traced, bench.py model ({bench.K_LAYERS} layers, d = {bench.D}), entity table '
             f'{args.n_concept} x {wl["concept_in"]}; {len(os.sched_getaffinity(0))} CPUs, {torch.get_num_threads()} torch threads', '']
    for nq in args.sizes:
        lines += measure(nq, wl, args) + ['']
    lines += kernels_alone(wl, args)
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
