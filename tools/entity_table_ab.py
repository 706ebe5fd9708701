"""The decoder's training step with a TRAINABLE entity table two ways, in ONE process:

  stock   ops.TRAINABLE_TABLE_FUSED = False: nn.Embedding, the materialised [B, n - 1, in] matrix, rocBLAS, torch's embedding backward
  fused   ops.TRAINABLE_TABLE_FUSED = True:  the gather-GEMM input stage and the row-grouped table gradient (include/qagnn_hip_rows.h)

on bench.py's CSQA-shaped workload and model at 10 and 320 subgraphs per batch, with a MedQA-sized table (9 958 x 768) and the CSQA
table (799 273 x 1024).  Per (table, batch size): the eager step and the replayed step (graphed.GraphedStep, native cross-entropy), the
input stage's forward + backward alone and its backward alone (HIP events), the allocator peak of the eager step; then the pieces whose
cost is the reference's semantics or the capacity, not this change: zeroing and scattering the dense gradient, RAdam over the table,
the projection over the capacity against the projection over the U live rows.  Three rounds; in a round the arms run one after another;
the rounds, their median and their spread (max - min).  A difference is called OUTSIDE only where it exceeds the larger spread.

    python tools/entity_table_ab.py [--steps 30] [--warmup 5] [--rounds 3] [--out profiles/entity_table_ab.txt]
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
from qagnn_amd import optimization_utils as OU  # noqa: E402

TABLES = {'MedQA-sized 9958 x 768': (9958, 768), 'CSQA 799273 x 1024': (799273, 1024)}


def table_line(name, ts):
    return f'  {name:34s} ' + ' '.join(f'{t:9.3f}' for t in ts) + f' {statistics.median(ts):9.3f} {max(ts) - min(ts):9.3f}'


def verdict(what, a, b):
    d, s = statistics.median(a) - statistics.median(b), max(max(a) - min(a), max(b) - min(b))
    return f'  {what} = {d:+.3f} ms, larger spread of the two arms {s:.3f} ms: {"OUTSIDE" if abs(d) > s else "inside"} the spread'


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def event_timed(setup, fn, steps, warmup):
    """ms per call of fn(state) alone on the device: setup() runs untimed in front of every call"""
    total = 0.0
    for i in range(warmup + steps):
        state = setup()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(state)
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            total += e0.elapsed_time(e1)
    return total / steps


def input_stage(model, b, fused):
    """the input stage of QAGNN.forward alone -> its output (graph attached)"""
    ce, dev = model.concept_emb, b['flat'][0].device
    sent, cids, nt, ns, al = b['flat']
    n = nt.size(1)
    if fused:
        _, _, ridx = ops.kernels().node_prep(ns.contiguous(), al.contiguous(), nt.contiguous(), cids.contiguous(), table_rows=ce.emb.weight.size(0))
        L = MQ.head_layout(model.concept_dim, dev)
        W, bias = ce.cpt_transform.weight, ce.cpt_transform.bias
        return ops.concept_input(ce.emb.weight, ridx, L.pad(W.t()), L.pad(bias), L.pad(model.svec2nvec(sent)), n, model.dropout_e.p, True,
                                 Wc=L.pad(W.t()).t().contiguous())
    g0 = model.activation(model.svec2nvec(sent)).unsqueeze(1)
    return model.dropout_e(torch.cat([g0, ce(cids[:, 1:] - 1, None)], dim=1))


def measure(label, rows, width, nq, args, dev):
    wl = dict(bench.WORKLOADS['configs[1]'], concept_in=width, sent_dim=width)
    nc = wl['nc']
    model = bench.build_model(MQ, wl, rows, p=args.dropout).to(dev).train()
    bench.fill_table(model, rows)
    table = model.concept_emb.emb.weight.requires_grad_(True)
    bs = []
    for i in range(args.batches):
        hb = bench.make_batch(wl, nq, 700 + i, rows)
        B, E, store, ids = hb['blob_meta']
        bs.append(dict(flat=[hb[k].to(dev) for k in ('sent', 'cids', 'nt', 'ns', 'al')], labels=hb['labels'].to(dev),
                       adj=data_utils.PackedGraphBatch(hb['blobs'].to(dev), B, E, store, ids, nc)))
    ids_all = torch.cat([b['flat'][1][:, 1:].reshape(-1) for b in bs])
    N = bs[0]['flat'][1].numel()
    share = 1.0 - sum(b['flat'][1][:, 1:].unique().numel() for b in bs) / ids_all.numel()
    lines = [f'{label}, {nq * nc} subgraphs per batch ({nq} questions x {nc}, {N} node rows), {len(bs)} batches; {share:.2f} of the non-context positions '
             f'repeat an id of their batch; {args.steps} steps per round behind {args.warmup} untimed; ms per step']
    lines.append(f'  {"":34s} ' + ' '.join(f'{"round " + str(r + 1):>9s}' for r in range(args.rounds)) + f' {"median":>9s} {"spread":>9s}')
    steps = {}
    it = [0]

    def eager():
        b = bs[it[0] % len(bs)]
        it[0] += 1
        for p in model.parameters():
            p.grad = None
        logits, _ = model(*b['flat'], b['adj'])
        ops.choice_loss(logits.view(-1, nc), b['labels'], 'cross_entropy', 0.1, 1.0).backward()

    def replay(fused):
        b = bs[it[0] % len(bs)]
        it[0] += 1
        steps[fused](*b['flat'], b['adj'], b['labels'], 1.0)

    def stage_setup(fused):
        b = bs[it[0] % len(bs)]
        it[0] += 1
        for p in model.parameters():
            p.grad = None
        out = input_stage(model, b, fused)
        return out, torch.ones_like(out)

    arms = {}
    peak = {}
    capturable = {}
    for fused in (False, True):
        ops.TRAINABLE_TABLE_FUSED = fused
        steps[fused] = graphed.GraphedStep(model, nc, loss='cross_entropy')
        tag = 'fused' if fused else 'stock'
        for _ in range(len(bs)):
            eager()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        eager()
        torch.cuda.synchronize()
        peak[tag] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        try:
            for _ in range(len(bs) + 1):
                replay(fused)
            torch.cuda.synchronize()
            capturable[tag] = True
        except Exception as e:  # (reported, not hidden: the arm is then absent)
            capturable[tag] = False
            lines.append(f'  replay {tag}: not captured: {type(e).__name__}: {str(e)[:120]}')
    for r in range(args.rounds):
        for fused in (False, True):
            ops.TRAINABLE_TABLE_FUSED = fused
            tag = 'fused' if fused else 'stock'
            arms.setdefault(f'eager {tag}', []).append(timed(eager, args.steps, args.warmup))
            if capturable[tag]:
                arms.setdefault(f'replay {tag}', []).append(timed(lambda: replay(fused), args.steps, args.warmup))
            arms.setdefault(f'input stage bwd alone {tag}', []).append(
                event_timed(lambda: stage_setup(fused), lambda st: st[0].backward(st[1]), max(5, args.steps // 3), 2))
    ops.TRAINABLE_TABLE_FUSED = True
    _lib.ERR_WATCH.poll(block=True)
    lines += [table_line(a, t) for a, t in arms.items()]
    for how in ('eager', 'replay', 'input stage bwd alone'):
        if f'{how} stock' in arms and f'{how} fused' in arms:
            lines.append(verdict(f'{how}: stock - fused', arms[f'{how} stock'], arms[f'{how} fused']))
    lines.append(f'  allocator peak of one eager step above the resident model: stock {peak["stock"]:.0f} MiB, fused {peak["fused"]:.0f} MiB')

    # the pieces: what belongs to the reference's semantics (a dense gradient, RAdam over every row) and what to the capacity
    K = ops.kernels()
    b = bs[0]
    _, _, ridx = K.node_prep(b['flat'][3].contiguous(), b['flat'][4].contiguous(), b['flat'][2].contiguous(), b['flat'][1].contiguous(), table_rows=rows)
    L = MQ.head_layout(model.concept_dim, dev)
    Wc_t = L.pad(model.concept_emb.cpt_transform.weight.detach().t()).contiguous()
    Wc = Wc_t.t().contiguous()
    dpre = torch.randn(N, L.DP, device=dev)
    uniq, count, rws = ops.table_row_gradient(ridx, dpre, Wc, rows, Wc_t=Wc_t)
    U, cap = int(count[0]), rws.size(0)
    G = torch.randn(cap, L.DP, device=dev)
    dense = torch.empty(rows, width, device=dev)
    opt = OU.RAdam([dict(params=[table], weight_decay=0.01)], lr=1e-3)
    table.grad = torch.zeros_like(table)
    n_piece = max(5, args.steps // 3)
    pieces = {
        'row groups + segment sums + product': lambda _: ops.table_row_gradient(ridx, dpre, Wc, rows, Wc_t=Wc_t),
        'zero + scatter of the dense gradient': lambda _: K.rows_scatter(rws, uniq, count, K.zero_words(dense)),
        f'product over the capacity ({cap} rows)': lambda _: K.gemm_nn(G, Wc, B1n=Wc_t),
        f'product over the U = {U} live rows': lambda _: K.gemm_nn(G[:max(U, 1)], Wc, B1n=Wc_t),
        'RAdam step over the table alone': lambda _: opt.step(),
    }
    res = {k: [event_timed(lambda: None, fn, n_piece, 2) for _ in range(args.rounds)] for k, fn in pieces.items()}
    lines.append(f'  pieces at batch 0 (HIP events, {n_piece} calls per round), ms per call:')
    lines += ['  ' + table_line(k, t) for k, t in res.items()]
    table.grad = None
    del opt, model, steps
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batches', type=int, default=3, help='different batches per size, cycled')
    ap.add_argument('--dropout', type=float, default=0.2)
    ap.add_argument('--sizes', type=int, nargs='+', default=[2, 64], help='questions per batch (x 5 choices = subgraphs)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda', 0)
    lines = [f'training step of the decoder with a trainable entity table, bench.py model ({bench.K_LAYERS} layers, d = {bench.D}); '
             f'{len(os.sched_getaffinity(0))} CPUs, {torch.get_num_threads()} torch threads', '']
    for label, (rows, width) in TABLES.items():
        for nq in args.sizes:
            lines += measure(label, rows, width, nq, args, dev) + ['']
            print('\n'.join(lines[-12:]), flush=True)
    text = '\n'.join(lines)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    print(text)


if __name__ == '__main__':
    main()
