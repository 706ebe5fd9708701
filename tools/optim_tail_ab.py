"""A/B/C of the tail of a training step -- clip the gradient norm, then RAdam -- on the decoder's real tensor list, in ONE process.

  A  torch.nn.utils.clip_grad_norm_(params, 1.0); opt.step()                            what a user of the fused RAdam alone runs
  B  optimization_utils.clip_grad_norm_(params, 1.0); opt.step()                        norm on the device + in-place scale
  C  optimization_utils.clip_grad_norm_(params, 1.0, defer_to=opt); opt.step()          norm on the device, scale inside the RAdam kernel

The three forms alternate round by round (A B C A B C ...) on their own clones of one (p, m, v) state at step 6 and later, HIP events on
the launch stream around each, the gradients restored from a saved copy in front of every timed region (outside it: A and B overwrite
them).  Twice: the trainable tensors of the CSQA decoder with gradients as misaligned views of one flat buffer, and ONE tensor holding the
whole flat buffer (parallel.GradBucket.flat).  Bytes are computed from shapes: 4 B per element and pass.

    python tools/optim_tail_ab.py [--rounds 60] [--warmup 10] [--out profiles/clip_radam_ab.txt]
    rocprofv3 --kernel-trace --stats ... -- python tools/optim_tail_ab.py --count FORM --list decoder|flat   (FORM: none, A, B, C)
        runs the set-up and then FORM `--rounds` times with nothing else in between: the kernel count of the run minus that of
        `--count none`, over the rounds, is the launches per call.
    python tools/optim_tail_ab.py --summarise DIR --rounds R    reads DIR/prof_<FORM>_<list>/**/*kernel_stats*.csv of those eight runs
"""
import argparse
import csv
import glob
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qagnn_amd import modeling_qagnn as MQ  # noqa: E402
from qagnn_amd import optimization_utils as OU  # noqa: E402

MAX_NORM = 1.0


def decoder_shapes():
    torch.manual_seed(0)
    model = MQ.QAGNN(None, 5, 4, 38, 1024, 3000, 200, 1024, 2, 200, 0, 0.2, 0.2, 0.2)
    return [tuple(p.shape) for p in model.parameters() if p.requires_grad]


class Form:
    """One form's own parameters, optimiser state and gradient views."""

    def __init__(self, shapes, p0, m0, v0, g0):
        self.g0 = g0
        self.flat = torch.empty(g0.numel() + 3, device='cuda')[3:]  # 12-byte offset: no view is 16-byte aligned
        self.params, off = [], 0
        for s, p in zip(shapes, p0):
            q = torch.nn.Parameter(p.clone())
            q.grad = self.flat[off:off + q.numel()].view(s)
            off += q.numel()
            self.params.append(q)
        self.opt = OU.RAdam(self.params, lr=1e-3, weight_decay=0.01)
        for q, m, v in zip(self.params, m0, v0):
            self.opt.state[q] = dict(step=5, exp_avg=m.clone(), exp_avg_sq=v.clone())

    def restore(self):
        self.flat.copy_(self.g0)

    def run(self, which):
        if which == 'A':
            torch.nn.utils.clip_grad_norm_(self.params, MAX_NORM)
        elif which == 'B':
            OU.clip_grad_norm_(self.params, MAX_NORM)
        else:
            OU.clip_grad_norm_(self.params, MAX_NORM, defer_to=self.opt)
        self.opt.step()


def make_forms(shapes, names='ABC'):
    gen = torch.Generator(device='cuda').manual_seed(6)
    p0 = [torch.randn(s, generator=gen, device='cuda') for s in shapes]
    m0 = [0.01 * torch.randn(s, generator=gen, device='cuda') for s in shapes]
    v0 = [(0.01 * torch.randn(s, generator=gen, device='cuda')) ** 2 for s in shapes]
    g0 = torch.randn(sum(p.numel() for p in p0), generator=gen, device='cuda')
    return {n: Form(shapes, p0, m0, v0, g0) for n in names}


def measure(shapes, rounds, warmup):
    forms = make_forms(shapes)
    ms = {n: [] for n in forms}
    for r in range(warmup + rounds):
        for n, f in forms.items():
            f.restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f.run(n)
            e1.record()
            e1.synchronize()
            if r >= warmup:
                ms[n].append(e0.elapsed_time(e1))
    # the three forms compute the same update: B and C bit for bit, A to the rounding of torch's fp32 norm
    same_bc = all(torch.equal(a, b) for a, b in zip(forms['B'].params, forms['C'].params))
    worst_ab = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(forms['A'].params, forms['B'].params) if a.numel())
    return ms, same_bc, worst_ab


def quant(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


def table(title, shapes, rounds, warmup):
    n_el = sum(int(torch.Size(s).numel()) for s in shapes)
    ms, same_bc, worst_ab = measure(shapes, rounds, warmup)
    passes = {'A': (3 + 7, 'clip: read g (norm), read + write g (scale); RAdam: 4 reads + 3 writes'),
              'B': (3 + 7, 'norm: read g; scale: read + write g; RAdam: 4 reads + 3 writes'),
              'C': (1 + 7, 'norm: read g; RAdam: 4 reads + 3 writes (g scaled as it is read)')}
    lines = [f'{title}: {len(shapes)} tensor(s), {n_el} fp32 elements; {rounds} rounds after {warmup} warm-up rounds, ms per clip + step (HIP events)',
             f'  {"form":4s} {"median":>8s} {"min":>8s} {"p10":>8s} {"p90":>8s} {"max":>8s}   {"MB moved":>9s}  passes']
    for n in 'ABC':
        x = ms[n]
        lines.append(f'  {n:4s} {statistics.median(x):8.4f} {min(x):8.4f} {quant(x, 0.1):8.4f} {quant(x, 0.9):8.4f} {max(x):8.4f}   '
                     f'{passes[n][0] * 4 * n_el / 1e6:9.1f}  {passes[n][1]}')
    lines.append(f'  results after {warmup + rounds} steps: B == C bit for bit: {same_bc}; max |A - B| over the parameters: {worst_ab:.3e}')
    return lines


def summarise(out, rounds):
    """Launches per clip + step from the rocprofv3 kernel statistics of the --count runs (per kernel name: calls beyond the set-up-only run)."""
    lines = []
    for lst in ('decoder', 'flat'):
        calls = {}
        for form in ('none', 'A', 'B', 'C'):
            files = glob.glob(os.path.join(out, f'prof_{form}_{lst}', '**', '*kernel_stats*.csv'), recursive=True)
            assert len(files) == 1, (form, lst, files)
            with open(files[0]) as fh:
                calls[form] = {r['Name']: int(r['Calls']) for r in csv.DictReader(fh)}
        base = calls['none']
        for form in 'ABC':
            extra = {n: (c - base.get(n, 0)) / rounds for n, c in calls[form].items() if c != base.get(n, 0)}
            lines.append(f'{lst:8s} form {form}: {sum(extra.values()):5.1f} launches per clip + step  ({sum(calls[form].values())} kernels in the run, '
                         f'{sum(base.values())} in the set-up-only run, {rounds} rounds)')
            lines += [f'    {c:5.1f}  {n[:140]}' for n, c in sorted(extra.items(), key=lambda x: (-x[1], x[0]))]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--count', choices=['none', 'A', 'B', 'C'], default=None)
    ap.add_argument('--list', choices=['decoder', 'flat'], default='decoder')
    ap.add_argument('--summarise', default=None)
    args = ap.parse_args()
    if args.summarise:
        print('\n'.join(summarise(args.summarise, args.rounds)))
        return
    assert torch.cuda.is_available(), 'needs an MI355X'
    dec = decoder_shapes()
    flat = [(sum(int(torch.Size(s).numel()) for s in dec),)]
    if args.count is not None:
        name = 'A' if args.count == 'none' else args.count
        f = make_forms(dec if args.list == 'decoder' else flat, name)[name]
        f.restore()
        if args.count != 'none':
            for _ in range(args.rounds):
                f.run(name)
        torch.cuda.synchronize()
        print(f'count run: form {args.count}, list {args.list}, {args.rounds} rounds')
        return
    lines = table('decoder tensor list', dec, args.rounds, args.warmup) + [''] + table('one flat bucket', flat, args.rounds, args.warmup)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
