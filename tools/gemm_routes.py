"""One call per branch of the GEMM dispatch (csrc/gemm_dispatch.hip), through the provider -- to be run under a kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/gemm_routes.py
    QAGNN_GEMM_SPLIT=0 rocprofv3 --kernel-trace --output-format csv -d OUT0 -- python tools/gemm_routes.py     (the fp32-MFMA pin)

Two builds of the library (QAGNN_LIB) route alike when their traces list the same launches in the same order:

    python tools/gemm_routes.py --compare A_kernel_trace.csv B_kernel_trace.csv [--symbols mangled_names.txt]

--symbols: every kernel named in the file (one mangled symbol per line) must occur in trace A; the ones that do not are listed.
No result is checked here (tests/ does that); the operands are ones."""
import csv
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

# (rows, output columns) -> column tiles per block of the bf16 kernels on 256 CUs: the tile narrows with the row count
NT_SHAPES = [(64000, 208, 13), (64000, 128, 8), (30000, 208, 7), (12800, 208, 4), (2000, 208, 2)]


def drive():
    import torch
    from qagnn_amd import ops
    K = ops.kernels()
    dev = torch.device('cuda')
    ones = lambda *s: torch.ones(*s, device=dev)  # noqa: E731
    split0 = K.gemm_split
    pinned = os.environ.get('QAGNN_GEMM_SPLIT') == '0'

    def nn(tag, M, K1, K2, No, affine=False, stats=False, gather=False, amax=False, epilogue=False, accumulate=False, fp32=False):
        print('NN', tag, M, K1, K2, No, flush=True)
        A1 = ones(M // 2 if gather else M, K1)
        B1, B1n = ones(K1, No), ones(No, K1)
        kw = {}
        if K2:
            kw.update(A2=ones(M, K2), B2=ones(K2, No), B2n=None if fp32 else ones(No, K2))
        if affine:
            kw.update(a_scale=ones(K1), a_shift=ones(K1))
        if gather:
            kw.update(a_rowidx=torch.arange(M, device=dev) % (M // 2))
        if amax:
            kw.update(a_amax1=K.absmax(A1), a_amax2=K.absmax(kw['A2']) if K2 else None)
        if epilogue:
            kw.update(bias=ones(No), rowtab=ones(4, No), rowidx=torch.arange(M, device=dev) % 4)
        if accumulate:
            kw.update(out=ones(M, No), accumulate=True)
        K.gemm_nn(A1, B1, B1n=None if fp32 else B1n, colstats=stats, **kw)

    def tn(tag, R, Ka, No, Ka2=0, h2=False, affine=False, gather=False, groups=0, accumulate=False):
        print('TN', tag, R, Ka, Ka2, No, flush=True)
        A, B = ones(R // 2 if gather else R, Ka), ones(R, No)
        sc = dict(a_scale=ones(Ka), a_shift=ones(Ka)) if affine else {}
        if h2:
            A2 = ones(R, Ka2) if Ka2 else None
            K.gemm_tn_h2(A, B, K.absmax(A), K.absmax(B), A2=A2, amax_a2=K.absmax(A2) if Ka2 else None, **sc)
        elif Ka2:
            K.gemm_tn2(A, ones(R, Ka2), B)
        else:
            if gather:
                sc.update(a_rowidx=torch.arange(R, device=dev) % (R // 2))
            if groups:
                sc.update(colsum_groups=groups, b_rowidx=(torch.arange(R, device=dev) % groups) if groups > 1 else None)
            if accumulate:
                sc.update(out=ones(Ka, No), accumulate=True)
            K.gemm_tn(A, B, **sc)

    # ---- weight gradients on the fp32-MFMA kernels: what the split kernels decline (column sums, < 1024 rows, narrow operands) -- or all, pinned
    for aff in (False, True):
        for No in (208, 128, 112, 64, 32):
            tn('runtime', 1000, 80, No, affine=aff)                      # k_gemm_tn<13 | 8 | 7 | 4 | 2>
        for Ka in (112, 208, 1024):
            tn('strip', 1000, Ka, 208, affine=aff)                       # k_gemm_tn_strip<13, 7 | 13 | 16 waves>
            tn('strip colsum 1', 64000, Ka, 208, affine=aff, groups=1)
    tn('strip colsum 4', 20000, 208, 208, groups=4)
    tn('runtime colsum 4', 2000, 80, 128, groups=4)
    tn('strip accumulate', 700, 208, 208, accumulate=True)
    tn('strip 64000 x 208 x 624 (split unless pinned)', 64000, 208, 624)
    tn('two operands, unmerged (32 columns of A2)', 64000, 208, 208, Ka2=32)
    if pinned:  # the NN products of a provider that reads the same pin: fp32-MFMA kernels only
        for No in (208, 128, 112, 64, 32):
            for aff in (False, True):
                nn('pinned', 2000, 208, 0, No, affine=aff)
        torch.cuda.synchronize()
        return

    # ---- weight gradients on the split kernels
    for gs in (1, 2, 3):  # six MFMAs | three (scaled fp16 pairs) | one (fp16)
        K.gemm_split = gs
        for aff in (False, True):
            tn('split (7,13)', 20000, 112, 624, h2=gs > 1, affine=aff)
            tn('split (13,7)', 20000, 208, 208, h2=gs > 1, affine=aff)
        tn('split, 32-row chunks', 2000, 208, 208, h2=gs > 1)
        tn('two operands, k_gemm_tn_ws', 64000, 208, 624, Ka2=112, h2=gs > 1)
        tn('two operands, short chunks', 12800, 208, 208, Ka2=208, h2=gs > 1)
        tn('two operands, 10 subgraphs', 2000, 208, 624, Ka2=112, h2=gs > 1)
        tn('declared fallback: 60 rows', 60, 208, 624, Ka2=112, h2=gs > 1)
        tn('declared fallback: 257 rows', 257, 624, 208, h2=gs > 1)
    K.gemm_split = split0
    tn('split gather', 20000, 208, 208, gather=True)
    tn('gather the split kernels decline (112 columns)', 20000, 112, 208, gather=True)
    tn('split accumulate', 20000, 208, 208, accumulate=True)

    # ---- NN, fp32 MFMA (no [No, K] weights handed over)
    for No in (208, 128, 112, 64, 32):
        for aff in (False, True):
            nn('fp32', 2000, 208, 0, No, affine=aff, fp32=True)
    nn('fp32 two segments + epilogue', 12800, 208, 112, 624, epilogue=True, fp32=True)

    # ---- NN, first-generation split kernel: a K that is no multiple of 8
    K.gemm_split = 1
    for M, No, _ in NT_SHAPES:
        for aff in (False, True):
            for gather in (False, True):
                nn('split gen 1', M, 12, 0, No, affine=aff, gather=gather)
        if No == 208:
            nn('split gen 1 stats', M, 12, 0, No, stats=True)
    nn('split gen 1 two segments + epilogue', 12800, 12, 20, 208, epilogue=True)

    # ---- NN, second generation.  In-kernel split of B: below the row threshold (raised for the wide tiles)
    old = K.packed_min_rows(10 ** 9)
    for M, No, _ in NT_SHAPES:
        for aff in (False, True):
            nn('nn2 in-kernel', M, 208, 0, No, affine=aff)
        if No == 208:
            nn('nn2 in-kernel stats', M, 208, 0, No, stats=True)
    nn('nn2 in-kernel gather', 12800, 208, 0, 208, gather=True)
    nn('nn2 in-kernel two segments + epilogue', 2000, 208, 112, 624, epilogue=True)
    K.packed_min_rows(1)  # ... and every row count in the packed forms
    for gs in (1, 2, 3):  # B packed per call: six MFMAs (4-wave blocks: 7 k-tiles) | three | one
        K.gemm_split = gs
        for M, No, _ in NT_SHAPES:
            for aff in (False, True):
                nn('nn2 pack', M, 208, 0, No, affine=aff, amax=gs > 1)
            if No == 208:
                nn('nn2 pack stats', M, 208, 0, No, stats=True, amax=gs > 1)
    K.gemm_split = 1
    for No in (624, 128):  # the staggered 8-wave block: >= 10 k-tiles, >= 0.9 256-row tiles per CU, 13 or 8 column tiles
        for aff in (False, True):
            nn('nn2 staggered', 64000, 208, 112, No, affine=aff)
    nn('nn2 staggered 624 -> 208', 64000, 624, 0, 208)
    nn('nn2 staggered stats', 64000, 320, 0, 208, stats=True)
    nn('nn2 staggered gather', 64000, 320, 0, 208, gather=True)
    nn('nn2 staggered accumulate', 64000, 624, 0, 208, accumulate=True)
    nn('staggered refused: 7 k-tiles', 64000, 208, 0, 208)
    nn('staggered refused: 7 column tiles', 64000, 624, 0, 112)
    K.packed_min_rows(old)
    nn('threshold: 8191 rows', 8191, 208, 112, 624)
    nn('threshold: 8192 rows', 8192, 208, 112, 624)
    K.gemm_split = 2
    nn('threshold: 8191 rows, maxima known', 8191, 208, 112, 624, amax=True)
    nn('threshold: 8192 rows, maxima known', 8192, 208, 112, 624, amax=True)
    # registered images (one launch packs them all): six-MFMA and three-MFMA images of the same weights
    W1, W2, W3 = ones(624, 208), ones(624, 112), ones(208, 624)
    keep = K.prepack([(W1, W2), (W1, W2, 2), (W3, None), (W3, None, 2)], tag=77)
    for amax in (False, True):
        print('NN registered image', amax, flush=True)
        A1, A2, A3 = ones(64000, 208), ones(64000, 112), ones(64000, 624)
        K.gemm_nn(A1, W1.t().contiguous(), A2=A2, B2=W2.t().contiguous(), B1n=W1, B2n=W2, a_amax1=K.absmax(A1) if amax else None,
                  a_amax2=K.absmax(A2) if amax else None)
        K.gemm_nn(A3, W3.t().contiguous(), B1n=W3, a_amax1=K.absmax(A3) if amax else None)
    K.prepack_clear(77)
    del keep
    K.gemm_split = split0
    torch.cuda.synchronize()


def launches(path):
    """the ordered (kernel, grid, workgroup, LDS bytes) list of a rocprofv3 kernel trace"""
    with open(path, newline='') as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r['Dispatch_Id']))  # enqueue order
    col = lambda r, stem: tuple(int(r[f'{stem}_{a}']) for a in 'XYZ')  # noqa: E731
    return [(r['Kernel_Name'], col(r, 'Grid_Size'), col(r, 'Workgroup_Size'), int(r['LDS_Block_Size'])) for r in rows]


def compare(a_path, b_path, symbols=None):
    a, b = launches(a_path), launches(b_path)
    print(f'{a_path}: {len(a)} launches, {len({k[0] for k in a})} distinct kernels;  {b_path}: {len(b)} launches')
    bad = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
    for i, x, y in bad[:10]:
        print(f'  launch {i} differs:\n    {x}\n    {y}')
    same = len(a) == len(b) and not bad
    print('launch lists', 'IDENTICAL' if same else 'DIFFER')
    if symbols:
        with open(symbols) as f:
            names = f.read().split()
        plain = subprocess.run(['c++filt'] + names, capture_output=True, text=True, check=True).stdout.split('\n')
        strip = lambda s: s.replace(' ', '').replace('.kd', '')  # noqa: E731
        seen = {strip(k[0]) for k in a}
        missing = [n for n, p in zip(names, plain) if strip(p) not in seen and strip(p.split('(')[0]) not in {s.split('(')[0] for s in seen}]
        print(f'{len(names) - len(missing)} of {len(names)} kernel symbols traced; not traced:')
        for n in missing:
            print('  ', n)
    return 0 if same else 1


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[5] if len(sys.argv) > 5 and sys.argv[4] == '--symbols' else None))
    drive()
