"""Every host-only answer of the GEMM dispatch, one line each: the scratch queries over a grid of shapes.  Needs no device (the CU
count falls back to 256).  Two builds of the library dispatch alike when their outputs are equal:

    QAGNN_LIB=<other build> python tools/gemm_host_queries.py > a.txt;  python tools/gemm_host_queries.py > b.txt;  cmp a.txt b.txt
"""
import ctypes as C
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from qagnn_amd import _lib  # noqa: E402

# (K1, K2, No): GOLDEN_TRIPLES and the H2_SHAPES of tests/test_hip_kernels.py
TRIPLES = [(208, 112, 624), (208, 208, 208), (624, 0, 208), (208, 0, 208), (32, 16, 96), (32, 0, 32), (96, 0, 16), (16, 0, 16), (64, 32, 192),
           (64, 0, 64), (624, 0, 112), (40, 56, 200), (320, 0, 200)]
ROWS = [1, 255, 2000, 8191, 8192, 12800, 64000]


def main():
    lib = _lib.load_library()
    for R, Ka, No in itertools.product([1, 7, 100, 1024, 2000, 4096, 4097, 12800, 64000, 102400], [16, 32, 64, 112, 208, 320, 624, 1024],
                                       [16, 96, 104, 112, 208, 624]):
        print('tn_workspace_elems', R, Ka, No, lib.qagnn_gemm_tn_workspace_elems(R, Ka, No))
    buf = (C.c_float * 64)()  # stands in for every operand: the queries look at pointers' presence and alignment only
    ptr = C.cast(buf, C.c_void_p)
    for K1, K2, No in TRIPLES:
        print('nn_pack_bytes', K1, K2, No, lib.qagnn_gemm_nn_pack_bytes(No, K1, K2))
        for pieces in (0, 1, 2, 3):
            d = _lib.qagnn_pack_desc(ptr, K1, K1, ptr if K2 else None, K2, K2, No, pieces)
            print('nn_prepack_bytes', K1, K2, No, pieces, lib.qagnn_gemm_nn_prepack_bytes(C.byref(d), 1))
    for thr in (8192, 1):
        old = lib.qagnn_packed_min_rows(thr)
        try:
            for (K1, K2, No), M, amax, pieces, gather in itertools.product(TRIPLES, ROWS, (0, 1), (0, 1), (None, 0, 5000)):
                a = _lib.qagnn_gemm_nn_args()
                a.A1, a.lda1, a.K1 = ptr, K1, K1
                if K2:
                    a.A2, a.lda2, a.K2 = ptr, K2, K2
                a.C, a.ldc, a.M, a.No, a.pieces = ptr, No, M, No, pieces
                if amax:
                    a.a_amax1, a.a_amax2 = ptr, (ptr if K2 else None)
                if gather is not None:
                    a.a_rowidx, a.a_rows = ptr, gather
                print('nn_ws_bytes', thr, K1, K2, No, M, amax, pieces, gather,
                      lib.qagnn_gemm_nn_ws_bytes(C.byref(a), ptr, K1, ptr if K2 else None, K2))
        finally:
            lib.qagnn_packed_min_rows(old)
    # the hop workspaces: N at both sides of the packed-row and row-block thresholds, Ep = 7.2 N as in the benchmark's batches
    for N, DP, SP in itertools.product([1, 2000, 8191, 8192, 12800, 32767, 32768, 64000], (16, 64, 112, 208, 256), (0, 16, 112, 128)):
        Ep = N * 36 // 5
        if SP == 0:
            print('hop_fwd_workspace_elems', N, Ep, DP, lib.qagnn_hop_fwd_workspace_elems(N, Ep, DP))
        for cls_rows in (0, 2, 640, 40960):
            print('hop_bwd_workspace_elems', N, Ep, DP, SP, cls_rows, lib.qagnn_hop_bwd_workspace_elems(N, Ep, DP, SP, cls_rows))


if __name__ == '__main__':
    main()
