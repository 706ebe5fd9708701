// Timings of k_gemm_tn_ws / k_gemm_tn_split (csrc/gemm_split.hip compiled into this program): the weight-gradient products of the
// 320-subgraph batch, kernel alone (no chunk sum), HIP events.  Build: tools/build_micro.sh, run: tools/bin/tn_ablate.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../qagnn_amd/csrc/gemm_split.hip"

namespace qagnn {
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}
}  // namespace qagnn

#define CK(x)                                                                      \
  do {                                                                             \
    hipError_t e = (x);                                                            \
    if (e != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e)); exit(1); } \
  } while (0)

static float* dev_rand(size_t n, unsigned seed) {
  std::vector<float> h(n);
  unsigned s = seed * 2654435761u + 12345u;
  for (size_t i = 0; i < n; ++i) {
    s = s * 1664525u + 1013904223u;
    h[i] = ((s >> 8) & 0xFFFF) / 32768.0f - 1.0f;
  }
  float* d;
  CK(hipMalloc(&d, n * 4));
  CK(hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice));
  return d;
}

int main() {
  const int R = 64000;
  // chunk: the rows per split-K chunk the library takes for the shape at 64 000 rows on 256 CUs (tn_route, gemm_dispatch.hip)
  struct Shape { const char* name; int Ka1, Ka2, No, chunk; } shapes[] = {{"[X|S]^T dKMQ  208+112 x 624", 208, 112, 624, 2304}, {"208 x 624", 208, 0, 624, 768},
                                                                         {"208 x 208", 208, 0, 208, 256}, {"112 x 624", 112, 0, 624, 384}};
  hipStream_t st;
  CK(hipStreamCreate(&st));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  printf("R=%d\n", R);
  for (auto& sh : shapes) {
    float* A1 = dev_rand((size_t)R * sh.Ka1, 1);
    float* A2 = sh.Ka2 ? dev_rand((size_t)R * sh.Ka2, 2) : nullptr;
    float* B = dev_rand((size_t)R * sh.No, 3);
    const int chunk = sh.chunk, nchunk = (R + chunk - 1) / chunk;
    float* P;
    CK(hipMalloc(&P, (size_t)nchunk * (sh.Ka1 + sh.Ka2) * sh.No * 4));
    const qagnn::TnProduct p = qagnn::tn_product(A1, sh.Ka1, sh.Ka1, A2, sh.Ka2, sh.Ka2, B, sh.No, nullptr, sh.No, R, sh.No, nullptr, nullptr, P);
    const bool wide_b = sh.Ka2 || sh.Ka1 <= 112;  // (KT, NT) = (7, 13), else (13, 7)
    qagnn::TnRoute r = {};
    r.np = 3; r.kt = wide_b ? 7 : 13; r.nt = 20 - r.kt; r.chunk_rows = chunk; r.nchunks = nchunk;
    r.grid = dim3((sh.No + r.nt * 16 - 1) / (r.nt * 16), (sh.Ka1 + r.kt * 16 - 1) / (r.kt * 16) + (sh.Ka2 ? (sh.Ka2 + 111) / 112 : 0), nchunk);
    for (int ws = 0; ws < 2; ++ws) {
      auto run = [&] {
        if (wide_b) ws ? qagnn::launch_tn_ws_i<7, 13>(r, p, st) : qagnn::launch_tn_split_i<7, 13, false>(r, p, st);
        else ws ? qagnn::launch_tn_ws_i<13, 7>(r, p, st) : qagnn::launch_tn_split_i<13, 7, false>(r, p, st);
      };
      for (int i = 0; i < 3; ++i) run();
      CK(hipStreamSynchronize(st));
      const int reps = 30;
      CK(hipEventRecord(e0, st));
      for (int i = 0; i < reps; ++i) run();
      CK(hipEventRecord(e1, st));
      CK(hipStreamSynchronize(st));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      const double us = ms * 1e3 / reps;
      printf("  %-30s %s  chunks %3d x %4d rows  %8.1f us  %7.1f TFLOP/s fp32-eq\n", sh.name, ws ? "k_gemm_tn_ws   " : "k_gemm_tn_split", nchunk, chunk, us,
             2.0 * R * (sh.Ka1 + sh.Ka2) * sh.No / us / 1e6);
    }
    CK(hipFree(A1)); CK(hipFree(B)); CK(hipFree(P));
    if (A2) CK(hipFree(A2));
  }
  return 0;
}
