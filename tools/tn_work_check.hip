// The partition of the live-tile weight gradient (csrc/common.h: tn_work / tn_slot) checked on the host over a grid of (S, T, L): a
// stand-alone program, no device needed.  Meant for a sanitizer build of the host side:
//
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -o tn_work_check tools/tn_work_check.hip
//     ./tn_work_check
//
// For every case: the units of a row block are a bijection onto the S partial tiles; the M ranges cover every k-tile exactly once; the K
// and the Q lists cover every list position in [0, L) exactly once, slot lengths differing by at most one; cM + 2 cK == S; without a
// dead tile the partition is that of the launch without a table (S / 3 chunks of chunk_tiles for every column block).
#include <stdio.h>

#include <vector>

#include "../qagnn_amd/csrc/common.h"

using namespace qagnn;

static int check(int S, int T, int L) {
  const int nch = S / 3, ct = (T + nch - 1) / nch;
  const TnWork w = tn_work(S, T, L, ct);
  int bad = 0;
#define EXPECT(c)                                                                  \
  if (!(c)) {                                                                      \
    if (!bad) printf("S=%d T=%d L=%d: %s\n", S, T, L, #c);                         \
    ++bad;                                                                         \
  }
  EXPECT(w.cK >= 1 && w.cM >= 1 && w.cM + 2 * w.cK == S);
  std::vector<int> ps(S, 0), m(T, 0), kq[2] = {std::vector<int>(T, 0), std::vector<int>(T, 0)};
  int lo[2] = {1 << 30, 1 << 30}, hi[2] = {-1, -1}, prev_cb = -1, prev_j = -1;
  for (int u = 0; u < S; ++u) {
    const TnSlot s = tn_slot(w, S, T, u);
    EXPECT(s.pslot >= 0 && s.pslot < S && s.cnt >= 0 && s.beg >= 0 && s.beg + s.cnt <= T);
    if (s.pslot < 0 || s.pslot >= S || s.cnt < 0 || s.beg < 0 || s.beg + s.cnt > T) continue;
    ++ps[s.pslot];
    EXPECT(s.cb == (s.pslot < w.cK ? 0 : s.pslot < 2 * w.cK ? 2 : 1));
    if (s.cb == 1) {
      EXPECT(!s.list);
      for (int i = 0; i < s.cnt; ++i) ++m[s.beg + i];
    } else {
      const int k = s.cb == 2;
      EXPECT(s.list == (L < T));
      for (int i = 0; i < s.cnt; ++i) ++kq[k][s.beg + i];
      if (s.list) { lo[k] = s.cnt < lo[k] ? s.cnt : lo[k]; hi[k] = s.cnt > hi[k] ? s.cnt : hi[k]; }
      // the Q block of a slot index follows its K block: same list, neighbours in the block order
      if (s.cb == 2) EXPECT(prev_cb == 0 && prev_j == s.pslot - w.cK);
    }
    prev_cb = s.cb;
    prev_j = s.pslot;
  }
  for (int i = 0; i < S; ++i) EXPECT(ps[i] == 1);
  for (int t = 0; t < T; ++t) EXPECT(m[t] == 1);
  const int covered = L < T ? L : T;  // lists: positions of the live list; no dead tile: ranges of tiles
  for (int k = 0; k < 2; ++k) {
    for (int t = 0; t < T; ++t) EXPECT(kq[k][t] == (t < covered ? 1 : 0));
    if (L < T) EXPECT(hi[k] - lo[k] <= 1);
  }
  if (L >= T) {
    EXPECT(w.cK == nch && w.cM == nch && w.lenM == ct);
    for (int u = 0; u < S; ++u) {
      const TnSlot s = tn_slot(w, S, T, u);
      const int j = s.cb == 0 ? s.pslot : s.cb == 2 ? s.pslot - w.cK : s.pslot - 2 * w.cK;
      const int beg = j * ct < T ? j * ct : T, cnt = T - beg < ct ? T - beg : ct;
      EXPECT(!s.list && s.beg == beg && s.cnt == cnt);
    }
  }
#undef EXPECT
  return bad;
}

int main() {
  int bad = 0, cases = 0;
  for (int S : {3, 6, 9, 12, 27, 84, 87, 162, 165, 300})
    for (int T : {1, 2, 3, 5, 31, 32, 33, 84, 100, 756, 757, 1513, 2000, 2001, 4099})
      for (int L : {0, 1, 2, T / 4, T / 3, T / 2, (3 * T) / 4, T - 2, T - 1, T, T + 5, -3}) {
        if (T < S / 3) continue;  // (a route with fewer k-tiles than chunks does not exist)
        bad += check(S, T, L < 0 ? 0 : L > T ? T : L) ? 1 : 0;
        ++cases;
      }
  printf("%d cases, %d bad\n", cases, bad);
  return bad ? 1 : 0;
}
