// cfz_delay.inl -- the start delays that make a plan set conflict-free (cfz_delay_search / cfz_plan_delays / cfz_loop_plan_delays),
// searched over the conflict map of cfz_conflict.inl.  The map holds, per pair q = (u, w) and lag tau in [-D, D], what the two bodies do
// to each other when w starts tau samples later than u; a vector of start delays d[0..V-1] puts pair q at lag d[w] - d[u], so the search
// reads the map and nothing else.  Plain CFZ_CALL functions, so that the CPU test build (tests/emu/cfz_delay_emu.cpp) compiles the same
// source as delay_kernel in cfz_engine.hip.
//
// Definitions (include/confrez_hip.h states them for the caller).  count[npair][2D+1] (entries `cs` ints apart: the map's info rows carry
// it as their third column), clear[npair][2D+1] or NULL; a slack r >= 0; caps cap[v] in [0, D].
//   free(q, j):     count[q][j] == 0, and clear[q][j] finite where clear is given
//   window(q, j):   every j' in [j - r, j + r] lies in [0, 2D] and is free
//   feasible(d):    0 <= d[v] <= cap[v] for all v, and window(q, d[w] - d[u] + D) for every pair
// The answer is the feasible d that is smallest under (span = max d, total = sum d, idx = sum_v d[v] (D+1)^(V-1-v)).
//
// The search goes through the spans m = 0, 1, ... in ascending order.  Shell m holds the vectors with max = m, each once, as V blocks:
// block k has the vectors whose first digit equal to m is digit k (digits before k in [0, m-1], digits after k in [0, m]), so it has
// m^k (m+1)^(V-1-k) members and the shell (m+1)^V - m^V.  Within a shell a lane keeps the smallest (total, idx) it has seen; delay_merge
// is a minimum under that total order, so the result does not depend on how the candidates are dealt out or in which order the lanes
// are merged.  All integers fit 32 bits: the entry points refuse (D+1)^V > 2^31.
#ifndef CFZ_DELAY_INL
#define CFZ_DELAY_INL

#include <math.h>
#include <stdint.h>

#include "cfz_wave.inl"  // CFZ_CALL, bit_words, bit_test

namespace cfz {

constexpr int kDelayNInfo = 3;  // CFZ_DELAY_NINFO: found, span, total
constexpr int kDelayMaxV = 8;   // CFZ_MAX_NBR + 1

// words of one pair's row of the windowed free mask
CFZ_CALL int delay_words(int D) { return bit_words(2 * D + 1); }

// lag index j of one pair's row is free
CFZ_CALL bool delay_free(const int32_t *count, int cs, const double *clear, int j) {
  if (count[(size_t)j * cs] != 0) return false;
  return !clear || fabs(clear[j]) < INFINITY;  // (false for a NaN)
}

// every lag index in [j - r, j + r] lies inside the row and is free: at most 2D + 1 reads whatever r is
CFZ_CALL bool delay_window_free(const int32_t *count, int cs, const double *clear, int D, int r, int j) {
  if (j < r || j > 2 * D - r) return false;
  for (int t = j - r; t <= j + r; ++t)
    if (!delay_free(count, cs, clear, t)) return false;
  return true;
}

// Shell m of V digits: start[k] is the number of candidates in the blocks before block k, start[V] the size of the shell.
struct DelayShell {
  uint32_t start[kDelayMaxV + 1];
};

CFZ_CALL void delay_shell(int V, int m, DelayShell &sh) {
  const uint32_t b = (uint32_t)m + 1u;
  uint32_t blk = 1u, acc = 0u;  // block k: m^k (m+1)^(V-1-k)
#pragma unroll
  for (int k = 1; k < kDelayMaxV; ++k)
    if (k < V) blk *= b;
#pragma unroll
  for (int k = 0; k < kDelayMaxV; ++k) {
    sh.start[k] = acc;
    if (k < V) { acc += blk; blk = blk / b * (uint32_t)m; }
  }
  sh.start[kDelayMaxV] = acc;
}

CFZ_CALL uint32_t delay_shell_size(const DelayShell &sh) { return sh.start[kDelayMaxV]; }

// A delay vector as the search holds it: eight digits of 16 bits (a digit is at most D <= 46,339), vehicle v in bits 16 (v & 3) of
// lo (v < 4) or hi.  The functions below go over the vehicles and the pairs in loops whose counters are the same for every lane and
// read the digits by shifts, so that no array is indexed by a variable (which would put it into scratch memory) and no condition is
// held per vehicle or per pair.
struct DelayVec {
  uint64_t lo, hi;
};

CFZ_CALL int delay_digit(const DelayVec &d, int v) { return (int)(((v < 4 ? d.lo : d.hi) >> (16 * (v & 3))) & 0xffffu); }

CFZ_CALL void delay_set_digit(DelayVec &d, int v, int x) {
  const uint64_t b = (uint64_t)(uint32_t)x << (16 * (v & 3));
  if (v < 4) d.lo |= b; else d.hi |= b;
}

CFZ_CALL void delay_pack(int V, const int32_t *x, int fill, DelayVec &d) {  // x[0..V-1], or `fill` for every vehicle where x is NULL
  d.lo = d.hi = 0u;
  for (int v = 0; v < V; ++v) delay_set_digit(d, v, x ? x[v] : fill);
}

// candidate c in [0, size) of shell m -> d
CFZ_CALL void delay_decode(int V, int m, const DelayShell &sh, uint32_t c, DelayVec &d) {
  int k = 0;
  uint32_t rem = c;  // (start[0] = 0)
#pragma unroll
  for (int i = 1; i < kDelayMaxV; ++i)
    if (c >= sh.start[i]) { k = i; rem = c - sh.start[i]; }  // (start[i] is the size of the shell from i = V on: never reached)
  // Selects, no branch on the lane's own k: one division per digit.  A digit before k exists only in shells m >= 1.
  const uint32_t lo = m > 0 ? (uint32_t)m : 1u, hi = (uint32_t)m + 1u;
  d.lo = d.hi = 0u;
  for (int v = V - 1; v >= 0; --v) {
    const uint32_t b = v > k ? hi : lo, qt = rem / b;
    delay_set_digit(d, v, v == k ? m : (int)(rem - qt * b));
    rem = v == k ? rem : qt;
  }
}

// d respects the caps and every pair's lag is inside a free window.  Without a branch on the lane's own digits.
CFZ_CALL bool delay_feasible(int V, int D, const DelayVec &d, const DelayVec &cap, const uint32_t *mask, int nw) {
  bool ok = true;
  int q = 0;
  for (int u = 0; u < V; ++u) {
    const int du = delay_digit(d, u);
    ok &= du <= delay_digit(cap, u);
    for (int w = u + 1; w < V; ++w, ++q) { const int j = delay_digit(d, w) - du + D; ok &= (mask[q * nw + (j >> 5)] >> (j & 31)) & 1u; }  // (bit j of row q, one index: measured)
  }
  return ok;
}

// What one lane has seen of one shell: the smallest (total, idx); total INT32_MAX while none.
struct DelayAcc {
  int total;
  int idx;
};

CFZ_CALL void delay_clear(DelayAcc &a) { a.total = INT32_MAX; a.idx = INT32_MAX; }

CFZ_CALL void delay_merge(DelayAcc &a, const DelayAcc &b) {
  if (b.total < a.total || (b.total == a.total && b.idx < a.idx)) a = b;
}

CFZ_CALL void delay_take(DelayAcc &a, int V, int D, const DelayVec &d) {
  DelayAcc b;
  b.total = 0; b.idx = 0;
  for (int v = 0; v < V; ++v) {
    const int x = delay_digit(d, v);
    b.total += x; b.idx = b.idx * (D + 1) + x;
  }
  delay_merge(a, b);
}

// Lane `lane` of `nl` over shell m: candidates lane, lane + nl, ...
CFZ_CALL void delay_lane(DelayAcc &acc, int lane, int nl, int V, int D, int m, const DelayShell &sh, const DelayVec &cap,
                         const uint32_t *mask, int nw) {
  delay_clear(acc);
  const uint32_t n = delay_shell_size(sh);
  for (uint32_t c = (uint32_t)lane; c < n; c += (uint32_t)nl) {
    DelayVec d;
    delay_decode(V, m, sh, c, d);
    if (delay_feasible(V, D, d, cap, mask, nw)) delay_take(acc, V, D, d);
  }
}

// The outputs of one set from the merged accumulator of the shell at which the search stopped (m; acc empty: nothing is feasible).
// count, clear: the set's rows; rclear is written only where clear is given.
CFZ_CALL void delay_store(const DelayAcc &a, int V, int D, int m, const double *clear, int32_t *delays, int32_t *info, double *rclear) {
  const bool found = a.total != INT32_MAX;
  int idx = found ? a.idx : 0;
  for (int v = V - 1; v >= 0; --v) {
    const int qt = idx / (D + 1);
    delays[v] = found ? idx - qt * (D + 1) : -1;
    idx = qt;
  }
  info[0] = found ? 1 : 0; info[1] = found ? m : -1; info[2] = found ? a.total : -1;
  if (!clear || !rclear) return;
  double best = found ? INFINITY : -INFINITY;
  if (found) {
    int q = 0;
    for (int u = 0; u < V - 1; ++u)
      for (int w = u + 1; w < V; ++w, ++q) {
        const double c = clear[(size_t)q * (2 * D + 1) + (delays[w] - delays[u] + D)];
        if (c < best) best = c;
      }
  }
  *rclear = best;
}

}  // namespace cfz

#endif  // CFZ_DELAY_INL
