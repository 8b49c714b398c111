// cfz_schedule.inl -- hold-point schedules that make a plan set conflict-free (cfz_plan_schedule / cfz_loop_plan_schedule), searched
// over the coordination diagrams of cfz_coord.inl.  The delay search (cfz_delay.inl) lets a vehicle wait at its first sample only; here
// it may wait wherever the caller's hold mask says so (a parking manoeuvre rests at every cusp), and the vehicles are scheduled one
// after the other in a priority order.  Plain CFZ_CALL functions without any floating point, so that the CPU test build
// (tests/emu/cfz_schedule_emu.cpp) compiles the same source as schedule_kernel in cfz_engine.hip and every output is the same integer.
//
// Definitions (include/confrez_hip.h states them for the caller).  A schedule s(t), t in [0, H): s(0) = 0, steps of 0 or 1, a step of 0
// only at a holdable sample or at the goal g = length - 1, s(H-1) = g.  Conflict-free with slack r against fixed schedules s_e: for
// every t and every t' = clamp(t + d, 0, H-1), |d| <= r, the diagram of the pair has a 0 at (s(t), s_e(t')) and at (s(t'), s_e(t)); both
// say the same: s(t) avoids the blocked rows of s_e(t') for every such t'.  An order pi schedules pi_0, pi_1, ... in turn, each with the
// smallest arrival and, among those, the pointwise largest schedule.
//
// One vehicle of one order is a reachability recursion over rows of T bits, lane l of the wavefront holding word l (T <= 2048):
//   R_0 = {0} & free_0,   R_t = ((R_{t-1} << 1, with bit 31 of lane l-1 carried in) | (R_{t-1} & hold)) & free_t
//   free_t = valid & AND over the earlier vehicles e of the order and |d| <= r of ~row_e(s_e(clamp(t + d)))
// row_e(i): the row of the pair's diagram on the side whose rows are e's samples.  The rows R_t are kept (hist[H][words]); the walk back
// from (g, H-1) stays at i where bit i of R_{t-1} is set and i may be held, else comes from i - 1: the pointwise largest schedule.  While
// it stays at g it runs through the last unbroken run of t with bit g set, so where it leaves g is the smallest arrival.
#ifndef CFZ_SCHEDULE_INL
#define CFZ_SCHEDULE_INL

#include <stdint.h>

#include "cfz_coord.inl"

namespace cfz {

constexpr int kScheduleNInfo = 5;       // CFZ_SCHEDULE_NINFO: found, order, makespan, total, feasible orders
constexpr int kScheduleMaxV = 8;        // CFZ_MAX_NBR + 1
constexpr int kScheduleMaxT = 2048;     // CFZ_SCHEDULE_MAX_T: 64 lanes x 32 bits
constexpr int kScheduleMaxH = 32768;    // CFZ_SCHEDULE_MAX_H
constexpr int kScheduleLdsBytes = 147456;  // the four wavefronts' rows and schedules lie in LDS up to these 144 KB of the CU's 160, else in global memory
constexpr int kScheduleAhead = 8;       // steps whose free words are loaded before their dependent chain runs

// An order as the search holds it: vehicle pi_k in bits 4 k of one word (V <= 8), read by shifts: no array indexed by a variable.
CFZ_CALL int schedule_digit(uint32_t order, int k) { return (int)((order >> (4 * k)) & 15u); }

CFZ_CALL uint32_t schedule_pack(int V, const int32_t *pi) {
  uint32_t o = 0u;
  for (int k = 0; k < V; ++k) o |= (uint32_t)pi[k] << (4 * k);
  return o;
}

// pi[0..V-1] is a permutation of 0..V-1
CFZ_CALL bool schedule_is_permutation(int V, const int32_t *pi) {
  uint32_t seen = 0u;
  for (int k = 0; k < V; ++k) {
    if (pi[k] < 0 || pi[k] >= V) return false;
    seen |= 1u << pi[k];
  }
  return seen == (1u << V) - 1u;
}

// 32-bit words one wavefront keeps for one order: the rows R_t and the schedules of the order's vehicles as 16-bit samples
CFZ_CALL size_t schedule_wave_words(int V, int T, int H) { return (size_t)H * coord_words(T) + ((size_t)V * H + 1) / 2; }

// word l of the samples of a plan of `len` samples: all of them
CFZ_CALL uint32_t schedule_valid_word(int len, int l) {
  const int n = len - 32 * l;
  return n <= 0 ? 0u : (n >= 32 ? 0xffffffffu : (1u << n) - 1u);
}

// word l of the samples that may be held: the caller's bytes hold[0..len-1], and the goal
CFZ_CALL uint32_t schedule_hold_word(const uint8_t *hold, int len, int l) {
  uint32_t w = 0u;
  for (int b = 0; b < 32; ++b) {
    const int i = 32 * l + b;
    if (i < len && (hold[i] != 0 || i == len - 1)) w |= 1u << b;
  }
  return w;
}

// word l of free_t for the vehicle at position k of the order: diag the set's [npair][2][T][nw], sched[k'][H] the schedules of the
// positions before k.  Does not depend on R.  l < nw.
CFZ_CALL uint32_t schedule_free_word(const uint32_t *diag, int V, int T, int nw, int H, int r, uint32_t order, int k, const uint16_t *sched,
                                     int t, int l, uint32_t valid) {
  const int v = schedule_digit(order, k);
  uint32_t f = valid;
  for (int kk = 0; kk < k; ++kk) {
    const int e = schedule_digit(order, kk);
    const int q = e < v ? coord_pair_index(V, e, v) : coord_pair_index(V, v, e);
    const uint32_t *rows = diag + ((size_t)q * 2 + (e < v ? 0 : 1)) * (size_t)T * nw;  // the side whose rows are e's samples
    for (int d = -r; d <= r; ++d) {
      int tt = t + d;
      tt = tt < 0 ? 0 : (tt > H - 1 ? H - 1 : tt);
      f &= ~rows[(size_t)sched[(size_t)kk * H + tt] * nw + l];
    }
  }
  return f;
}

// word l of R_0
CFZ_CALL uint32_t schedule_first(int l, uint32_t fr) { return (l == 0 ? 1u : 0u) & fr; }

// word l of R_t from word l and word l - 1 (prev; 0 for lane 0) of R_{t-1}
CFZ_CALL uint32_t schedule_step(uint32_t r, uint32_t prev, uint32_t hold, uint32_t fr) { return (((r << 1) | (prev >> 31)) | (r & hold)) & fr; }

// The walk back over the rows hist[H][nw] of one vehicle, hold[nw] its hold words, g its goal sample: s[0..H-1] and the arrival, or -1
// (s unwritten) if bit g of the last row is not set.  The same for every lane: every read is of an address all lanes share.
CFZ_CALL int schedule_walk(const uint32_t *hist, int nw, const uint32_t *hold, int g, int H, uint16_t *s, bool write) {
  if (!bit_test(hist + (size_t)(H - 1) * nw, g)) return -1;
  int i = g, arrival = 0;
  if (write) s[H - 1] = (uint16_t)g;
  for (int t = H - 1; t > 0; --t) {
    const bool stay = bit_test(hist + (size_t)(t - 1) * nw, i) && bit_test(hold, i);
    if (!stay) {
      if (i == g) arrival = t;
      if (i > 0) --i;
    }
    if (write) s[t - 1] = (uint16_t)i;
  }
  return arrival;
}

// What a wavefront has seen of its orders: the smallest (makespan, total, index), makespan INT32_MAX while none, and how many were feasible.
struct ScheduleBest {
  int makespan, total, index, feasible;
};

CFZ_CALL void schedule_clear(ScheduleBest &a) { a.makespan = INT32_MAX; a.total = INT32_MAX; a.index = INT32_MAX; a.feasible = 0; }

// a minimum under a total order and an integer sum: the result does not depend on how the orders are dealt out
CFZ_CALL void schedule_merge(ScheduleBest &a, const ScheduleBest &b) {
  const bool less = b.makespan != a.makespan ? b.makespan < a.makespan : (b.total != a.total ? b.total < a.total : b.index < a.index);
  const int n = a.feasible + b.feasible;
  if (less) a = b;
  a.feasible = n;
}

// a feasible order with its arrivals' maximum and sum
CFZ_CALL void schedule_take(ScheduleBest &a, int makespan, int total, int index) {
  ScheduleBest b;
  b.makespan = makespan; b.total = total; b.index = index; b.feasible = 1;
  schedule_merge(a, b);
}

// info[kScheduleNInfo] of one set
CFZ_CALL void schedule_info(const ScheduleBest &a, int32_t *info) {
  const bool found = a.makespan != INT32_MAX;
  info[0] = found ? 1 : 0; info[1] = found ? a.index : -1; info[2] = found ? a.makespan : -1; info[3] = found ? a.total : -1;
  info[4] = a.feasible;
}

}  // namespace cfz

#endif  // CFZ_SCHEDULE_INL
