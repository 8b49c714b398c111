// Test-only CPU build of the coordination diagrams and the hold-point schedules: conflict_rez_amd/csrc/cfz_coord.inl and cfz_schedule.inl
// compiled with g++ (-ffp-contract=off), the lanes of coord_kernel and schedule_kernel executed as loops, the __shfl_up carry as an index,
// the wavefronts that take the orders as a loop merged by the host form of block_merge (cfz_wave.inl).  Never shipped, never loaded by the package.
#include <vector>

#include "../../conflict_rez_amd/csrc/cfz_schedule.inl"
#include "emu_columns.h"

namespace {

// one order as schedule_order of cfz_engine.hip runs it; hist[H][nw], sched[V][H] by position, arr[2 kScheduleMaxV]
bool emu_order(int V, int T, int H, int r, uint32_t order, const uint32_t *diag, const int32_t *lens, const uint8_t *hold, uint32_t *hist,
               uint16_t *sched, int *arr, int &makespan, int &total) {
  const int nw = cfz::coord_words(T);
  makespan = 0; total = 0;
  for (int k = 0; k < V; ++k) {
    const int v = cfz::schedule_digit(order, k), len = lens[v], g = len - 1;
    uint32_t valid[64], hw[64], R[64], N[64];
    for (int l = 0; l < 64; ++l) { valid[l] = cfz::schedule_valid_word(len, l); hw[l] = cfz::schedule_hold_word(hold + (size_t)v * T, len, l); }
    for (int l = 0; l < 64; ++l) {
      R[l] = cfz::schedule_first(l, l < nw ? cfz::schedule_free_word(diag, V, T, nw, H, r, order, k, sched, 0, l, valid[l]) : 0u);
      if (l < nw) hist[l] = R[l];
    }
    for (int t = 1; t < H; ++t) {
      bool any = false;
      for (int l = 0; l < 64; ++l) {
        const uint32_t fr = l < nw ? cfz::schedule_free_word(diag, V, T, nw, H, r, order, k, sched, t, l, valid[l]) : 0u;
        N[l] = cfz::schedule_step(R[l], l ? R[l - 1] : 0u, hw[l], fr);
        any |= N[l] != 0u;
      }
      for (int l = 0; l < 64; ++l) { R[l] = N[l]; if (l < nw) hist[(size_t)t * nw + l] = R[l]; }
      if (!any) return false;  // (the kernel looks every kScheduleAhead steps: an empty row stays empty)
    }
    const int a = cfz::schedule_walk(hist, nw, hw, g, H, sched + (size_t)k * H, true);
    if (a < 0) return false;
    arr[v] = a; arr[cfz::kScheduleMaxV + v] = a - g;
    makespan = a > makespan ? a : makespan; total += a;
  }
  return true;
}

}  // namespace

extern "C" {

int cfz_emu_schedule_lds_bytes(void) { return cfz::kScheduleLdsBytes; }
int cfz_emu_schedule_wave_words(int V, int T, int H) { return (int)cfz::schedule_wave_words(V, T, H); }

// tables[P][V][T][7], length[P][V] or NULL, g[4] the body -> diag[P][npair][2][T][words], both sides as coord_kernel writes them
int cfz_emu_plan_coordination(int P, int V, int T, const double *tables, const int32_t *length, const double *g, double margin, uint32_t *diag) {
  if (P < 1 || V < 1 || V > cfz::kScheduleMaxV || T < 1 || !(margin >= 0.0) || !diag) return -1;
  const int npair = V * (V - 1) / 2, nw = cfz::coord_words(T);
  const double il[2] = {cfz::audit_body_il(g, 0), cfz::audit_body_il(g, 1)};
  const std::vector<double> cols = emu_columns((size_t)P * V, T, tables);
  for (int p = 0; p < P; ++p)
    for (int q = 0; q < npair; ++q) {
      int u, w;
      cfz::conflict_pair(V, q, u, w);
      if (cfz::coord_pair_index(V, u, w) != q) return -2;
      const double *U = cols.data() + ((size_t)p * V + u) * 4 * T, *W = cols.data() + ((size_t)p * V + w) * 4 * T;
      const int lu = length ? length[(size_t)p * V + u] : T, lw = length ? length[(size_t)p * V + w] : T;
      uint32_t *out = diag + cfz::coord_offset(npair, T, p, q, 0);
      for (int side = 0; side < 2; ++side)
        for (int row = 0; row < T; ++row)
          for (int c = 0; c * 64 < T; ++c) {
            uint64_t m = 0u;
            for (int lane = 0; lane < 64; ++lane)
              if (cfz::coord_entry(side, T, lu, lw, row, c * 64 + lane, U, W, g, il, margin, margin * margin)) m |= (uint64_t)1 << lane;
            cfz::coord_store(out + ((size_t)side * T + row) * nw, nw, c, m);
          }
    }
  return 0;
}

// diag as above (the emu's or any bitmap of that layout), hold[P][V][T], orders[O][V]; nwave wavefronts (1..4) take the orders
// wave, wave + nwave, ...; schedule[P][V][H], arrival[P][V], waits[P][V], info[P][5]
int cfz_emu_plan_schedule(int P, int V, int T, const uint32_t *diag, const int32_t *length, const uint8_t *hold, int H, int slack, int O,
                          const int32_t *orders, int nwave, int32_t *schedule, int32_t *arrival, int32_t *waits, int32_t *info) {
  if (P < 1 || V < 2 || V > cfz::kScheduleMaxV || T < 1 || T > cfz::kScheduleMaxT || H < T || H > cfz::kScheduleMaxH || slack < 0 || O < 1 ||
      nwave < 1 || nwave > 4 || !diag || !hold || !orders)
    return -1;
  for (int o = 0; o < O; ++o)
    if (!cfz::schedule_is_permutation(V, orders + (size_t)o * V)) return -1;
  const int npair = V * (V - 1) / 2, nw = cfz::coord_words(T);
  std::vector<uint32_t> hist((size_t)H * nw);
  std::vector<uint16_t> sched((size_t)V * H);
  for (int p = 0; p < P; ++p) {
    int32_t lens[cfz::kScheduleMaxV];
    for (int v = 0; v < V; ++v) {
      lens[v] = length ? length[(size_t)p * V + v] : T;
      if (lens[v] < 1 || lens[v] > T) return -1;
    }
    const uint32_t *dg = diag + cfz::coord_offset(npair, T, p, 0, 0);
    const uint8_t *hd = hold + (size_t)p * V * T;
    int arr[2 * cfz::kScheduleMaxV], mk, tot;
    cfz::ScheduleBest best[4], all;
    for (int w = 0; w < nwave; ++w) {
      cfz::schedule_clear(best[w]);
      for (int o = w; o < O; o += nwave)
        if (emu_order(V, T, H, slack, cfz::schedule_pack(V, orders + (size_t)o * V), dg, lens, hd, hist.data(), sched.data(), arr, mk, tot))
          cfz::schedule_take(best[w], mk, tot, o);
    }
    cfz::schedule_clear(all);
    cfz::block_merge_host<cfz::ScheduleBest, cfz::schedule_merge>(all, best, nwave);
    int32_t *s = schedule + (size_t)p * V * H;
    if (all.makespan != INT32_MAX) {
      const uint32_t order = cfz::schedule_pack(V, orders + (size_t)all.index * V);
      if (!emu_order(V, T, H, slack, order, dg, lens, hd, hist.data(), sched.data(), arr, mk, tot)) return -3;
      for (int k = 0; k < V; ++k)
        for (int t = 0; t < H; ++t) s[(size_t)cfz::schedule_digit(order, k) * H + t] = sched[(size_t)k * H + t];
      for (int v = 0; v < V; ++v) { arrival[(size_t)p * V + v] = arr[v]; waits[(size_t)p * V + v] = arr[cfz::kScheduleMaxV + v]; }
    } else {
      for (int i = 0; i < V * H; ++i) s[i] = -1;
      for (int v = 0; v < V; ++v) arrival[(size_t)p * V + v] = waits[(size_t)p * V + v] = -1;
    }
    cfz::schedule_info(all, info + (size_t)p * cfz::kScheduleNInfo);
  }
  return 0;
}
}
