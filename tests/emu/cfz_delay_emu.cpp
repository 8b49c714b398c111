// Test-only CPU build of the delay search over a conflict map (conflict_rez_amd/csrc/cfz_delay.inl with g++): delay_kernel's lanes as a loop,
// merged as there by wave_merge_host per min(nl, 64) lanes, then block_merge_host.  Never shipped, never loaded by the package.
#include <algorithm>
#include <vector>

#include "../../conflict_rez_amd/csrc/cfz_delay.inl"
#include "../../conflict_rez_amd/csrc/cfz_wave.inl"

extern "C" {

// count[P][npair][2D+1], clear likewise or NULL, cap[P][V] or NULL; nl lanes per set (a power of two up to 256);
// delays[P][V], info[P][3], rclear[P] (written only where clear is given)
int cfz_emu_delay_search(int P, int V, int D, const int32_t *count, const double *clear, int slack, const int32_t *cap, int nl,
                         int32_t *delays, int32_t *info, double *rclear) {
  if (P < 1 || V < 1 || V > cfz::kDelayMaxV || D < 0 || slack < 0 || !count || !delays || !info || nl < 1 || nl > 256 || (nl & (nl - 1))) return -1;
  double box = 1.0;
  for (int v = 0; v < V; ++v) box *= D + 1.0;
  if (box > 2147483648.0) return -1;
  const int npair = V * (V - 1) / 2, L = 2 * D + 1, nw = cfz::delay_words(D), width = std::min(nl, 64);
  std::vector<uint32_t> mask((size_t)(npair ? npair : 1) * nw);
  std::vector<cfz::DelayAcc> acc(nl);
  for (int p = 0; p < P; ++p) {
    const int32_t *cnt = count + (size_t)p * npair * L;
    const double *clr = clear ? clear + (size_t)p * npair * L : nullptr;
    for (auto &w : mask) w = 0u;
    for (int q = 0; q < npair; ++q)
      for (int j = 0; j < L; ++j)
        if (cfz::delay_window_free(cnt + (size_t)q * L, 1, clr ? clr + (size_t)q * L : nullptr, D, slack, j)) mask[q * nw + (j >> 5)] |= 1u << (j & 31);
    for (int v = 0; v < V && cap; ++v)
      if (cap[(size_t)p * V + v] < 0 || cap[(size_t)p * V + v] > D) return -1;
    cfz::DelayVec capv;
    cfz::delay_pack(V, cap ? cap + (size_t)p * V : nullptr, D, capv);
    int maxcap = 0;
    for (int v = 0; v < V; ++v) maxcap = std::max(maxcap, cfz::delay_digit(capv, v));
    cfz::DelayAcc best;
    cfz::delay_clear(best);
    int m = 0;
    for (; m <= maxcap; ++m) {
      cfz::DelayShell sh;
      cfz::delay_shell(V, m, sh);
      for (int l = 0; l < nl; ++l) cfz::delay_lane(acc[l], l, nl, V, D, m, sh, capv, mask.data(), nw);
      cfz::wave_merge_host<cfz::DelayAcc, cfz::delay_merge>(acc.data(), nl, width);
      cfz::block_merge_host<cfz::DelayAcc, cfz::delay_merge>(best, acc.data(), nl / width, width);
      if (best.total != INT32_MAX) break;
    }
    cfz::delay_store(best, V, D, m, clr, delays + (size_t)p * V, info + (size_t)p * cfz::kDelayNInfo, rclear ? rclear + p : nullptr);
  }
  return 0;
}
}
