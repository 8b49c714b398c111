// Test-only CPU build of the conflict map of a plan pool: conflict_rez_amd/csrc/cfz_conflict.inl compiled with g++ (-ffp-contract=off),
// the lanes that conflict_kernel gives a lag executed as a loop and merged by the butterfly of cfz_wave.inl.  Never shipped, never loaded by the package.
#include <vector>

#include "../../conflict_rez_amd/csrc/cfz_conflict.inl"
#include "../../conflict_rez_amd/csrc/cfz_wave.inl"
#include "emu_columns.h"

extern "C" {

int cfz_emu_conflict_lds_t(void) { return cfz::kConflictLdsT; }

// tables[P][V][T][7], g[4] the body; nl lanes per lag (a power of two up to 64); clear[P][npair][2D+1], info[P][npair][2D+1][3]
int cfz_emu_plan_conflicts(int P, int V, int T, const double *tables, const double *g, int D, double margin, int nl, double *clear,
                           int32_t *info) {
  if (P < 1 || V < 1 || V > cfz::kAuditMaxV || T < 1 || D < 0 || !(margin >= 0.0) || nl < 1 || nl > 64 || (nl & (nl - 1))) return -1;
  const int npair = V * (V - 1) / 2;
  const double il[2] = {cfz::audit_body_il(g, 0), cfz::audit_body_il(g, 1)};
  const std::vector<double> cols = emu_columns((size_t)P * V, T, tables);
  for (int p = 0; p < P; ++p)
    for (int q = 0; q < npair; ++q) {
      int u, w;
      cfz::conflict_pair(V, q, u, w);
      const double *U = cols.data() + ((size_t)p * V + u) * 4 * T, *W = cols.data() + ((size_t)p * V + w) * 4 * T;
      for (int j = 0; j < 2 * D + 1; ++j) {
        cfz::ConflictAcc acc[64];
        for (int l = 0; l < nl; ++l) cfz::conflict_lane(acc[l], l, nl, T, j - D, U, W, g, il, margin, margin * margin);
        cfz::wave_merge_host<cfz::ConflictAcc, cfz::conflict_merge>(acc, nl, nl);
        const size_t o = ((size_t)p * npair + q) * (2 * D + 1) + j;
        cfz::conflict_store(acc[0], clear + o, info + o * cfz::kConflictNInfo);
        clear[o] = cfz::audit_key_distance(clear[o]);
      }
    }
  return 0;
}
}
