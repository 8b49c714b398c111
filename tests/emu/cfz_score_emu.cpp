// Test-only CPU build of the closed-loop score: conflict_rez_amd/csrc/cfz_score.inl compiled with g++ (-ffp-contract=off), the lanes
// of score_kernel's wavefront executed as a loop and merged by the butterfly of cfz_wave.inl.  Never shipped, never loaded by the package.
#include <vector>

#include "../../conflict_rez_amd/csrc/cfz_score.inl"
#include "../../conflict_rez_amd/csrc/cfz_wave.inl"

extern "C" {

int cfz_emu_score_group(int V) { return cfz::score_group(V); }

// traj[K][S][V][7], status / iters [K][S][V] (NULL: all 0), tables[P][V][T][7], table_of[S], k0[S], g[4] the body; L lanes per vehicle
// (a power of two up to 64; 0: the kernel's grouping score_group(V)); val[S][V][10], cnt[S][V][11]
int cfz_emu_score(int K, int S, int V, const double *traj, const int32_t *status, const int32_t *iters, int P, int T, const double *tables,
                  const int32_t *table_of, const int32_t *k0, const double *g, double pos_tol, double psi_tol, double v_tol, double near,
                  int L, double *val, int32_t *cnt) {
  if (L == 0) L = cfz::score_group(V);
  if (K < 1 || S < 1 || V < 1 || V > cfz::kAuditMaxV || P < 1 || T < 1 || L < 1 || L > 64 || (L & (L - 1))) return -1;
  std::vector<double> cs((size_t)K * S * V * 2);  // as audit_headings
  for (size_t i = 0; i < (size_t)K * S * V; ++i) { cs[2 * i] = cos(traj[7 * i + 2]); cs[2 * i + 1] = sin(traj[7 * i + 2]); }
  const double il[2] = {cfz::audit_body_il(g, 0), cfz::audit_body_il(g, 1)};
  for (int s = 0; s < S; ++s) {
    if (table_of[s] < 0 || table_of[s] >= P || k0[s] < 0) return -1;
    for (int v = 0; v < V; ++v) {
      cfz::ScoreIn in;
      cfz::score_in(in, s, v, K, S, V, traj, cs.data(), status, iters, (long)S * V, T, tables, table_of, k0, 0, g, il, pos_tol, psi_tol, v_tol,
                    near * near);
      int t0[64], t1[64], arrive = INT32_MAX;
      for (int j = 0; j < L; ++j) {
        cfz::score_lane_chunk(K, L, j, t0[j], t1[j]);
        const int a = cfz::score_arrive_chunk(in, t0[j], t1[j]);
        arrive = a < arrive ? a : arrive;
      }
      if (arrive == INT32_MAX) arrive = -1;
      cfz::ScoreSeg acc[64];
      for (int j = 0; j < L; ++j) cfz::score_chunk(acc[j], in, t0[j], t1[j], arrive);
      cfz::wave_merge_ordered_host<cfz::ScoreSeg, cfz::score_merge>(acc, L, L);
      cfz::score_store(acc[0], K, arrive, val + ((size_t)s * V + v) * cfz::kScoreNVal, cnt + ((size_t)s * V + v) * cfz::kScoreNCnt);
    }
  }
  return 0;
}
}
