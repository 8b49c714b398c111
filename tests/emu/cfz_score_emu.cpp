// Test-only CPU build of the closed-loop score: conflict_rez_amd/csrc/cfz_score.inl compiled with g++ (-ffp-contract=off), the lanes
// of score_kernel's wavefront executed as a loop and merged as its butterfly does.  Never shipped, never loaded by the package.
#include <vector>

#include "../../conflict_rez_amd/csrc/cfz_score.inl"

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
  for (int s = 0; s < S; ++s) {
    if (table_of[s] < 0 || table_of[s] >= P || k0[s] < 0) return -1;
    for (int v = 0; v < V; ++v) {
      cfz::ScoreIn in;
      in.K = K; in.V = V; in.v = v; in.T = T; in.k0 = k0[s];
      in.traj = traj + (size_t)s * V * 7; in.cs = cs.data() + (size_t)s * V * 2;
      in.plan = tables + ((size_t)table_of[s] * V + v) * T * 7;
      in.step_stride = (long)S * V * 7; in.si_stride = (long)S * V;
      in.status = status ? status + (size_t)s * V + v : nullptr;
      in.iters = iters ? iters + (size_t)s * V + v : nullptr;
      for (int i = 0; i < 4; ++i) in.g[i] = g[i];
      in.il[0] = 1.0 / (g[0] + g[2]); in.il[1] = 1.0 / (g[1] + g[3]);  // as cfz_engine.hip's score_launch
      in.pos_tol = pos_tol; in.psi_tol = psi_tol; in.v_tol = v_tol; in.near2 = near * near;
      int t0[64], t1[64], arrive = INT32_MAX;
      for (int j = 0; j < L; ++j) {
        cfz::score_lane_chunk(K, L, j, t0[j], t1[j]);
        const int a = cfz::score_arrive_chunk(in, t0[j], t1[j]);
        arrive = a < arrive ? a : arrive;
      }
      if (arrive == INT32_MAX) arrive = -1;
      cfz::ScoreSeg acc[64], nxt[64];
      for (int j = 0; j < L; ++j) cfz::score_chunk(acc[j], in, t0[j], t1[j], arrive);
      for (int off = 1; off < L; off <<= 1) {
        for (int j = 0; j < L; ++j) {
          if (j & off) { nxt[j] = acc[j ^ off]; cfz::score_merge(nxt[j], acc[j]); }  // the lower lane is the left operand
          else { nxt[j] = acc[j]; cfz::score_merge(nxt[j], acc[j ^ off]); }
        }
        for (int j = 0; j < L; ++j) acc[j] = nxt[j];
      }
      cfz::score_store(acc[0], K, arrive, val + ((size_t)s * V + v) * cfz::kScoreNVal, cnt + ((size_t)s * V + v) * cfz::kScoreNCnt);
    }
  }
  return 0;
}
}
