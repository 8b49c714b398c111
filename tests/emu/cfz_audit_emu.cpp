// Test-only CPU build of the audit's geometry and bookkeeping: conflict_rez_amd/csrc/cfz_audit.inl compiled with g++, the lanes
// of audit_kernel's wavefront executed as a loop and merged by the butterfly of cfz_wave.inl.  Never shipped, never loaded by the package.
#include <string.h>

#include <vector>

#include "../../conflict_rez_amd/csrc/cfz_audit.inl"
#include "../../conflict_rez_amd/csrc/cfz_wave.inl"

extern "C" {

static cfz::AuditPoly poly(const double *V) {
  cfz::AuditPoly P;
  memcpy(P.v, V, sizeof P.v);
  cfz::audit_poly_prepare(P);
  return P;
}

double cfz_emu_signed_distance(const double *P, const double *Q) {
  return cfz::audit_key_distance(cfz::audit_signed_key(poly(P), poly(Q)));
}

// traj[K][S][V][7], goal[S][V][3], obs[n_obs][4][2]; nl lanes per scenario (a power of 2)
int cfz_emu_audit(int K, int S, int V, const double *traj, const double *goal, int n_obs, const double *obs, const double *g,
                  double pos_tol, double psi_tol, double v_tol, int nl, double *clear, int32_t *where, int32_t *first_contact,
                  int32_t *arrive) {
  if (V < 1 || V > cfz::kAuditMaxV || nl < 1 || nl > 64 || (nl & (nl - 1))) return -1;
  std::vector<cfz::AuditPoly> ob((size_t)(n_obs > 0 ? n_obs : 1));
  for (int j = 0; j < n_obs; ++j) ob[j] = poly(obs + (long)j * 8);
  const double il[2] = {cfz::audit_body_il(g, 0), cfz::audit_body_il(g, 1)};
  std::vector<double> cs((size_t)K * S * V * 2);  // as audit_headings
  for (size_t i = 0; i < (size_t)K * S * V; ++i) { cs[2 * i] = cos(traj[7 * i + 2]); cs[2 * i + 1] = sin(traj[7 * i + 2]); }
  cfz::AuditAcc acc[64];
  for (int s = 0; s < S; ++s) {
    for (int l = 0; l < nl; ++l)
      cfz::audit_lane(acc[l], l, nl, K, V, traj + (long)s * V * 7, (long)S * V * 7, goal + (long)s * V * 3, cs.data() + (long)s * V * 2, n_obs, ob.data(), g, il,
                      pos_tol, psi_tol, v_tol);
    cfz::wave_merge_host<cfz::AuditAcc, cfz::audit_merge>(acc, nl, nl);
    cfz::audit_store(acc[0], V, clear + (long)s * 2, where + (long)s * 6, first_contact + s, arrive + (long)s * V);
    for (int i = 0; i < 2; ++i) clear[s * 2 + i] = cfz::audit_key_distance(clear[s * 2 + i]);
  }
  return 0;
}
}
