// Test-only CPU build of the planning solver source (conflict_rez_amd/csrc/cfz_plan.inl), see cfz_emu.cpp.
#include <stdlib.h>

#include "../../conflict_rez_amd/csrc/cfz_plan.inl"

extern "C" {
int cfzp_emu_sizeof_spec(void) { return (int)sizeof(cfzp::PSpec); }
int cfzp_emu_n(const cfzp::PSpec *sp) { return cfzp::dims(*sp).n; }
int cfzp_emu_state_ws(const cfzp::PSpec *sp, const double *tube, double *X, int *out_i, double *out_d) {
  double *slab = (double *)calloc(cfzp::work_doubles(*sp), sizeof(double));
  if (!slab) return -1;
  cfzp::solve_state_ws<false>(*sp, tube, X, slab, out_i, out_d);
  free(slab);
  return 0;
}

// The backward sweep ALONE (tests/test_sweeps_host.py; oracle/sweeps.py) on the caller's stage data st [(T + 1) kSt]; fb [(T + 1) kFb] and
// vf [(T + 1) kVf] are written for the stages the sweep visits; -> its flag.
// The plain loops of the homogeneous form; built with -DCFZP_DENSE_TRANSPOSED they take the accumulator as the matrix-core sweep does.
int cfzp_emu_riccati_dense(int T, double dt, int has_final, double *st, double *fb, double *vf) {
  cfzp::PSpec sp = {};
  sp.T = T; sp.dt = dt; sp.has_final = has_final;
  cfzp::PWork w = {};
  w.vf = vf;
  return cfzp::riccati_backward_dense(sp, w, st, fb);
}
// The one-lane sweep; ce [n_chk 6]: the pose blocks of the cell ends, stages N, 2 N, .. n_chk N = T.
int cfzp_emu_riccati(int T, int N, int n_chk, double dt, int has_final, double *st, double *ce, double *fb, double *vf) {
  cfzp::PSpec sp = {};
  sp.T = T; sp.N = N; sp.n_chk = n_chk; sp.dt = dt; sp.has_final = has_final;
  cfzp::PWork w = {};
  w.vf = vf; w.ce = ce;
  return cfzp::riccati_backward(sp, w, st, fb);
}
}
