// cfz_score.inl -- what a realised closed loop cost (cfz_loop_score / cfz_score): per scenario and vehicle the sums of the reference's
// own objective along the trajectory actually driven (vehicle_follower.py:263-272: tracking error, a^2, v^2 w^2, delta^2; the six
// weights of cfz_spec.weights are applied by the caller), the deviation from the plan, the time spent waiting, the changes of
// direction, the roughness of the inputs, the steps on the shift fallback (:501-524, whose back_up_steps counts the same consecutive
// failures) and the steps driven close to another body.  Plain CFZ_CALL functions, so that the CPU test build
// (tests/emu/cfz_score_emu.cpp) compiles the same source as score_kernel in cfz_engine.hip.  The audit (cfz_audit.inl) says whether a
// loop was safe; this says what it cost.
//
// Definitions (include/confrez_hip.h cites them).  For scenario s, vehicle v over a window of K recorded steps:
//   z_t = (x, y, psi, v, delta, a, w), t = 0..K-1: the state after the plant of step t and the input applied in it (cfz_loop_history),
//   with status_t and iters_t of that step's solve;
//   plan[T][7] the vehicle's plan in the set the scenario follows; k0 the clock index of the state BEFORE the window's first step;
//   r_t = plan[min(k0 + t + 1, T - 1)] the plan row of z_t.  Phase: loop_seed starts the state at plan[kidx], step t of the window
//   solves at clock k0 + t against the window plan[k0 + t + k] (prep_stage) and loop_post integrates the plant from there, so z_t is
//   the state at clock k0 + t + 1; a vehicle that follows its plan exactly has z_t = r_t.  The clamp is prep_stage's.
//   arrive = the audit's arrival (audit_arrived against the plan's last sample; first such step, -1 never);
//   upto = arrive + 1 if the vehicle arrived, else K.  EVERY quantity runs over t < upto: a parked vehicle is not charged for
//   standing at its goal, and windows of different length compare.
// val[kScoreNVal] (raw sums; the caller derives means, roots and dt x):
//   0-2  dx2, dy2, psi2     sum (x - x_r)^2, (y - y_r)^2, wrap(psi - psi_r)^2; wrap(e) = e - 2 pi rint(e (1 / 2 pi))
//   3-5  a2, vw2, delta2    sum a^2, (v w)^2, delta^2
//   6-7  da2, dw2           sum over 1 <= t < upto of (a_t - a_{t-1})^2, (w_t - w_{t-1})^2 (the predecessor is read from the record)
//   8    absv               sum |v_t|
//   9    dev2_max           max_t (x - x_r)^2 + (y - y_r)^2; ties go to the lowest step
// cnt[kScoreNCnt]:
//   0 steps = upto   1 arrive   2 failed: steps with status != 0   3 fail_run: longest run of consecutive such steps
//   4 reversals: changes of sign in the sequence of sign(v_t) over the steps with |v_t| > v_tol (a vehicle creeping around zero
//     does not count)
//   5 waiting: steps with |v_t| <= v_tol and (t < arrive or never arrived)
//   6 near_steps: steps at which the signed distance (audit_signed_key) of this body to any other body of the scenario is < near,
//     compared as key <= 0 || key < near^2 (bodies that touch count at every near)   7 first_near: the first such step, -1 none
//   8-9 iters_sum, iters_max   10 dev_max_step: the step of dev2_max
//
// Three outputs (fail_run, reversals, the floating-point sums) depend on the order of the steps, so a vehicle's steps are dealt out
// in CONTIGUOUS chunks: lane j of the vehicle's L lanes owns [j C, min((j + 1) C, K)), C = ceil(K / L), and summaries merge in order,
// the earlier segment on the left.  Apart from what audit_arrived carries the functions have no sqrt, no division and no sin / cos
// ("Record and audit"): headings' cos / sin come from audit_headings, the body's inverse edge lengths from the host.
// Every function here switches contraction off, so a * b + c is a multiplication and an addition in the device build as in the CPU
// build (-ffp-contract=off): the sums have the same bits in both.  (Inside the functions: at file scope the pragma would reach
// whatever the including file defines next.)
#ifndef CFZ_SCORE_INL
#define CFZ_SCORE_INL

#include <stddef.h>

#include "cfz_audit.inl"

#if defined(__clang__)
#define CFZ_SCORE_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CFZ_SCORE_NO_CONTRACT
#endif

namespace cfz {

constexpr int kScoreNVal = 10, kScoreNCnt = 11;  // CFZ_SCORE_NVAL, CFZ_SCORE_NCNT
constexpr int kScoreNSum = 9;                    // val[0:9] are sums, val[9] a maximum

// lanes of a 64-lane wavefront that one of V vehicles owns: the largest power of two <= 64 / V
CFZ_CALL int score_group(int V) {
  int L = 64;
  while (L * V > 64) L >>= 1;
  return L;
}

// What one lane has seen of its segment of one vehicle's steps.  score_merge is associative with score_clear as its identity, but
// not commutative: run and rv are ordered.
struct ScoreSeg {
  double sum[kScoreNSum];
  double dev2;                                 // largest squared deviation from the plan
  int dev_t;                                   // its step; -1: empty segment
  int failed, run_n, run_pre, run_suf, run_best;  // failed steps; segment length, failed prefix, failed suffix, longest failed run
  int rv_first, rv_last, rv_count;             // first / last significant sign of v (0: none in the segment), changes between them
  int waiting, near_steps, first_near;         // first_near INT32_MAX: none
  int iters_sum, iters_max;
};

CFZ_CALL void score_clear(ScoreSeg &a) {
  for (int i = 0; i < kScoreNSum; ++i) a.sum[i] = 0.0;
  a.dev2 = 0.0; a.dev_t = -1;
  a.failed = a.run_n = a.run_pre = a.run_suf = a.run_best = 0;
  a.rv_first = a.rv_last = a.rv_count = 0;
  a.waiting = a.near_steps = 0; a.first_near = INT32_MAX;
  a.iters_sum = a.iters_max = 0;
}

// a <- a followed by b (a the earlier segment)
CFZ_CALL void score_merge(ScoreSeg &a, const ScoreSeg &b) {
  CFZ_SCORE_NO_CONTRACT
  for (int i = 0; i < kScoreNSum; ++i) a.sum[i] = a.sum[i] + b.sum[i];
  if (b.dev_t >= 0 && (a.dev_t < 0 || b.dev2 > a.dev2)) { a.dev2 = b.dev2; a.dev_t = b.dev_t; }
  a.failed += b.failed;
  const int across = a.run_suf + b.run_pre;
  int best = a.run_best > b.run_best ? a.run_best : b.run_best;
  if (across > best) best = across;
  a.run_pre = a.run_pre == a.run_n ? a.run_n + b.run_pre : a.run_pre;
  a.run_suf = b.run_suf == b.run_n ? b.run_n + a.run_suf : b.run_suf;
  a.run_best = best;
  a.run_n += b.run_n;
  if (a.rv_first == 0) {
    a.rv_first = b.rv_first; a.rv_last = b.rv_last; a.rv_count = b.rv_count;
  } else if (b.rv_first != 0) {
    a.rv_count += b.rv_count + (a.rv_last != b.rv_first);
    a.rv_last = b.rv_last;
  }
  a.waiting += b.waiting;
  a.near_steps += b.near_steps;
  if (b.first_near < a.first_near) a.first_near = b.first_near;
  a.iters_sum += b.iters_sum;
  if (b.iters_max > a.iters_max) a.iters_max = b.iters_max;
}

// heading error wrapped into [-pi, pi], the quotient as a multiplication by the reciprocal
CFZ_CALL double score_wrap(double e) {
  CFZ_SCORE_NO_CONTRACT
  const double two_pi = 6.283185307179586, inv_two_pi = 0.15915494309189535;
  return e - two_pi * rint(e * inv_two_pi);
}

// One vehicle of one scenario as the functions below read it.  traj points at step 0, vehicle 0 of the scenario, consecutive steps
// step_stride doubles apart, vehicles 7 apart; cs the (cos, sin) of every heading laid out as traj with 2 doubles per vehicle (steps
// step_stride * 2 / 7 apart, as audit_lane); status / iters point at step 0 of THIS vehicle, steps si_stride apart (NULL: all 0);
// plan[T][7] this vehicle's plan, k0 the clock before the window's first step.
struct ScoreIn {
  int K, V, v, T, k0;
  const double *traj, *cs, *plan;
  long step_stride, si_stride;
  const int32_t *status, *iters;
  double g[4], il[2];
  double pos_tol, psi_tol, v_tol, near2;
};

// vehicle v of scenario s from the arrays of the whole window, as score_kernel receives them: traj[K][S][V][7] and its headings
// cs[K][S][V][2], status / iters at the window's first step with steps si_stride apart (NULL: all 0), tables[P][V][T][7], table_of[S];
// the clock before the window's first step is k0[s] - back, not below 0 (the CPU build passes back = 0)
CFZ_CALL void score_in(ScoreIn &in, int s, int v, int K, int S, int V, const double *traj, const double *cs, const int32_t *status,
                       const int32_t *iters, long si_stride, int T, const double *tables, const int32_t *table_of, const int32_t *k0,
                       int back, const double g[4], const double il[2], double pos_tol, double psi_tol, double v_tol, double near2) {
  in.K = K; in.V = V; in.v = v; in.T = T;
  in.k0 = k0[s] - back;
  if (in.k0 < 0) in.k0 = 0;
  in.traj = traj + (size_t)s * V * 7; in.cs = cs + (size_t)s * V * 2;
  in.plan = tables + ((size_t)table_of[s] * V + v) * T * 7;
  in.step_stride = (long)S * V * 7; in.si_stride = si_stride;
  in.status = status ? status + (size_t)s * V + v : nullptr;
  in.iters = iters ? iters + (size_t)s * V + v : nullptr;
  for (int i = 0; i < 4; ++i) in.g[i] = g[i];
  in.il[0] = il[0]; in.il[1] = il[1];
  in.pos_tol = pos_tol; in.psi_tol = psi_tol; in.v_tol = v_tol; in.near2 = near2;
}

CFZ_CALL const double *score_plan_row(const ScoreIn &in, int t) {
  long kr = (long)in.k0 + t + 1;
  if (kr > in.T - 1) kr = in.T - 1;
  return in.plan + kr * 7;
}

// pass 1: the first step in [t0, t1) at which the vehicle is at its goal (audit_arrived against the plan's last sample), INT32_MAX none
CFZ_CALL int score_arrive_chunk(const ScoreIn &in, int t0, int t1) {
  const double *goal = in.plan + (long)(in.T - 1) * 7;
  for (int t = t0; t < t1; ++t)
    if (audit_arrived(in.traj + t * in.step_stride + (long)in.v * 7, goal, in.pos_tol, in.psi_tol, in.v_tol)) return t;
  return INT32_MAX;
}

// pass 2: the summary of the steps [t0, min(t1, upto)); arrive -1: never
CFZ_CALL void score_chunk(ScoreSeg &a, const ScoreIn &in, int t0, int t1, int arrive) {
  CFZ_SCORE_NO_CONTRACT
  score_clear(a);
  const int upto = arrive >= 0 ? arrive + 1 : in.K;
  if (t1 > upto) t1 = upto;
  const long cs_stride = in.step_stride / 7 * 2;
  for (int t = t0; t < t1; ++t) {
    const double *z = in.traj + t * in.step_stride + (long)in.v * 7, *r = score_plan_row(in, t);
    const double dx = z[0] - r[0], dy = z[1] - r[1], dp = score_wrap(z[2] - r[2]), vw = z[3] * z[6];
    const double dx2 = dx * dx, dy2 = dy * dy;
    a.sum[0] = a.sum[0] + dx2; a.sum[1] = a.sum[1] + dy2; a.sum[2] = a.sum[2] + dp * dp;
    a.sum[3] = a.sum[3] + z[5] * z[5]; a.sum[4] = a.sum[4] + vw * vw; a.sum[5] = a.sum[5] + z[4] * z[4];
    if (t > 0) {
      const double *zp = z - in.step_stride;
      const double da = z[5] - zp[5], dw = z[6] - zp[6];
      a.sum[6] = a.sum[6] + da * da; a.sum[7] = a.sum[7] + dw * dw;
    }
    const double av = fabs(z[3]);
    a.sum[8] = a.sum[8] + av;
    const double dev2 = dx2 + dy2;
    if (a.dev_t < 0 || dev2 > a.dev2) { a.dev2 = dev2; a.dev_t = t; }
    const bool bad = in.status && in.status[t * in.si_stride] != 0;
    if (bad) {
      ++a.failed;
      if (a.run_pre == a.run_n) ++a.run_pre;
      ++a.run_suf;
      if (a.run_suf > a.run_best) a.run_best = a.run_suf;
    } else {
      a.run_suf = 0;
    }
    ++a.run_n;
    if (av > in.v_tol) {
      const int sg = z[3] > 0.0 ? 1 : -1;
      if (a.rv_first == 0) a.rv_first = sg;
      else a.rv_count += a.rv_last != sg;
      a.rv_last = sg;
    } else if (t != arrive) {
      ++a.waiting;
    }
    if (in.V > 1) {
      const double *c = in.cs + t * cs_stride + (long)in.v * 2;
      AuditPoly P, Q;
      audit_body(in.g, in.il, z[0], z[1], c[0], c[1], P);
      bool close = false;
      for (int u = 0; u < in.V; ++u) {
        if (u == in.v) continue;
        const double *zu = in.traj + t * in.step_stride + (long)u * 7, *cu = in.cs + t * cs_stride + (long)u * 2;
        audit_body(in.g, in.il, zu[0], zu[1], cu[0], cu[1], Q);
        const double key = audit_signed_key(P, Q);
        close = close || key <= 0.0 || key < in.near2;
      }
      if (close) {
        ++a.near_steps;
        if (t < a.first_near) a.first_near = t;
      }
    }
    const int it = in.iters ? in.iters[t * in.si_stride] : 0;
    a.iters_sum += it;
    if (it > a.iters_max) a.iters_max = it;
  }
}

// the chunk [t0, t1) of lane j of the L lanes of a vehicle over K steps (empty past the end)
CFZ_CALL void score_lane_chunk(int K, int L, int j, int &t0, int &t1) {
  const int C = (K + L - 1) / L;
  const long b = (long)j * C, e = b + C;
  t0 = b < K ? (int)b : K;
  t1 = e < K ? (int)e : K;
}

// the outputs of one vehicle from the merged summary of all its steps
CFZ_CALL void score_store(const ScoreSeg &a, int K, int arrive, double *val, int32_t *cnt) {
  for (int i = 0; i < kScoreNSum; ++i) val[i] = a.sum[i];
  val[9] = a.dev2;
  cnt[0] = arrive >= 0 ? arrive + 1 : K; cnt[1] = arrive;
  cnt[2] = a.failed; cnt[3] = a.run_best; cnt[4] = a.rv_count; cnt[5] = a.waiting;
  cnt[6] = a.near_steps; cnt[7] = a.first_near == INT32_MAX ? -1 : a.first_near;
  cnt[8] = a.iters_sum; cnt[9] = a.iters_max; cnt[10] = a.dev_t;
}

}  // namespace cfz

#endif  // CFZ_SCORE_INL
