// cfz_audit.inl -- geometry and bookkeeping of the realised-trajectory audit (cfz_loop_audit / cfz_audit): signed distances of the
// bodies to each other and to the static obstacles along a recorded closed loop, first contact and arrival of every scenario.
// Plain CFZ_CALL functions, so that the CPU test build (tests/emu/cfz_audit_emu.cpp) compiles the same source as audit_kernel in
// cfz_engine.hip.  The reference keeps the same trajectory per vehicle (`final_traj`, vehicle_follower.py:74-82, :556-563) and
// leaves its inspection to the user.
//
// Signed distance of two convex polygons P, Q (four vertices each, either orientation):
//   disjoint:          their Euclidean distance (the smallest vertex-to-edge distance of the two boundaries);
//   touching/overlap:  minus the penetration depth, min over the face normals n of both polygons of
//                      min(max P.n - min Q.n, max Q.n - min P.n) (the shortest translation along n that separates them), 0 when
//                      they only touch.
// By the separating-axis theorem the polygons are disjoint exactly when that overlap is negative along some face normal.
#ifndef CFZ_AUDIT_INL
#define CFZ_AUDIT_INL

#include <math.h>
#include <stdint.h>

#ifndef CFZ_CALL
#if defined(__HIPCC__)
#define CFZ_CALL __host__ __device__ __forceinline__
#else
#define CFZ_CALL static inline
#endif
#endif

namespace cfz {

constexpr int kAuditMaxV = 8;  // CFZ_MAX_NBR + 1

// A convex quadrilateral as the audit's inner loop reads it: vertices in order around it, the unit normals of its faces (opposite
// faces of a rectangle share one: nn = 2) and the inverse length of every edge (0 for a degenerate one).  Normals and inverse lengths
// are formed where sqrt and division are cheap and exact to the last bit (the host; from the pose's cos / sin for a body), so that
// the loop over (step, item) pairs is multiplications, additions and comparisons only.
struct AuditPoly {
  double v[4][2], n[4][2], il[4];
  int nn;
};

// normals and inverse edge lengths of a polygon whose vertices are set (host side and CPU build)
CFZ_CALL void audit_poly_prepare(AuditPoly &P) {
  for (int e = 0; e < 4; ++e) {
    const double ex = P.v[(e + 1) & 3][0] - P.v[e][0], ey = P.v[(e + 1) & 3][1] - P.v[e][1], len = sqrt(ex * ex + ey * ey);
    P.il[e] = len > 0.0 ? 1.0 / len : 0.0;
    P.n[e][0] = ey * P.il[e]; P.n[e][1] = -ex * P.il[e];
  }
  P.nn = 4;
}

// il[e] of the body g = (front, left, rear, right): the inverse length of its long (e = 0) or short (e = 1) edges.  Formed on the host,
// by every launcher and every CPU build through this one function
CFZ_CALL double audit_body_il(const double g[4], int e) { return 1.0 / (g[e] + g[e + 2]); }

// the body rectangle g at (x, y) with heading cos c, sin s, corners counter-clockwise (as dual_ws_kernel); il[2] as audit_body_il
CFZ_CALL void audit_body(const double g[4], const double il[2], double x, double y, double c, double s, AuditPoly &W) {
  const double BV[4][2] = {{g[0], g[1]}, {-g[2], g[1]}, {-g[2], -g[3]}, {g[0], -g[3]}};
  for (int i = 0; i < 4; ++i) { W.v[i][0] = x + c * BV[i][0] - s * BV[i][1]; W.v[i][1] = y + s * BV[i][0] + c * BV[i][1]; }
  W.n[0][0] = c; W.n[0][1] = s; W.n[1][0] = -s; W.n[1][1] = c;
  W.il[0] = il[0]; W.il[1] = il[1]; W.il[2] = il[0]; W.il[3] = il[1];
  W.nn = 2;
}

// smallest squared distance of a vertex of A to an edge of B: the perpendicular foot where it falls inside the edge
// (|cross| / |e|), else the nearer end point
CFZ_CALL double audit_vertex_edge2(const AuditPoly &A, const AuditPoly &B) {
  double best = INFINITY;
  for (int e = 0; e < 4; ++e) {
    const double ax = B.v[e][0], ay = B.v[e][1], ex = B.v[(e + 1) & 3][0] - ax, ey = B.v[(e + 1) & 3][1] - ay;
    const double ee = ex * ex + ey * ey;
    for (int v = 0; v < 4; ++v) {
      const double wx = A.v[v][0] - ax, wy = A.v[v][1] - ay, we = wx * ex + wy * ey;
      double d2;
      if (we <= 0.0) {
        d2 = wx * wx + wy * wy;
      } else if (we >= ee) {
        const double ux = wx - ex, uy = wy - ey;
        d2 = ux * ux + uy * uy;
      } else {
        const double h = (wx * ey - wy * ex) * B.il[e];
        d2 = h * h;
      }
      if (d2 < best) best = d2;
    }
  }
  return best;
}

// the smallest overlap of the projections of P and Q over the face normals of A (negative: A has a separating face)
CFZ_CALL double audit_face_overlap(const AuditPoly &A, const AuditPoly &P, const AuditPoly &Q) {
  double best = INFINITY;
  for (int e = 0; e < A.nn; ++e) {
    const double nx = A.n[e][0], ny = A.n[e][1];
    if (nx == 0.0 && ny == 0.0) continue;
    double p0 = INFINITY, p1 = -INFINITY, q0 = INFINITY, q1 = -INFINITY;
    for (int v = 0; v < 4; ++v) {
      const double hp = P.v[v][0] * nx + P.v[v][1] * ny, hq = Q.v[v][0] * nx + Q.v[v][1] * ny;
      p0 = hp < p0 ? hp : p0; p1 = hp > p1 ? hp : p1; q0 = hq < q0 ? hq : q0; q1 = hq > q1 ? hq : q1;
    }
    const double o = (p1 - q0) < (q1 - p0) ? (p1 - q0) : (q1 - p0);
    if (o < best) best = o;
  }
  return best;
}

// what the audit minimises: the squared distance if the polygons are disjoint, else minus the penetration depth (0 when they only
// touch).  Monotone in the signed distance, so minima and ties are those of the signed distance; audit_key_distance converts.
CFZ_CALL double audit_signed_key(const AuditPoly &P, const AuditPoly &Q) {
  const double op = audit_face_overlap(P, P, Q), oq = audit_face_overlap(Q, P, Q);
  const double o = op < oq ? op : oq;
  if (o >= 0.0) return o > 0.0 ? -o : 0.0;
  const double a = audit_vertex_edge2(P, Q), b = audit_vertex_edge2(Q, P);
  return a < b ? a : b;
}

CFZ_CALL double audit_key_distance(double k) { return k > 0.0 ? sqrt(k) : k; }

// heading error wrapped into [-pi, pi]
CFZ_CALL double audit_wrap(double e) {
  const double two_pi = 6.283185307179586;
  return e - two_pi * rint(e / two_pi);
}

// record z = (x, y, psi, v, delta, a, w) at the goal (x, y, psi) within the tolerances
CFZ_CALL bool audit_arrived(const double *z, const double *goal, double pos_tol, double psi_tol, double v_tol) {
  const double dx = z[0] - goal[0], dy = z[1] - goal[1];
  return dx * dx + dy * dy <= pos_tol * pos_tol && fabs(audit_wrap(z[2] - goal[2])) <= psi_tol && fabs(z[3]) <= v_tol;
}

// What one lane has seen of one scenario; merged over the lanes (audit_merge is a minimum under a total order, so the result does
// not depend on how the items are dealt out or in which order the lanes are merged).
struct AuditAcc {
  double vv, vo;          // smallest vehicle-vehicle / vehicle-obstacle audit_signed_key (+inf: none)
  int vv_t, vv_u, vv_w;   // its (step, u, w), u < w; -1 while none
  int vo_t, vo_v, vo_j;   // its (step, vehicle, obstacle)
  int first;              // first step with a negative signed distance (INT32_MAX: none)
  int arrive[kAuditMaxV]; // first step at the goal per vehicle (INT32_MAX: none)
};

CFZ_CALL void audit_clear(AuditAcc &a) {
  a.vv = INFINITY; a.vo = INFINITY;
  a.vv_t = a.vv_u = a.vv_w = -1; a.vo_t = a.vo_v = a.vo_j = -1;
  a.first = INT32_MAX;
  for (int v = 0; v < kAuditMaxV; ++v) a.arrive[v] = INT32_MAX;
}

// (d, t, i, j) < (bd, bt, bi, bj) lexicographically; an entry with bt < 0 is empty, NaN distances never win
CFZ_CALL bool audit_less(double d, int t, int i, int j, double bd, int bt, int bi, int bj) {
  if (!(d == d)) return false;
  if (bt < 0) return true;
  if (d != bd) return d < bd;
  if (t != bt) return t < bt;
  if (i != bi) return i < bi;
  return j < bj;
}

CFZ_CALL void audit_merge(AuditAcc &a, const AuditAcc &b) {
  if (b.vv_t >= 0 && audit_less(b.vv, b.vv_t, b.vv_u, b.vv_w, a.vv, a.vv_t, a.vv_u, a.vv_w)) { a.vv = b.vv; a.vv_t = b.vv_t; a.vv_u = b.vv_u; a.vv_w = b.vv_w; }
  if (b.vo_t >= 0 && audit_less(b.vo, b.vo_t, b.vo_v, b.vo_j, a.vo, a.vo_t, a.vo_v, a.vo_j)) { a.vo = b.vo; a.vo_t = b.vo_t; a.vo_v = b.vo_v; a.vo_j = b.vo_j; }
  if (b.first < a.first) a.first = b.first;
  for (int v = 0; v < kAuditMaxV; ++v) if (b.arrive[v] < a.arrive[v]) a.arrive[v] = b.arrive[v];
}

// Lane `lane` of `nl` over one scenario's record: traj points at step 0, vehicle 0 of the scenario, consecutive steps `step_stride`
// doubles apart, vehicles 7 apart; cs the (cos, sin) of every heading, laid out as traj with 2 doubles per vehicle (steps
// step_stride * 2 / 7 apart); goal [V][3]; obs [n_obs] the obstacles.  Items: (step, pair u < w), then
// (step, vehicle, obstacle), then (step, vehicle) for the arrivals, all dealt out round-robin.
CFZ_CALL void audit_lane(AuditAcc &acc, int lane, int nl, int K, int V, const double *traj, long step_stride, const double *goal,
                         const double *cs, int n_obs, const AuditPoly *obs, const double g[4], const double il[2], double pos_tol,
                         double psi_tol, double v_tol) {
  const long cs_stride = step_stride / 7 * 2;
  audit_clear(acc);
  const int npair = V * (V - 1) / 2;
  for (long i = lane; i < (long)K * npair; i += nl) {
    const int t = (int)(i / npair);
    int p = (int)(i - (long)t * npair), u = 0;
    while (p >= V - 1 - u) { p -= V - 1 - u; ++u; }
    const int w = u + 1 + p;
    const double *zu = traj + t * step_stride + (long)u * 7, *zw = traj + t * step_stride + (long)w * 7;
    const double *cu = cs + t * cs_stride + (long)u * 2, *cw = cs + t * cs_stride + (long)w * 2;
    AuditPoly P, Q;
    audit_body(g, il, zu[0], zu[1], cu[0], cu[1], P); audit_body(g, il, zw[0], zw[1], cw[0], cw[1], Q);
    const double d = audit_signed_key(P, Q);
    if (audit_less(d, t, u, w, acc.vv, acc.vv_t, acc.vv_u, acc.vv_w)) { acc.vv = d; acc.vv_t = t; acc.vv_u = u; acc.vv_w = w; }
    if (d < 0.0 && t < acc.first) acc.first = t;
  }
  const int nvo = V * n_obs;
  for (long i = lane; i < (long)K * nvo; i += nl) {
    const int t = (int)(i / nvo), r = (int)(i - (long)t * nvo), v = r / n_obs, j = r - v * n_obs;
    const double *z = traj + t * step_stride + (long)v * 7;
    const double *c = cs + t * cs_stride + (long)v * 2;
    AuditPoly P;
    audit_body(g, il, z[0], z[1], c[0], c[1], P);
    const double d = audit_signed_key(P, obs[j]);
    if (audit_less(d, t, v, j, acc.vo, acc.vo_t, acc.vo_v, acc.vo_j)) { acc.vo = d; acc.vo_t = t; acc.vo_v = v; acc.vo_j = j; }
    if (d < 0.0 && t < acc.first) acc.first = t;
  }
  for (long i = lane; i < (long)K * V; i += nl) {
    const int t = (int)(i / V), v = (int)(i - (long)t * V);
    if (t < acc.arrive[v] && audit_arrived(traj + t * step_stride + (long)v * 7, goal + 3 * v, pos_tol, psi_tol, v_tol)) acc.arrive[v] = t;
  }
}

// the outputs of one scenario: clear[2] (as keys: audit_key_distance makes them signed distances), where[6], first_contact,
// arrive[V] (steps relative to the audited window)
CFZ_CALL void audit_store(const AuditAcc &a, int V, double *clear, int32_t *where, int32_t *first_contact, int32_t *arrive) {
  clear[0] = a.vv; clear[1] = a.vo;
  where[0] = a.vv_t; where[1] = a.vv_u; where[2] = a.vv_w; where[3] = a.vo_t; where[4] = a.vo_v; where[5] = a.vo_j;
  *first_contact = a.first == INT32_MAX ? -1 : a.first;
  for (int v = 0; v < V; ++v) arrive[v] = a.arrive[v] == INT32_MAX ? -1 : a.arrive[v];
}

}  // namespace cfz

#endif  // CFZ_AUDIT_INL
