// cfz_conflict.inl -- the conflict map of a set of plans (cfz_plan_conflicts / cfz_loop_plan_conflicts): per plan set and pair of
// vehicles the clearance of their bodies along the plans, against the delay of one vehicle relative to the other.  The audit
// (cfz_audit.inl) inspects a closed loop that was run; this inspects the plans before any loop is run, and is the only place where
// the two vehicles of a pair sit at different samples of their plans.  Plain CFZ_CALL functions over audit_body / audit_signed_key, so
// that the CPU test build (tests/emu/cfz_conflict_emu.cpp) compiles the same source as conflict_kernel in cfz_engine.hip.
//
// Definitions (include/confrez_hip.h states them for the caller).  tables[P][V][T][7], rows (x, y, psi, ...); pair q = (u, w), u < w,
// in the audit's order; lag tau in [-D, D]: tau > 0, w runs tau samples late, tau < 0, u runs |tau| late.  A late vehicle waits at its
// first sample, a vehicle past its plan stays at its last.  For step i in [0, T + |tau|):
//   iu = clamp(i - max(-tau, 0), 0, T - 1), iw = clamp(i - max(tau, 0), 0, T - 1),
//   key_i = audit_signed_key(body at tables[p][u][iu][0:3], body at tables[p][w][iw][0:3]).
// Per (p, q, tau): the smallest key and the lowest step that attains it, the lowest step below the margin and the number of such steps.
// A step is below the margin when the signed distance is: key < margin^2 for disjoint bodies (key > 0), key < margin for bodies that
// touch or overlap (key <= 0); no root is taken.
//
// Layout.  The loop reads columns, not table rows: cols[P][V][4][T] holds x, y, cos psi, sin psi of every table sample as four arrays
// of T doubles per vehicle (conflict_columns in cfz_engine.hip forms them, one sincos per table sample), so that consecutive lanes,
// which take consecutive steps, read consecutive doubles, whether the columns of the pair lie in LDS or in global memory.  The
// functions have no sqrt, no division and no sin / cos; both indices are clamped, so every read is inside the columns.
#ifndef CFZ_CONFLICT_INL
#define CFZ_CONFLICT_INL

#include "cfz_audit.inl"

namespace cfz {

constexpr int kConflictNInfo = 3;     // CFZ_CONFLICT_NINFO: when, first, count
constexpr int kConflictLdsT = 1024;   // plans of up to this many samples are staged in LDS: 2 vehicles x 4 columns x 8 B = 64 B per sample

// u < w of pair q in the audit's order (0,1), (0,2), ..., (1,2), ...
CFZ_CALL void conflict_pair(int V, int q, int &u, int &w) {
  u = 0;
  while (q >= V - 1 - u) { q -= V - 1 - u; ++u; }
  w = u + 1 + q;
}
// and back: the pair index of vehicles a < b
CFZ_CALL int coord_pair_index(int V, int a, int b) { return a * (2 * V - a - 1) / 2 + (b - a - 1); }

// What one lane has seen of one (set, pair, lag).  conflict_merge is a minimum under a total order, a minimum and an integer sum, so the
// result does not depend on how the steps are dealt out or in which order the lanes are merged.
struct ConflictAcc {
  double key;  // smallest audit_signed_key (+inf: none)
  int when;    // its step, -1 while none
  int first;   // first step below the margin (INT32_MAX: none)
  int count;   // steps below the margin
};

CFZ_CALL void conflict_clear(ConflictAcc &a) { a.key = INFINITY; a.when = -1; a.first = INT32_MAX; a.count = 0; }

// (k, i) < (bk, bi) lexicographically; an entry with bi < 0 is empty, a NaN key never wins
CFZ_CALL bool conflict_less(double k, int i, double bk, int bi) {
  if (!(k == k)) return false;
  if (bi < 0) return true;
  if (k != bk) return k < bk;
  return i < bi;
}

// the signed distance that `key` stands for is below the margin (margin2 = margin * margin)
CFZ_CALL bool conflict_below(double key, double margin, double margin2) { return key > 0.0 ? key < margin2 : key < margin; }

CFZ_CALL void conflict_merge(ConflictAcc &a, const ConflictAcc &b) {
  if (b.when >= 0 && conflict_less(b.key, b.when, a.key, a.when)) { a.key = b.key; a.when = b.when; }
  if (b.first < a.first) a.first = b.first;
  a.count += b.count;
}

// Lane `lane` of `nl` over lag tau of one pair: steps lane, lane + nl, ... of [0, T + |tau|).  U, W: the columns of the two vehicles,
// x | y | cos | sin, T doubles each.
CFZ_CALL void conflict_lane(ConflictAcc &acc, int lane, int nl, int T, int tau, const double *U, const double *W, const double g[4],
                            const double il[2], double margin, double margin2) {
  conflict_clear(acc);
  const int du = tau < 0 ? -tau : 0, dw = tau > 0 ? tau : 0, n = T + du + dw;
  for (int i = lane; i < n; i += nl) {
    int iu = i - du, iw = i - dw;
    iu = iu < 0 ? 0 : (iu > T - 1 ? T - 1 : iu);
    iw = iw < 0 ? 0 : (iw > T - 1 ? T - 1 : iw);
    AuditPoly A, B;
    audit_body(g, il, U[iu], U[T + iu], U[2 * T + iu], U[3 * T + iu], A);
    audit_body(g, il, W[iw], W[T + iw], W[2 * T + iw], W[3 * T + iw], B);
    const double k = audit_signed_key(A, B);
    if (conflict_less(k, i, acc.key, acc.when)) { acc.key = k; acc.when = i; }
    if (conflict_below(k, margin, margin2)) {
      if (i < acc.first) acc.first = i;
      ++acc.count;
    }
  }
}

// the outputs of one (set, pair, lag): clear as a key (audit_key_distance makes it the signed distance), info[kConflictNInfo]
CFZ_CALL void conflict_store(const ConflictAcc &a, double *clear, int32_t *info) {
  *clear = a.key;
  info[0] = a.when; info[1] = a.first == INT32_MAX ? -1 : a.first; info[2] = a.count;
}

}  // namespace cfz

#endif  // CFZ_CONFLICT_INL
