// cfz_coord.inl -- the coordination diagrams of a set of plans (cfz_plan_coordination, and the input of cfz_schedule.inl): per plan set
// and pair of vehicles the T x T bitmap that says which sample of the one plan is too close to which sample of the other.  The conflict
// map (cfz_conflict.inl) holds the sums of its diagonals; a schedule that lets a vehicle wait in the middle of its plan leaves the
// diagonals, so it needs the diagram itself.  Plain CFZ_CALL functions over audit_body / audit_signed_key / conflict_below, so that the
// CPU test build (tests/emu/cfz_schedule_emu.cpp) compiles the same source as coord_kernel in cfz_engine.hip.
//
// Definitions (include/confrez_hip.h states them for the caller).  Pair q = (u, w), u < w, in the audit's order; length[v] in [1, T]:
//   B_q[i][j] = conflict_below(audit_signed_key(body of u at sample i, body of w at sample j), margin, margin^2), i < length[u], j < length[w]
// and 0 elsewhere.  u's body is the first argument everywhere.
//
// Layout.  Rows of coord_words(T) 32-bit words, bit (c & 31) of word (c >> 5) for column c; every pair has both orientations:
//   side 0: row i (u's sample), column j (w's sample);   side 1: row j (w's sample), column i (u's sample)
// as diag[P][npair][2][T][words].  Side 1 is not a transposition of stored bits: it evaluates the same audit_signed_key(u's body, w's
// body) with the columns over i, so the two sides agree bit for bit by construction.  The bodies are read from the columns of
// conflict_columns (cols[P][V][4][T]: x, y, cos psi, sin psi); every index is clamped before it is read.
#ifndef CFZ_COORD_INL
#define CFZ_COORD_INL

#include "cfz_conflict.inl"
#include "cfz_wave.inl"  // bit_words, bit_test

namespace cfz {

CFZ_CALL int coord_words(int T) { return bit_words(T); }

// where the rows of (set p, pair q, side) begin in diag, in words
CFZ_CALL size_t coord_offset(int npair, int T, int p, int q, int side) {
  return (((size_t)p * npair + q) * 2 + side) * (size_t)T * coord_words(T);
}

// B_q[i][j]: u at its sample i, w at its sample j; lu, lw their lengths.  i, j may lie anywhere: outside the lengths the entry is 0.
CFZ_CALL bool coord_blocked(int T, int lu, int lw, int i, int j, const double *U, const double *W, const double g[4], const double il[2],
                            double margin, double margin2) {
  if (i < 0 || j < 0 || i >= lu || j >= lw) return false;
  const int ic = i > T - 1 ? T - 1 : i, jc = j > T - 1 ? T - 1 : j;  // (lu, lw <= T: never taken; the reads stay inside whatever the caller says)
  AuditPoly A, B;
  audit_body(g, il, U[ic], U[T + ic], U[2 * T + ic], U[3 * T + ic], A);
  audit_body(g, il, W[jc], W[T + jc], W[2 * T + jc], W[3 * T + jc], B);
  return conflict_below(audit_signed_key(A, B), margin, margin2);
}

// the entry at (row, col) of a side
CFZ_CALL bool coord_entry(int side, int T, int lu, int lw, int row, int col, const double *U, const double *W, const double g[4],
                          const double il[2], double margin, double margin2) {
  return side ? coord_blocked(T, lu, lw, col, row, U, W, g, il, margin, margin2) : coord_blocked(T, lu, lw, row, col, U, W, g, il, margin, margin2);
}

// the 64 predicates of columns 64 c .. 64 c + 63 of a row (a wavefront's ballot) into the row's words
CFZ_CALL void coord_store(uint32_t *row, int nw, int c, uint64_t ballot) {
  row[2 * c] = (uint32_t)ballot;
  if (2 * c + 1 < nw) row[2 * c + 1] = (uint32_t)(ballot >> 32);
}

}  // namespace cfz

#endif  // CFZ_COORD_INL
