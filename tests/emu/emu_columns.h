// Test-only: the columns that conflict_columns of cfz_engine.hip forms, for the CPU builds of the kernels that read them.
// tables[n][T][7] -> cols[n][4][T]: x, y, cos psi, sin psi.
#pragma once
#include <math.h>
#include <vector>

static inline std::vector<double> emu_columns(size_t n, int T, const double *tables) {
  std::vector<double> cols(n * 4 * T);
  for (size_t i = 0; i < n * T; ++i) {
    const double *z = tables + i * 7;
    double *col = cols.data() + i / T * 4 * T + i % T;
    col[0] = z[0]; col[T] = z[1]; col[2 * (size_t)T] = cos(z[2]); col[3 * (size_t)T] = sin(z[2]);
  }
  return cols;
}
