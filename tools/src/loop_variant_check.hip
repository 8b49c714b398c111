// loop_variant_check.hip -- host-only check of cfz_engine.hip's table of persistent kernels (no GPU needed, none touched): each of the
// 32 settings (sequential, disturbance, lossy exchange, problem pool, map pool) maps to a row of kLoopVariants whose compiled-in flags
// cover it (a map pool runs on the pool rows, alone or with a problem pool), and the ten rows are distinct kernels; prints the LDS
// bytes of the widest shape the ABI admits.
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -Xarch_host -fsanitize=address,undefined -Wno-unused-value \
//         -o tools/_bin/loop_variant_check tools/src/loop_variant_check.hip && tools/_bin/loop_variant_check
#include "../../conflict_rez_amd/csrc/cfz_engine.hip"

#include <set>

int main() {
  std::set<const void *> fns;
  for (const LoopVariant &v : kLoopVariants) fns.insert(v.fn);
  if (fns.size() != 10) { std::printf("kLoopVariants names %zu distinct kernels, not 10\n", fns.size()); return 1; }
  std::set<int> used;
  for (int m = 0; m < 32; ++m) {
    const bool seq = m & 1, dz = m & 2, cm = m & 4, pb = m & 8, mp = m & 16;
    const int i = loop_variant(seq, dz, cm, pb, mp);
    if (i < 0 || i >= 10) { std::printf("setting %d has no row\n", m); return 1; }
    const LoopVariant &v = kLoopVariants[i];
    // the exchange rule, the lossy exchange and the pool (of problems, of maps or of both) change what is computed: exact; kDist with zero
    // noise is neutral: covering
    if (v.seq != seq || v.comm != cm || v.pool != (pb || mp) || (dz && !v.dist)) { std::printf("setting %d lands on row %d, which does not cover it\n", m, i); return 1; }
    if ((cm || pb || mp) && !v.dist) { std::printf("row %d takes no disturbance argument\n", i); return 1; }
    used.insert(i);
  }
  if (used.size() != 10) { std::printf("%zu of 10 rows are reachable\n", used.size()); return 1; }
  const cfz::Lay widest = cfz::make_layout(CFZ_MAX_N, CFZ_MAX_OBS + CFZ_MAX_NBR, CFZ_MAX_NBR);
  std::printf("32 settings -> 10 rows, all reachable; widest shape (N %d, %d obstacles, %d neighbours): %zu B of LDS\n", CFZ_MAX_N, CFZ_MAX_OBS,
              CFZ_MAX_NBR, (size_t)widest.total * sizeof(double));
  return 0;
}
