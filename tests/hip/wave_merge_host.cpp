// Test-only g++ build of the host forms of conflict_rez_amd/csrc/cfz_wave.inl over the accumulators of wave_merge_case.h
// (tests/test_wave_merge_gpu.py).  Never shipped, never loaded by the package.
#include "../../conflict_rez_amd/csrc/cfz_wave.inl"
#include "wave_merge_case.h"

extern "C" {

// acc[nl] in place, in groups of `width` lanes (a power of two that divides nl)
int wave_host_min(WaveCase *acc, int nl, int width) {
  if (nl < 1 || width < 1 || (width & (width - 1)) || nl % width) return -1;
  cfz::wave_merge_host<WaveCase, case_min>(acc, nl, width);
  return 0;
}

int wave_host_concat(WaveSpan *acc, int nl, int width) {
  if (nl < 1 || width < 1 || (width & (width - 1)) || nl % width) return -1;
  cfz::wave_merge_ordered_host<WaveSpan, span_concat>(acc, nl, width);
  return 0;
}
}
