// Test-only g++ build of the host forms of conflict_rez_amd/csrc/cfz_wave.inl over the accumulators of wave_merge_case.h
// (tests/test_wave_merge_gpu.py, tests/test_block_merge_gpu.py).  Never shipped, never loaded by the package.
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

// the workgroup merge of acc[rounds][waves], one wavefront's accumulator each -> out[rounds]
int block_host_min(const WaveCase *acc, int rounds, int waves, WaveCase *out) {
  if (rounds < 1 || waves < 1) return -1;
  for (int r = 0; r < rounds; ++r) { case_clear(out[r]); cfz::block_merge_host<WaveCase, case_min>(out[r], acc + r * waves, waves); }
  return 0;
}

int block_host_sum(const WaveSum *acc, int rounds, int waves, WaveSum *out) {
  if (rounds < 1 || waves < 1) return -1;
  for (int r = 0; r < rounds; ++r) { sum_clear(out[r]); cfz::block_merge_host<WaveSum, sum_add>(out[r], acc + r * waves, waves); }
  return 0;
}
}
