// The accumulators and merges of tests/test_wave_merge_gpu.py and tests/test_block_merge_gpu.py, shared by the device programs
// (tests/hip/wave_merge.hip, block_merge.hip) and the g++ build of the host forms (tests/hip/wave_merge_host.cpp).  Nothing of the product but cfz_wave.inl is involved.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define WAVE_CASE_CALL __host__ __device__ __forceinline__
#else
#define WAVE_CASE_CALL static inline
#endif

// 32 bytes: a at 0, a padding word at 4, x at 8, b at 16, a padding word at 28
struct WaveCase {
  int a;
  double x;
  int b[3];
};
static_assert(sizeof(WaveCase) == 32, "the test relies on the padding words");

// the lexicographic minimum over (x, a, b[0], b[1], b[2]): commutative
WAVE_CASE_CALL void case_min(WaveCase &p, const WaveCase &q) {
  bool less = false;
  if (q.x != p.x) less = q.x < p.x;
  else if (q.a != p.a) less = q.a < p.a;
  else if (q.b[0] != p.b[0]) less = q.b[0] < p.b[0];
  else if (q.b[1] != p.b[1]) less = q.b[1] < p.b[1];
  else less = q.b[2] < p.b[2];
  if (less) p = q;
}

// 24 bytes: a run of lanes [first, last] with their count and a floating-point sum in the order of the lanes; a padding word at 12
struct WaveSpan {
  int first, last, count;
  double sum;
};
static_assert(sizeof(WaveSpan) == 24, "the test relies on the padding word");

// p followed by q: ordered (first comes from the left operand, last from the right one, and the sum is rounded in that order)
WAVE_CASE_CALL void span_concat(WaveSpan &p, const WaveSpan &q) {
  p.last = q.last;
  p.count += q.count;
  p.sum = p.sum + q.sum;
}

// 8 bytes: an integer sum and the number of accumulators that went into it, so that a slot lost or read twice shows
struct WaveSum {
  int sum, n;
};

// the identities of case_min and sum_add: what block_merge's caller clears its total to
WAVE_CASE_CALL void case_clear(WaveCase &p) { p.x = INFINITY; p.a = p.b[0] = p.b[1] = p.b[2] = INT32_MAX; }
WAVE_CASE_CALL void sum_clear(WaveSum &p) { p.sum = p.n = 0; }

WAVE_CASE_CALL void sum_add(WaveSum &p, const WaveSum &q) {
  p.sum += q.sum;
  p.n += q.n;
}
