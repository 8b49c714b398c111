// cfz_wave.inl -- how the analysis kernels of cfz_engine.hip (audit, score, conflict, delay, schedule) merge the accumulator structs T of
// a wavefront's lanes, and of a workgroup's wavefronts, with the `*_merge(T &a, const T &b)` of their .inl, stated once for the device
// and for the CPU test builds (tests/emu); and what the .inl files of those kernels share: CFZ_CALL (compiled by hipcc and g++ alike), rows of bits.
// width: the lanes of a group, a power of two (on the device at most 64: a group lies in one wavefront); the host forms run the lanes
// acc[0 .. nl) in groups of width.  Device and host form of a butterfly stand side by side: the order of the merges is read in one place.
#ifndef CFZ_WAVE_INL
#define CFZ_WAVE_INL

#include <stdint.h>
#include <type_traits>

#ifndef CFZ_CALL
#if defined(__HIPCC__)
#define CFZ_CALL __host__ __device__ __forceinline__
#else
#define CFZ_CALL static inline
#endif
#endif

namespace cfz {
// a row of n bits as 32-bit words (the free mask of cfz_delay.inl, the diagram rows of cfz_coord.inl): bit (c & 31) of word (c >> 5)
CFZ_CALL int bit_words(int n) { return (n + 31) / 32; }
CFZ_CALL bool bit_test(const uint32_t *row, int c) { return (row[c >> 5] >> (c & 31)) & 1u; }

#if defined(__HIPCC__)
// v of lane (lane ^ off), shuffled word by word: no list of T's fields to keep in step with the struct (padding travels too)
template <class T>
__device__ __forceinline__ T wave_xor(const T &v, int off) {
  static_assert(std::is_trivially_copyable<T>::value, "wave_xor copies T as words");
  static_assert(sizeof(T) % 4 == 0, "wave_xor shuffles whole 32-bit words");
  int w[sizeof(T) / 4];
  __builtin_memcpy(w, &v, sizeof(T));
  for (unsigned i = 0; i < sizeof(T) / 4; ++i) w[i] = __shfl_xor(w[i], off, 64);
  T o;
  __builtin_memcpy(&o, w, sizeof(T));
  return o;
}
// commutative Merge (a minimum under a total order, an integer sum): off = width / 2 .. 1, lane 0 of a group ends with its total
template <class T, void (*Merge)(T &, const T &)>
__device__ __forceinline__ void wave_merge(T &acc, int width) {
  for (int off = width / 2; off > 0; off >>= 1) Merge(acc, wave_xor(acc, off));
}
#endif
template <class T, void (*Merge)(T &, const T &)>
inline void wave_merge_host(T *acc, int nl, int width) {
  for (int off = width / 2; off > 0; off >>= 1)
    for (int l = 0; l < nl; ++l)
      if (!(l & off)) { const T lo = acc[l]; Merge(acc[l], acc[l | off]); Merge(acc[l | off], lo); }
}

// ordered Merge (a followed by b; lane j holds the j-th segment): off = 1 .. width / 2 with the LOWER lane as the left operand in both
// lanes of a pair, so every lane of a group ends with the same total, merged in one fixed tree
#if defined(__HIPCC__)
template <class T, void (*Merge)(T &, const T &)>
__device__ __forceinline__ void wave_merge_ordered(T &acc, int lane, int width) {
  for (int off = 1; off < width; off <<= 1) {
    T o = wave_xor(acc, off);
    if (lane & off) { Merge(o, acc); acc = o; }
    else Merge(acc, o);
  }
}
#endif
template <class T, void (*Merge)(T &, const T &)>
inline void wave_merge_ordered_host(T *acc, int nl, int width) {
  for (int off = 1; off < width; off <<= 1)
    for (int l = 0; l < nl; ++l)
      if (!(l & off)) { Merge(acc[l], acc[l | off]); acc[l | off] = acc[l]; }
}

// A workgroup's wavefronts (acc: a wavefront's total, in its lane 0 after wave_merge) merged into tot, which the caller has cleared, with
// a commutative Merge: lane 0 of each stores acc as words into slots[parity][wave] (LDS), one barrier, every lane merges slots 0 .. Waves - 1
// in that order, so tot is workgroup-uniform.  Two sets of slots by the parity of the caller's round: a wavefront still reading round m
// must not see round m + 1, which a fast one may already be storing; so a loop of rounds needs one barrier per round.  One round: 0.
#if defined(__HIPCC__)
template <class T, void (*Merge)(T &, const T &), int Waves>
__device__ __forceinline__ void block_merge(T &tot, const T &acc, int (*slots)[Waves][sizeof(T) / 4], int parity) {
  static_assert(std::is_trivially_copyable<T>::value && sizeof(T) % 4 == 0, "block_merge copies T as whole 32-bit words");
  int(*x)[sizeof(T) / 4] = slots[parity & 1];
  if ((threadIdx.x & 63) == 0) __builtin_memcpy(x[threadIdx.x >> 6], &acc, sizeof(T));
  __syncthreads();
  T o;
  for (int k = 0; k < Waves; ++k) { __builtin_memcpy(&o, x[k], sizeof(T)); Merge(tot, o); }
}
#endif
// the same fold over acc[0], acc[stride], ... of `waves` wavefronts (stride: the lanes of a wavefront, where acc holds every lane)
template <class T, void (*Merge)(T &, const T &)>
inline void block_merge_host(T &tot, const T *acc, int waves, int stride = 1) {
  for (int k = 0; k < waves; ++k) Merge(tot, acc[k * stride]);
}

}  // namespace cfz

#endif  // CFZ_WAVE_INL
