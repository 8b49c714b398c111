// cfz_wave.inl -- how the analysis kernels of cfz_engine.hip (audit, score, conflict, delay) merge the accumulator structs T of a
// wavefront's lanes with the `*_merge(T &a, const T &b)` of their .inl, stated once for the device and for the CPU test builds (tests/emu).
// width: the lanes of a group, a power of two (on the device at most 64: a group lies in one wavefront); the host forms run the lanes
// acc[0 .. nl) in groups of width.  Device and host form of a butterfly stand side by side: the order of the merges is read in one place.
#ifndef CFZ_WAVE_INL
#define CFZ_WAVE_INL

#include <type_traits>

namespace cfz {
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

}  // namespace cfz

#endif  // CFZ_WAVE_INL
