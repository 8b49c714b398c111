// cfz_devmem.h -- who owns device memory in libconfrez_hip.so: DevBuf, one block that is released when its owner goes, and Arena, the
// bump allocator over such blocks that the planning and analysis entry points draw from.  No HIP in here: memory comes from a policy
// Mem with  static int alloc(void **p, size_t bytes)  (0, or -1 with the library's error text set) and  static void free(void *p);
// the library's policies, HipMem and HipHostMem, stand in cfz_common.h, and tests/hip/devmem_host.cpp runs this header on malloc.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace {

struct HipMem;  // cfz_common.h

// n elements of T, or nothing: the pointer is null exactly when the size is 0.  Move-only; converts to T * so that launches and
// copies read as they do with a plain pointer.
template <class T, class Mem = HipMem>
class DevBuf {
  T *p_ = nullptr;
  size_t n_ = 0;

 public:
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
    return *this;
  }
  ~DevBuf() { reset(); }

  void reset() {
    if (p_) Mem::free(p_);
    p_ = nullptr; n_ = 0;
  }
  // exactly n elements, contents undefined; what was held is released first.  A failure leaves the buffer empty.
  int alloc(size_t n) {
    reset();
    void *p = nullptr;
    if (n == 0) return 0;
    if (Mem::alloc(&p, n * sizeof(T))) return -1;
    p_ = static_cast<T *>(p); n_ = n;
    return 0;
  }
  // at least n elements; grows by alloc (the old block goes before the new one comes, contents are not kept)
  int reserve(size_t n) { return n_ >= n ? 0 : alloc(n); }

  T *get() const { return p_; }
  operator T *() const { return p_; }
  size_t size() const { return n_; }
};

// Device memory of one caller, kept between calls: a bump allocator over blocks that go with the arena (or at arena_destroy), are
// merged into one larger block at the next reset, or given back when the calls have become much smaller than the block (a 256-plan
// four-vehicle joint launch takes 25 GB; the next reset after a call that used less than a quarter of a block above 256 MB frees
// it).  Replaces an allocation and a release per call in the planning entry points (each of those is a device-wide synchronisation).
template <class Mem>
struct Arena {
  struct Block { DevBuf<char, Mem> base; size_t off = 0; };
  std::vector<Block> blocks;
  size_t used_last = 0;
};

template <class Mem>
int arena_grow(Arena<Mem> &a, size_t cap, size_t off) {  // one more block of cap bytes, the first off of them handed out
  typename Arena<Mem>::Block b;
  if (b.base.alloc(cap)) return -1;
  b.off = off;
  a.blocks.push_back(std::move(b));
  return 0;
}

template <class Mem>
int arena_reset(Arena<Mem> &a) {  // start of a call: everything handed out before is free again
  size_t used = 0, cap = 0;
  for (auto &b : a.blocks) { used += b.off; cap += b.base.size(); b.off = 0; }
  a.used_last = used;
  if (a.blocks.size() > 1) {  // the last call spilled into extra blocks: one block of the total size from now on
    a.blocks.clear();
    return arena_grow(a, cap, 0);
  }
  if (a.blocks.size() == 1 && cap > ((size_t)1 << 28) && used < cap / 4)
    a.blocks.clear();  // the previous call needed a fraction of what an earlier one left behind
  return 0;
}

template <class Mem>
int arena_alloc(Arena<Mem> &a, void **out, size_t bytes) {
  bytes = (bytes + 255) & ~(size_t)255;
  for (auto &b : a.blocks)
    if (b.base.size() - b.off >= bytes) { *out = b.base.get() + b.off; b.off += bytes; return 0; }
  if (arena_grow(a, bytes > ((size_t)1 << 20) ? bytes : ((size_t)1 << 20), bytes)) return -1;
  *out = a.blocks.back().base.get();
  return 0;
}

template <class Mem>
void arena_destroy(Arena<Mem> &a) { a.blocks.clear(); }  // what cfz_plan_ws_trim gives back; an arena that goes needs no call

}  // namespace
