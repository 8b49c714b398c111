// devmem_host.cpp -- conflict_rez_amd/csrc/cfz_devmem.h alone, on the CPU: DevBuf and Arena over a counting allocator on malloc that can
// be told to fail its k-th call.  Stand-alone (tests/test_devmem_host.py builds it with g++ -fsanitize=address,undefined and runs it once
// per case); no HIP, nothing of the library but that header.   usage: devmem_host <case>   exit 0: every check held and nothing is live
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "../../conflict_rez_amd/csrc/cfz_devmem.h"

namespace {

struct CountMem {
  static inline std::map<void *, size_t> live;
  static inline size_t live_bytes = 0, peak_bytes = 0;
  static inline long calls = 0, fail_at = 0;  // fail_at: the call (counted from 1 after arm) that fails; 0: none
  static inline std::string err;
  static void arm(long k) { calls = 0; fail_at = k; peak_bytes = live_bytes; }
  static int alloc(void **p, size_t bytes) {
    if (++calls == fail_at) { err = "CountMem: out of memory"; return -1; }
    *p = std::malloc(bytes);
    if (!*p) std::abort();
    live[*p] = bytes;
    live_bytes += bytes;
    if (live_bytes > peak_bytes) peak_bytes = live_bytes;
    return 0;
  }
  static void free(void *p) {
    auto it = live.find(p);
    if (it == live.end()) { std::fprintf(stderr, "free of a block that is not live\n"); std::abort(); }
    live_bytes -= it->second;
    live.erase(it);
    std::free(p);
  }
};

typedef DevBuf<int, CountMem> Buf;

int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } } while (0)

void fill(Buf &b, int v) { for (size_t i = 0; i < b.size(); ++i) b[i] = v + (int)i; }
bool holds(const Buf &b, int v) { for (size_t i = 0; i < b.size(); ++i) if (b[i] != v + (int)i) return false; return true; }

void case_alloc_reset() {
  Buf b;
  CHECK(b.get() == nullptr && b.size() == 0 && !b);
  CHECK(b.alloc(7) == 0 && b.get() != nullptr && b.size() == 7 && CountMem::live.size() == 1 && CountMem::live_bytes == 7 * sizeof(int));
  int *raw = b;  // the implicit conversion
  CHECK(raw == b.get());
  fill(b, 3);
  CHECK(b.alloc(9) == 0 && b.size() == 9 && CountMem::live.size() == 1 && CountMem::live_bytes == 9 * sizeof(int));  // the first block went
  b.reset();
  CHECK(b.get() == nullptr && b.size() == 0 && CountMem::live.empty());
  b.reset();  // twice is harmless
  CHECK(b.alloc(0) == 0 && b.get() == nullptr && b.size() == 0 && CountMem::live.empty());
  CountMem::arm(1);
  CHECK(b.alloc(4) == -1 && b.get() == nullptr && b.size() == 0 && CountMem::err == "CountMem: out of memory");
}

void case_reserve() {
  Buf b;
  CHECK(b.reserve(10) == 0 && b.size() == 10);
  int *p = b;
  CHECK(b.reserve(5) == 0 && b.get() == p && b.size() == 10);
  CHECK(b.reserve(10) == 0 && b.get() == p);
  CountMem::arm(0);
  CHECK(b.reserve(20) == 0 && b.size() == 20);
  CHECK(CountMem::peak_bytes == 20 * sizeof(int));  // released before it allocated: the larger block, not the sum
  CountMem::arm(1);
  CHECK(b.reserve(40) == -1 && b.get() == nullptr && b.size() == 0 && CountMem::live.empty());
  CHECK(b.reserve(40) == 0 && b.size() == 40 && CountMem::live.size() == 1);  // the repeat completes it
}

void case_move() {
  Buf a;
  CHECK(a.alloc(4) == 0);
  fill(a, 10);
  int *pa = a;
  Buf b(std::move(a));
  CHECK(a.get() == nullptr && a.size() == 0 && b.get() == pa && b.size() == 4 && holds(b, 10) && CountMem::live.size() == 1);
  Buf c;
  CHECK(c.alloc(6) == 0);
  c = std::move(b);  // c's block is released, b is left empty
  CHECK(b.get() == nullptr && b.size() == 0 && c.get() == pa && c.size() == 4 && holds(c, 10) && CountMem::live.size() == 1);
  Buf &self = c;
  c = std::move(self);
  CHECK(c.get() == pa && c.size() == 4 && holds(c, 10) && CountMem::live.size() == 1);
}

struct Five { Buf a, b, c, d, e; int n = 0; };

void case_release_by_assignment() {  // the idiom of loop_release
  Five f;
  CHECK(f.a.alloc(1) == 0 && f.b.alloc(2) == 0 && f.c.alloc(3) == 0 && f.d.alloc(4) == 0 && f.e.alloc(5) == 0);
  f.n = 5;
  CHECK(CountMem::live.size() == 5);
  f = Five();
  CHECK(CountMem::live.empty() && !f.a && !f.b && !f.c && !f.d && !f.e && f.e.size() == 0 && f.n == 0);
}

struct Three { Buf a, b, c; int tag = 0; };

// an entry point under the commit rule: build into locals, check every step, move into the handle last
int set_three(Three &h, size_t n, int v) {
  Buf a, b, c;
  if (a.alloc(n) || b.alloc(2 * n) || c.alloc(3 * n)) return -1;
  fill(a, v); fill(b, v + 100); fill(c, v + 200);
  h.a = std::move(a); h.b = std::move(b); h.c = std::move(c);
  h.tag = v;
  return 0;
}

void case_commit() {
  Three h;
  CHECK(set_three(h, 3, 1) == 0 && CountMem::live.size() == 3);
  for (long k = 1; k <= 3; ++k) {
    int *const pa = h.a, *const pb = h.b, *const pc = h.c;
    CountMem::arm(k);
    CHECK(set_three(h, 5, 7) == -1);
    CHECK(h.a.get() == pa && h.b.get() == pb && h.c.get() == pc && h.a.size() == 3 && h.b.size() == 6 && h.c.size() == 9);
    CHECK(holds(h.a, 1) && holds(h.b, 101) && holds(h.c, 201) && h.tag == 1);
    CHECK(CountMem::live.size() == 3 && CountMem::live_bytes == 18 * sizeof(int));
  }
  CountMem::arm(0);
  CHECK(set_three(h, 5, 7) == 0 && h.a.size() == 5 && holds(h.c, 207) && h.tag == 7 && CountMem::live.size() == 3);
}

void case_arena() {
  const size_t MB = (size_t)1 << 20;
  Arena<CountMem> a;
  void *p = nullptr, *q = nullptr;
  CHECK(arena_alloc(a, &p, 100) == 0 && p && a.blocks.size() == 1 && a.blocks[0].base.size() == MB && a.blocks[0].off == 256);
  CHECK(arena_alloc(a, &q, 300) == 0 && q == (char *)p + 256 && a.blocks[0].off == 256 + 512);
  CHECK(arena_reset(a) == 0 && a.used_last == 768 && a.blocks.size() == 1 && a.blocks[0].off == 0);  // one block: kept
  // a call that spills: a second block; the next reset merges the two into one of the total size, the old ones released first
  CHECK(arena_alloc(a, &p, MB) == 0 && arena_alloc(a, &q, 3 * MB) == 0 && a.blocks.size() == 2 && CountMem::live_bytes == 4 * MB);
  CountMem::arm(0);
  CHECK(arena_reset(a) == 0 && a.blocks.size() == 1 && a.blocks[0].base.size() == 4 * MB && a.blocks[0].off == 0);
  CHECK(CountMem::live.size() == 1 && CountMem::peak_bytes == 4 * MB);
  // the merge allocation fails: the reset is refused, the arena is empty and holds nothing; the next call starts anew
  CHECK(arena_alloc(a, &p, 4 * MB) == 0 && arena_alloc(a, &q, 100) == 0 && a.blocks.size() == 2);
  CountMem::arm(1);
  CHECK(arena_reset(a) == -1 && a.blocks.empty() && CountMem::live.empty());
  CHECK(arena_reset(a) == 0 && arena_alloc(a, &p, 100) == 0 && a.blocks.size() == 1 && CountMem::live_bytes == MB);
  // a failing block leaves the arena as it was
  CountMem::arm(1);
  CHECK(arena_alloc(a, &q, 2 * MB) == -1 && a.blocks.size() == 1 && CountMem::live_bytes == MB);
  arena_destroy(a);
  CHECK(a.blocks.empty() && CountMem::live.empty());
  // the shrink rule: a block above 256 MB of which the last call used less than a quarter goes at the next reset (never touched here)
  CHECK(arena_alloc(a, &p, 300 * MB) == 0 && arena_reset(a) == 0 && a.blocks.size() == 1);  // used all of it: kept
  CHECK(arena_alloc(a, &p, 75 * MB) == 0 && arena_reset(a) == 0 && a.blocks.size() == 1);   // a quarter: kept
  CHECK(arena_alloc(a, &p, 74 * MB) == 0 && arena_reset(a) == 0 && a.blocks.empty() && CountMem::live.empty());
  CHECK(arena_alloc(a, &p, 200 * MB) == 0 && arena_alloc(a, &q, 256) == 0 && arena_reset(a) == 0);
  CHECK(a.blocks.size() == 1 && a.blocks[0].base.size() == 201 * MB);  // merged
  CHECK(arena_alloc(a, &p, 256) == 0 && arena_reset(a) == 0 && a.blocks.size() == 1);  // not above 256 MB: kept however little is used
  // (the arena goes out of scope holding a block: the destructor releases it)
}

}  // namespace

int main(int argc, char **argv) {
  const std::map<std::string, void (*)()> cases = {{"alloc_reset", case_alloc_reset}, {"reserve", case_reserve}, {"move", case_move},
                                                   {"release_by_assignment", case_release_by_assignment}, {"commit", case_commit},
                                                   {"arena", case_arena}};
  const auto it = argc == 2 ? cases.find(argv[1]) : cases.end();
  if (it == cases.end()) { std::fprintf(stderr, "usage: devmem_host <case>\n"); return 2; }
  it->second();
  if (!CountMem::live.empty()) { std::fprintf(stderr, "%zu blocks still live\n", CountMem::live.size()); ++g_bad; }
  if (CountMem::live_bytes != 0) ++g_bad;
  std::printf("%s: %s, live blocks %zu\n", argv[1], g_bad ? "FAILED" : "ok", CountMem::live.size());
  return g_bad ? 1 : 0;
}
