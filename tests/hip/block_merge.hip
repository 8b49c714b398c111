// tests/test_block_merge_gpu.py: the workgroup merge of conflict_rez_amd/csrc/cfz_wave.inl alone, one workgroup of four wavefronts and
// one of two.
//   block_merge <in> <out>
// in:  WaveCase[33][4], WaveSum[33][4], WaveCase[33][2], WaveSum[33][2]: the accumulator of every wavefront in every round (raw structs
//      of tests/hip/wave_merge_case.h).
// out: WaveCase[33][256], WaveSum[33][256], WaveCase[33][128], WaveSum[33][128]: every lane's result of every round.
// A round is one block_merge with the round's parity and nothing else, as a shell of delay_kernel is: one barrier per round.  In odd
// rounds wavefront (round % Waves) runs a chain of dependent integer operations that starts from the value it has just merged, so that
// the others have stored the next round and wait at its barrier while it is still busy with this one.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../conflict_rez_amd/csrc/cfz_wave.inl"
#include "wave_merge_case.h"

static void die(const char *what) { fprintf(stderr, "block_merge: %s\n", what); exit(1); }
#define CHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) die(hipGetErrorString(e_)); } while (0)

constexpr int kRounds = 33, kChain = 400;

template <class T, void (*Merge)(T &, const T &), void (*Clear)(T &), int Waves>
__device__ __forceinline__ void rounds(const T *in, T *out, int (*slots)[Waves][sizeof(T) / 4], unsigned *chain) {
  const int wave = threadIdx.x >> 6;
  for (int r = 0; r < kRounds; ++r) {
    T tot;
    Clear(tot);
    cfz::block_merge<T, Merge, Waves>(tot, in[r * Waves + wave], slots, r);
    if ((r & 1) && wave == r % Waves) {
      unsigned z;
      __builtin_memcpy(&z, &tot, 4);
      for (int i = 0; i < kChain; ++i) z = z * 1664525u + 1013904223u + threadIdx.x;
      chain[threadIdx.x] = z;  // (keeps the chain alive)
      __threadfence_block();
    }
    out[r * (Waves * 64) + threadIdx.x] = tot;
  }
}

template <int Waves>
__global__ __launch_bounds__(Waves * 64) void block_kernel(const WaveCase *c, const WaveSum *s, WaveCase *co, WaveSum *so, unsigned *chain) {
  __shared__ int cs[2][Waves][sizeof(WaveCase) / 4], ss[2][Waves][sizeof(WaveSum) / 4];
  rounds<WaveCase, case_min, case_clear, Waves>(c, co, cs, chain);
  __syncthreads();
  rounds<WaveSum, sum_add, sum_clear, Waves>(s, so, ss, chain);
}

template <int Waves>
static void run(FILE *fi, FILE *fo) {
  constexpr int L = Waves * 64;
  std::vector<WaveCase> c(kRounds * Waves), co(kRounds * L);
  std::vector<WaveSum> s(kRounds * Waves), so(kRounds * L);
  if (fread(c.data(), sizeof(WaveCase), c.size(), fi) != c.size() || fread(s.data(), sizeof(WaveSum), s.size(), fi) != s.size()) die("short input");
  WaveCase *dc, *dco;
  WaveSum *ds, *dso;
  unsigned *dch;
  CHECK(hipMalloc((void **)&dc, c.size() * sizeof(WaveCase))); CHECK(hipMalloc((void **)&dco, co.size() * sizeof(WaveCase)));
  CHECK(hipMalloc((void **)&ds, s.size() * sizeof(WaveSum))); CHECK(hipMalloc((void **)&dso, so.size() * sizeof(WaveSum)));
  CHECK(hipMalloc((void **)&dch, L * sizeof(unsigned)));
  CHECK(hipMemcpy(dc, c.data(), c.size() * sizeof(WaveCase), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(ds, s.data(), s.size() * sizeof(WaveSum), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(block_kernel<Waves>, dim3(1), dim3(L), 0, 0, dc, ds, dco, dso, dch);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(co.data(), dco, co.size() * sizeof(WaveCase), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(so.data(), dso, so.size() * sizeof(WaveSum), hipMemcpyDeviceToHost));
  if (fwrite(co.data(), sizeof(WaveCase), co.size(), fo) != co.size() || fwrite(so.data(), sizeof(WaveSum), so.size(), fo) != so.size()) die("cannot write the output");
}

int main(int argc, char **argv) {
  if (argc != 3) die("usage: block_merge <in> <out>");
  FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
  if (!fi || !fo) die("cannot open the files");
  run<4>(fi, fo);
  run<2>(fi, fo);
  if (fclose(fo) != 0) die("cannot write the output");
  return 0;
}
