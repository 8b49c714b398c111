// jstruct_blocks.hip -- test infrastructure (tests/test_jstruct_blocks_gpu.py): the device functions of the joint plan's separator recursion
// (cfz_jstruct.inl jbcr_*) and the 64-row eliminations under them (cfz_struct.inl lu64_*) run ALONE, on systems the test chooses.  They exist in
// the device pass only, so the CPU build of the same source never sees them.  This file includes the product sources as cfz_planning.hip does and
// adds three kernels that call cfzc:: functions; of their own they only load and store.
//
//   jstruct_blocks <in> <out>
// in:  int64 header[8] = {mode, n, p1, p2, 0..}, then the mode's data (below);  out: doubles.  Every HIP call is checked; the first error is printed
// and ends the program (exit status 1) before anything else is launched.
//
// The level loop of `recursion_kernel` is a COPY of jstruct_solve's phase 3 (cfz_jstruct.inl, "phase 3: recursion over the joint separators"):
// moving that loop into a function of its own changed the register allocation of colloc_kernel, so the product keeps it where it is.  Whoever
// changes one changes the other.

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>
#include <cstdlib>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/confrez_hip.h"
#include "../../conflict_rez_amd/csrc/cfz_common.h"
#include "../../conflict_rez_amd/csrc/cfz_solver.inl"
#include "../../conflict_rez_amd/csrc/cfz_plan.inl"
#include "../../conflict_rez_amd/csrc/cfz_colloc.inl"

namespace {

constexpr int kB = cfzc::kJB, kU = cfzc::kJU, kL = cfzc::kJL;

// mode 1: n blocks [A | B] column-major (64 rows, 64 + RB columns) -> A^-1 B column-major (64 x RB) and the flag of each block.
// One wavefront per block; the fill gives lane = row sixteen columns at a time, as jbcr_lu_all's does.
template <int RB>
__global__ __launch_bounds__(512) void blocks_kernel(int n, const double *in, double *out, double *flags) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ double wlds[];
  const int wave = threadIdx.x >> 6, k = blockIdx.x * (blockDim.x >> 6) + wave;
  if (k >= n) return;
  cfzb::lds_f64 *lds = cfzc::juni_lds((cfzb::lds_f64 *)wlds) + wave * cfzc::kLuLdsWave;
  const cfzb::glb_f64 *blk = cfzc::juni((const cfzb::glb_f64 *)in + (size_t)k * kB * (kB + RB));
  cfzb::glb_f64 *o = cfzc::juni((cfzb::glb_f64 *)out + (size_t)k * kB * RB);
  const int lane = cfzc::lu_opaque(threadIdx.x & 63);
  const int f = cfzc::lu64_build<RB>(lds, o, [&](auto Jc, double (&v)[16]) {
    constexpr int J = decltype(Jc)::value;
#pragma unroll
    for (int c = 0; c < 16; ++c) v[c] = blk[(16 * J + c) * kB + lane];
  });
  if ((threadIdx.x & 63) == 0) flags[k] = f ? 1.0 : 0.0;
#endif
}

// mode 2: n operand sets {A, G, B: 32 x 32 row-major, logically 28 x 28; vec: 32 x 2} -> per set X = A (G B) with the two vec columns
// (jbcr_triple<true>) and without (jbcr_triple<false>), each 32 x 32 row-major with the number of times every entry was reported.
// One wavefront (one workgroup of 64) per set.  The element functions clamp the index for the load and return zero beyond 27.
__global__ __launch_bounds__(512) void triple_kernel(int n, const double *in, double *X, unsigned *cnt) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int k = blockIdx.x;
  if (k >= n || threadIdx.x >= 64) return;
  const double *A = in + (size_t)k * (3 * 1024 + 64), *G = A + 1024, *Bm = G + 1024, *vec = Bm + 1024;
  auto in28 = [](int x) { return x < kL ? x : kL - 1; };
  auto el = [&](const double *M, int i, int j) { const double v = M[in28(i) * 32 + in28(j)]; return (i < kL && j < kL) ? v : 0.0; };
  double *Xt = X + (size_t)k * 2048, *Xf = Xt + 1024;
  unsigned *ct = cnt + (size_t)k * 2048, *cf = ct + 1024;
  cfzc::jbcr_triple<true>([&](int i, int j) { return el(A, i, j); }, [&](int i, int j) { return el(G, i, j); }, [&](int i, int j) { return el(Bm, i, j); },
                          [&](int i, int s_) { const double v = vec[in28(i) * 2 + s_]; return i < kL ? v : 0.0; },
                          [&](int i, int j, double v) { if (i >= 0 && i < 32 && j >= 0 && j < 32) { Xt[i * 32 + j] = v; atomicAdd(ct + i * 32 + j, 1u); } });
  cfzc::jbcr_triple<false>([&](int i, int j) { return el(A, i, j); }, [&](int i, int j) { return el(G, i, j); }, [&](int i, int j) { return el(Bm, i, j); },
                           [&](int, int) { return 0.0; },
                           [&](int i, int j, double v) { if (i >= 0 && i < 32 && j >= 0 && j < 32) { Xf[i * 32 + j] = v; atomicAdd(cf + i * 32 + j, 1u); } });
#endif
}

// mode 3: phase 3 of jstruct_solve on n systems, one workgroup each (blockDim.x = 64, 128 or 512: one, two or eight wavefronts).
// System k: blocks off[k] .. off[k] + Nm[k] of Ds [64 x 64], Us [64 x 32], Zs, Zb [64 x 32], Lc [28 x 28], xs [2 x 64]; flag[k].
__global__ __launch_bounds__(512) void recursion_kernel(int n, const int *Nms, const long long *off, double *Ds_, double *Us_, double *Zs_, double *Zb_, double *Lc_,
                                                        double *xs_, double *flags) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ double wlds[];
  const int k = blockIdx.x;
  if (k >= n) return;
  const int Nm = Nms[k];
  const size_t o = (size_t)off[k];
  struct { double *Ds, *Us, *Zs, *Zb, *Lc, *xs; } s = {Ds_ + o * kB * kB, Us_ + o * kB * kU, Zs_ + o * kB * kU, Zb_ + o * kB * kU, Lc_ + o * kL * kL, xs_ + o * 2 * kB};
  double *flag = flags + k;
  using namespace cfzc;
  // ---- the copy of jstruct_solve's phase 3 begins ----
  {
    const int wv = CFZS_WAVE, nwv = CFZS_NW;
    cfzb::lds_f64 *lb = cfzb::opaque((cfzb::lds_f64 *)wlds);
    int top = 1;
    for (int st = 1; st <= Nm; st *= 2) {
      top = st;
      if (jbcr_lu_all(wv, nwv, st, Nm, (const cfzb::glb_f64 *)s.Ds, (const cfzb::glb_f64 *)s.Us, (cfzb::glb_f64 *)s.Zs, (cfzb::glb_f64 *)s.Zb, lb) && CFZS_LANE == 0) flag[0] = 1.0;
      __syncthreads();
      if (flag[0] != 0.0) return;
      jbcr_update_all(wv, nwv, st, Nm, (cfzb::glb_f64 *)s.Ds, (cfzb::glb_f64 *)s.Us, (const cfzb::glb_f64 *)s.Zs, (const cfzb::glb_f64 *)s.Zb, (cfzb::glb_f64 *)s.Lc);
      __syncthreads();
    }
    if (jbcr_lu_all(wv, nwv, 0, Nm, (const cfzb::glb_f64 *)s.Ds, (const cfzb::glb_f64 *)s.Us, (cfzb::glb_f64 *)s.Zs, (cfzb::glb_f64 *)s.Zb, lb) && CFZS_LANE == 0) flag[0] = 1.0;
    __syncthreads();
    if (flag[0] != 0.0) return;
    for (int c = wv; c < 2; c += nwv) s.xs[c * kJB + CFZS_LANE] = s.Zs[(28 + c) * kJB + CFZS_LANE];  // (a workgroup of one wavefront copies both)
    __syncthreads();
    for (int st = top; st >= 1; st /= 2) {
      jbcr_back_all(wv, nwv, st, Nm, (const cfzb::glb_f64 *)s.Us, (const cfzb::glb_f64 *)s.Zs, (const cfzb::glb_f64 *)s.Zb, (const cfzb::glb_f64 *)s.Lc, (cfzb::glb_f64 *)s.xs);
      __syncthreads();
    }
  }
  // ---- the copy ends ----
#endif
}

#define CHECK(call)                                                                                   \
  do {                                                                                                \
    const hipError_t e_ = (call);                                                                     \
    if (e_ != hipSuccess) {                                                                           \
      fprintf(stderr, "jstruct_blocks: %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); \
      exit(1);                                                                                        \
    }                                                                                                 \
  } while (0)

void die(const char *msg) { fprintf(stderr, "jstruct_blocks: %s\n", msg); exit(1); }

template <class T>
T *to_device(const T *h, size_t n) {
  T *d = nullptr;
  CHECK(hipMalloc((void **)&d, std::max<size_t>(n, 1) * sizeof(T)));
  if (n) CHECK(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
  return d;
}
double *device_filled(size_t n, double v) {
  std::vector<double> h(std::max<size_t>(n, 1), v);
  return to_device(h.data(), h.size());
}
void finish() { CHECK(hipGetLastError()); CHECK(hipDeviceSynchronize()); }
void append(std::vector<double> &out, const double *d, size_t n) {
  const size_t at = out.size();
  out.resize(at + n);
  if (n) CHECK(hipMemcpy(out.data() + at, d, n * sizeof(double), hipMemcpyDeviceToHost));
}
constexpr size_t kLdsBytes = (size_t)8 * cfzc::kLuLdsWave * sizeof(double);  // every wavefront of a workgroup of eight its kLuLdsWave doubles

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) die("usage: jstruct_blocks <in> <out>");
  FILE *fi = fopen(argv[1], "rb");
  if (!fi) die("cannot open the input");
  int64_t hd[8];
  if (fread(hd, 8, 8, fi) != 8) die("short header");
  const int mode = (int)hd[0];
  const long long n = hd[1];
  if (n < 1 || n > 100000) die("bad count");
  std::vector<double> out;
  auto read_doubles = [&](std::vector<double> &v, size_t cnt) { v.resize(cnt); if (fread(v.data(), 8, cnt, fi) != cnt) die("short data"); };
  if (mode == 1) {
    const int RB = (int)hd[2];
    if (RB != 16 && RB != 32) die("RB is 16 or 32");
    std::vector<double> in;
    read_doubles(in, (size_t)n * kB * (kB + RB));
    double *din = to_device(in.data(), in.size()), *dout = device_filled((size_t)n * kB * RB, 0.0), *dfl = device_filled(n, -1.0);
    const int grid = (int)((n + 7) / 8);
    if (RB == 16) {
      CHECK(hipFuncSetAttribute((const void *)blocks_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
      hipLaunchKernelGGL(blocks_kernel<16>, dim3(grid), dim3(512), kLdsBytes, 0, (int)n, din, dout, dfl);
    } else {
      CHECK(hipFuncSetAttribute((const void *)blocks_kernel<32>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
      hipLaunchKernelGGL(blocks_kernel<32>, dim3(grid), dim3(512), kLdsBytes, 0, (int)n, din, dout, dfl);
    }
    finish();
    append(out, dout, (size_t)n * kB * RB);
    append(out, dfl, n);
  } else if (mode == 2) {
    std::vector<double> in;
    read_doubles(in, (size_t)n * (3 * 1024 + 64));
    double *din = to_device(in.data(), in.size()), *dX = device_filled((size_t)n * 2048, NAN);
    unsigned *dc = nullptr;
    CHECK(hipMalloc((void **)&dc, (size_t)n * 2048 * sizeof(unsigned)));
    CHECK(hipMemset(dc, 0, (size_t)n * 2048 * sizeof(unsigned)));
    hipLaunchKernelGGL(triple_kernel, dim3((int)n), dim3(64), 0, 0, (int)n, din, dX, dc);
    finish();
    std::vector<unsigned> hc((size_t)n * 2048);
    CHECK(hipMemcpy(hc.data(), dc, hc.size() * sizeof(unsigned), hipMemcpyDeviceToHost));
    append(out, dX, (size_t)n * 2048);
    for (unsigned c : hc) out.push_back((double)c);
  } else if (mode == 3) {
    // header[2]: threads per workgroup (64, 128, 512; 0 = one run with each, in that order); header[3]: what the workspaces Zs, Zb, Lc, xs and
    // the spare columns 30, 31 of every Us block hold before the launch (0 = zeros, 1 = NaN, 2 = one run with each, zeros first).
    // Output: per run (fills outermost) xs of every block, then the flag of every system.
    std::vector<int> shapes, fills;
    if (hd[2] == 0) shapes = {64, 128, 512}; else if (hd[2] == 64 || hd[2] == 128 || hd[2] == 512) shapes = {(int)hd[2]}; else die("0, 64, 128 or 512 threads");
    if (hd[3] == 2) fills = {0, 1}; else if (hd[3] == 0 || hd[3] == 1) fills = {(int)hd[3]}; else die("fill is 0, 1 or 2");
    std::vector<int64_t> nm64(n);
    if (fread(nm64.data(), 8, n, fi) != (size_t)n) die("short data");
    std::vector<int> Nms(n);
    std::vector<long long> off(n);
    long long tot = 0;
    for (long long k = 0; k < n; ++k) {
      if (nm64[k] < 1 || nm64[k] > 255) die("Nm is 1 .. 255");
      Nms[k] = (int)nm64[k]; off[k] = tot; tot += nm64[k] + 1;
    }
    std::vector<double> Ds, Us;
    read_doubles(Ds, (size_t)tot * kB * kB);
    read_doubles(Us, (size_t)tot * kB * kU);
    int *dN = to_device(Nms.data(), Nms.size());
    long long *doff = to_device(off.data(), off.size());
    CHECK(hipFuncSetAttribute((const void *)recursion_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
    for (int nanfill : fills)
      for (int threads : shapes) {
        const double fill = nanfill ? NAN : 0.0;
        for (long long b = 0; b < tot; ++b)
          for (int e = 30 * kB; e < 32 * kB; ++e) Us[(size_t)b * kB * kU + e] = fill;
        double *dDs = to_device(Ds.data(), Ds.size()), *dUs = to_device(Us.data(), Us.size());  // (a run overwrites both)
        double *dZs = device_filled((size_t)tot * kB * kU, fill), *dZb = device_filled((size_t)tot * kB * kU, fill), *dLc = device_filled((size_t)tot * kL * kL, fill);
        double *dxs = device_filled((size_t)tot * 2 * kB, fill), *dfl = device_filled(n, 0.0);
        hipLaunchKernelGGL(recursion_kernel, dim3((int)n), dim3(threads), kLdsBytes, 0, (int)n, dN, doff, dDs, dUs, dZs, dZb, dLc, dxs, dfl);
        finish();
        append(out, dxs, (size_t)tot * 2 * kB);
        append(out, dfl, n);
        for (double *p : {dDs, dUs, dZs, dZb, dLc, dxs, dfl}) CHECK(hipFree(p));
      }
  } else die("mode is 1 (blocks), 2 (triple) or 3 (recursion)");
  fclose(fi);
  FILE *fo = fopen(argv[2], "wb");
  if (!fo || fwrite(out.data(), 8, out.size(), fo) != out.size() || fclose(fo) != 0) die("cannot write the output");
  return 0;
}
