// sweep_blocks.hip -- test infrastructure (tests/test_sweeps_gpu.py): the device functions that compute every Newton step of the interior-point
// solvers -- cfz::riccati_backward_mfma, cfz::forward_scan, cfz::costate_scan (cfz_solver.inl) and cfzp::riccati_backward_mfma (cfz_plan.inl) --
// run ALONE, on systems the test chooses (oracle/sweeps.py).  They exist in the device pass only, so the CPU build of the same source never
// sees them.  This file includes the product sources as cfz_planning.hip does and adds two kernels that copy a workspace in, call, and copy
// out; there is no arithmetic of their own in them.
//
//   sweep_blocks <in> <out>
// in:  int64 header[8] = {mode, n, fill, ...}, then the mode's data (below);  out: doubles.  fill: what every workspace word that is no
// input of the functions called holds before the launch: 0 = zeros, 1 = NaN, 2 = one run with each, zeros first.  Every HIP call is checked;
// the first error is printed and ends the program (exit status 1) before anything else is launched.
//
// modes 1, 2, 3 (MPC step; header[3..5] = N, nb, n_nbr; data: dt, then n records of  ab [N 15] d [N 5] hc [N 11] gk [N 7] kk [N 12] rP [30] x0 [5]
//   p0 [5] pi0 [5] pi [N 5]):  one workgroup of cfz::kNL threads per system, the workspace of cfz::make_layout(N, nb, n_nbr) in LDS.
//   1: CFZ_RICCATI;  2: forward_scan, costate_scan through CFZ_WAVE0 from the record's kk and rP;  3: the three in the order of the solver's Newton
//   step.  Inputs placed: ab (without the word s20) and d of stages 0 .. N - 2, hc, gk;  2, 3 also x0, p0, pi0, pi of stages 0 .. N - 2;  2 also kk, rP.
//   out, per run and system:  kk [N 12], rP [30] as the sweep left it (1; zeros otherwise), dp [N 7], dpi0 [5], dpi [N 5].
// mode 4 (state_ws sweep; header[3] = 1: stage data and feedback in LDS, 0: in global memory, as newton_step<true / false> passes them; data:
//   dt, int64 T[n], int64 has_final[n], then per system st [(T + 1) kSt]):  one workgroup of 256 threads per system, its first wavefront sweeps.
//   out, per run:  fb [(T + 1) kFb] of every system, vf [(T + 1) kVf] of every system, the flag of every system.

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <vector>

#include "../../include/confrez_hip.h"
#include "../../conflict_rez_amd/csrc/cfz_common.h"
#include "../../conflict_rez_amd/csrc/cfz_solver.inl"
#include "../../conflict_rez_amd/csrc/cfz_plan.inl"

namespace {

__global__ __launch_bounds__(cfz::kNL) void mpc_kernel(int n, int N, int nb, int n_nbr, double dt, int sweep, int scans, const double *in, double *out, double *rP_out) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ double smem[];
  const int b = blockIdx.x;
  if (b >= n) return;
  using namespace cfz;  // (CFZ_RICCATI names the sweep as the solver does, from inside the namespace)
  const cfz::Lay L = cfz::make_layout(N, nb, n_nbr);
  double *m = smem;
  for (int i = threadIdx.x; i < L.total; i += cfz::kNL) m[i] = in[(size_t)b * L.total + i];
  __syncthreads();
  if (sweep) {
    CFZ_RICCATI(CFZ_WSP(m), N, dt, L.ab, L.hc, L.gk, L.d, L.kk, L.rP);
    for (int i = threadIdx.x; i < 30; i += cfz::kNL) rP_out[(size_t)b * 30 + i] = m[L.rP + i];
    __syncthreads();
  }
  if (scans) {
    CFZ_WAVE0(forward_scan(CFZ_WSP(m), N, dt, L.ab, L.d, L.kk, L.rP, L.p, L.dp, L.x0, L.pi0, L.dpi0));
    CFZ_WAVE0(costate_scan(CFZ_WSP(m), N, L.ab, L.hc, L.gk, L.kk, L.dp, L.dpi, L.pi));
  }
  for (int i = threadIdx.x; i < L.total; i += cfz::kNL) out[(size_t)b * L.total + i] = m[i];
#endif
}

// off[b]: the first stage of system b among all systems' stages
template <bool FAST>
__global__ __launch_bounds__(256) void plan_kernel(int n, const int *Ts, const int *has_final, const long long *off, double dt, double *st, double *fb, double *vf, double *flags) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ double smem[];
  const int b = blockIdx.x;
  if (b >= n) return;
  const int T = Ts[b];
  double *st_g = st + (size_t)off[b] * cfzp::kSt, *fb_g = fb + (size_t)off[b] * cfzp::kFb, *vf_g = vf + (size_t)off[b] * cfzp::kVf;
  double *const st_ = FAST ? smem : st_g;
  double *const fb_ = FAST ? smem + (size_t)cfzp::kSt * (T + 1) : fb_g;
  if (FAST) {
    for (int i = threadIdx.x; i < cfzp::kSt * (T + 1); i += blockDim.x) st_[i] = st_g[i];
    for (int i = threadIdx.x; i < cfzp::kFb * (T + 1); i += blockDim.x) fb_[i] = fb_g[i];
    __syncthreads();
  }
  if (threadIdx.x < 64) {
    int fail;
    if (FAST) fail = cfzp::riccati_backward_mfma(T, dt, has_final[b], vf_g, CFZP_OPAQUE((cfzp::fast_f64 *)st_), CFZP_OPAQUE((cfzp::fast_f64 *)fb_));
    else fail = cfzp::riccati_backward_mfma(T, dt, has_final[b], vf_g, (cfzb::glb_f64 *)st_, (cfzb::glb_f64 *)fb_);
    if (threadIdx.x == 0) flags[b] = (double)fail;
  }
  __syncthreads();
  if (FAST)
    for (int i = threadIdx.x; i < cfzp::kFb * (T + 1); i += blockDim.x) fb_g[i] = fb_[i];
#endif
}

#define CHECK(call)                                                                                 \
  do {                                                                                              \
    const hipError_t e_ = (call);                                                                   \
    if (e_ != hipSuccess) {                                                                         \
      fprintf(stderr, "sweep_blocks: %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); \
      exit(1);                                                                                      \
    }                                                                                               \
  } while (0)

void die(const char *msg) { fprintf(stderr, "sweep_blocks: %s\n", msg); exit(1); }

template <class T>
T *to_device(const std::vector<T> &h) {
  T *d = nullptr;
  CHECK(hipMalloc((void **)&d, std::max<size_t>(h.size(), 1) * sizeof(T)));
  if (!h.empty()) CHECK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return d;
}
void finish() { CHECK(hipGetLastError()); CHECK(hipDeviceSynchronize()); }
std::vector<double> to_host(const double *d, size_t n) {
  std::vector<double> h(n);
  if (n) CHECK(hipMemcpy(h.data(), d, n * sizeof(double), hipMemcpyDeviceToHost));
  return h;
}
int lds_limit() {
  int dev = 0, bytes = 0, per_cu = 0;  // (as cfz_planning.hip lds_per_workgroup: gfx950 gives a workgroup the CU's 160 KB)
  CHECK(hipGetDevice(&dev));
  CHECK(hipDeviceGetAttribute(&bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  if (hipDeviceGetAttribute(&per_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) == hipSuccess) bytes = std::max(bytes, per_cu);
  return bytes;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) die("usage: sweep_blocks <in> <out>");
  FILE *fi = fopen(argv[1], "rb");
  if (!fi) die("cannot open the input");
  int64_t hd[8];
  if (fread(hd, 8, 8, fi) != 8) die("short header");
  const int mode = (int)hd[0];
  const long long n = hd[1];
  if (n < 1 || n > 4096) die("bad count");
  std::vector<int> fills;
  if (hd[2] == 2) fills = {0, 1}; else if (hd[2] == 0 || hd[2] == 1) fills = {(int)hd[2]}; else die("fill is 0, 1 or 2");
  std::vector<double> out;
  auto read_doubles = [&](std::vector<double> &v, size_t cnt) { v.resize(cnt); if (cnt && fread(v.data(), 8, cnt, fi) != cnt) die("short data"); };
  std::vector<double> dtv;
  read_doubles(dtv, 1);
  const double dt = dtv[0];
  if (mode >= 1 && mode <= 3) {
    const int N = (int)hd[3], nb = (int)hd[4], n_nbr = (int)hd[5];
    if (N < 2 || N > cfz::kMaxN || nb < 0 || nb > 16 || n_nbr < 0 || n_nbr > nb) die("N is 2 .. 32, n_nbr <= nb <= 16");
    const cfz::Lay L = cfz::make_layout(N, nb, n_nbr);
    const size_t lds_bytes = (size_t)L.total * sizeof(double);
    if (lds_bytes > (size_t)lds_limit()) die("the workspace does not fit the LDS");
    const size_t rec = (size_t)N * 55 + 45;
    std::vector<double> in;
    read_doubles(in, (size_t)n * rec);
    CHECK(hipFuncSetAttribute((const void *)mpc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    for (int nanfill : fills) {
      std::vector<double> ws((size_t)n * L.total, nanfill ? NAN : 0.0);
      for (long long b = 0; b < n; ++b) {
        double *m = ws.data() + (size_t)b * L.total;
        const double *ab = in.data() + (size_t)b * rec, *d = ab + N * 15, *hc = d + N * 5, *gk = hc + N * 11, *kk = gk + N * 7, *rP = kk + N * 12,
                     *x0 = rP + 30, *p0 = x0 + 5, *pi0 = p0 + 5, *pi = pi0 + 5;
        for (int k = 0; k < N - 1; ++k) {
          for (int i = 0; i < 15; ++i) if (i != 10) m[L.ab + k * 15 + i] = ab[k * 15 + i];
          for (int i = 0; i < 5; ++i) m[L.d + k * 5 + i] = d[k * 5 + i];
        }
        for (int i = 0; i < N * 11; ++i) m[L.hc + i] = hc[i];
        for (int i = 0; i < N * cfz::kNP; ++i) m[L.gk + i] = gk[i];
        if (mode != 1) {
          for (int i = 0; i < 5; ++i) { m[L.x0 + i] = x0[i]; m[L.p + i] = p0[i]; m[L.pi0 + i] = pi0[i]; }
          for (int i = 0; i < (N - 1) * 5; ++i) m[L.pi + i] = pi[i];
        }
        if (mode == 2) {
          for (int i = 0; i < N * 12; ++i) m[L.kk + i] = kk[i];
          for (int i = 0; i < 30; ++i) m[L.rP + i] = rP[i];
        }
      }
      double *din = to_device(ws), *dout = to_device(std::vector<double>(ws.size(), 0.0)), *drP = to_device(std::vector<double>((size_t)n * 30, 0.0));
      hipLaunchKernelGGL(mpc_kernel, dim3((int)n), dim3(cfz::kNL), lds_bytes, 0, (int)n, N, nb, n_nbr, dt, mode != 2, mode != 1, din, dout, drP);
      finish();
      const std::vector<double> w = to_host(dout, ws.size()), r = to_host(drP, (size_t)n * 30);
      for (long long b = 0; b < n; ++b) {
        const double *m = w.data() + (size_t)b * L.total;
        out.insert(out.end(), m + L.kk, m + L.kk + N * 12);
        for (int i = 0; i < 30; ++i) out.push_back(mode == 1 ? r[(size_t)b * 30 + i] : 0.0);
        out.insert(out.end(), m + L.dp, m + L.dp + N * cfz::kNP);
        out.insert(out.end(), m + L.dpi0, m + L.dpi0 + 5);
        out.insert(out.end(), m + L.dpi, m + L.dpi + N * 5);
      }
      for (double *p : {din, dout, drP}) CHECK(hipFree(p));
    }
  } else if (mode == 4) {
    const bool fast = hd[3] != 0;
    std::vector<int64_t> t64(n), h64(n);
    if (fread(t64.data(), 8, n, fi) != (size_t)n || fread(h64.data(), 8, n, fi) != (size_t)n) die("short data");
    std::vector<int> Ts(n), hf(n);
    std::vector<long long> off(n);
    long long tot = 0;
    int Tmax = 0;
    for (long long b = 0; b < n; ++b) {
      if (t64[b] < 1 || t64[b] > 4096) die("T is 1 .. 4096");
      Ts[b] = (int)t64[b]; hf[b] = h64[b] != 0; off[b] = tot; tot += t64[b] + 1; Tmax = std::max(Tmax, Ts[b]);
    }
    const size_t lds_bytes = fast ? (size_t)(cfzp::kSt + cfzp::kFb) * (Tmax + 1) * sizeof(double) : 0;
    if (lds_bytes > (size_t)lds_limit()) die("the stage data do not fit the LDS");
    std::vector<double> st;
    read_doubles(st, (size_t)tot * cfzp::kSt);
    int *dT = to_device(Ts), *dhf = to_device(hf);
    long long *doff = to_device(off);
    if (fast) CHECK(hipFuncSetAttribute((const void *)plan_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    for (int nanfill : fills) {
      const double fill = nanfill ? NAN : 0.0;
      double *dst = to_device(st), *dfb = to_device(std::vector<double>((size_t)tot * cfzp::kFb, fill)), *dvf = to_device(std::vector<double>((size_t)tot * cfzp::kVf, fill));
      double *dfl = to_device(std::vector<double>(n, -1.0));
      if (fast) hipLaunchKernelGGL(plan_kernel<true>, dim3((int)n), dim3(256), lds_bytes, 0, (int)n, dT, dhf, doff, dt, dst, dfb, dvf, dfl);
      else hipLaunchKernelGGL(plan_kernel<false>, dim3((int)n), dim3(256), 0, 0, (int)n, dT, dhf, doff, dt, dst, dfb, dvf, dfl);
      finish();
      for (const std::vector<double> &v : {to_host(dfb, (size_t)tot * cfzp::kFb), to_host(dvf, (size_t)tot * cfzp::kVf), to_host(dfl, n)}) out.insert(out.end(), v.begin(), v.end());
      for (double *p : {dst, dfb, dvf, dfl}) CHECK(hipFree(p));
    }
  } else die("mode is 1 (sweep), 2 (scans), 3 (Newton step) or 4 (state_ws sweep)");
  fclose(fi);
  FILE *fo = fopen(argv[2], "wb");
  if (!fo || fwrite(out.data(), 8, out.size(), fo) != out.size() || fclose(fo) != 0) die("cannot write the output");
  return 0;
}
