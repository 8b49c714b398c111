// cfz_planning.hip -- the planning half of libconfrez_hip.so: Vehicle.state_ws (reference confrez/control/vehicle.py:99-231),
// the single-vehicle collocation plan (vehicle.py:360-661) and the joint plan of several vehicles
// (multi_vehicle_planner.py:343-480) as gfx950 kernels, with their C ABI entry points (include/confrez_hip.h).
// Kernel bodies: cfz_plan.inl, cfz_colloc.inl, cfz_band.inl; the separation-certificate geometry is shared with the MPC
// step (cfz_solver.inl).  Both translation units are built at -O3 (__graft_entry__.build).

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <cstdlib>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/confrez_hip.h"
#include "cfz_common.h"
#include "cfz_solver.inl"
#include "cfz_plan.inl"
#include "cfz_colloc.inl"

namespace {

// state_ws (reference vehicle.py:99-231): one planning NLP per workgroup of four wavefronts, workspace in global memory; see cfz_plan.inl.
// bound 512 = at most 256 VGPRs, no AGPRs: see colloc_kernel
// FAST: the sweep's per-stage data in dynamic LDS (41 (T + 1) doubles); otherwise in the workspace (plans too long for the LDS).
template <bool FAST>
__global__ __launch_bounds__(512) void state_ws_kernel(int B, const cfzp::PSpec *specs, const double *tube, const long long *tube_off, double *X,
                                const long long *x_off, double *slab, const long long *slab_off, int32_t *oi, double *od) {
  const int b = blockIdx.x;
  if (b >= B) return;
  // all 256 lanes run the solver's scalar logic redundantly and share the marked loops; the Riccati sweep is lane 0's (cfz_plan.inl)
  cfzp::solve_state_ws<FAST>(specs[b], tube + tube_off[b], X + x_off[b], slab + slab_off[b], oi + 2 * b, od + 3 * b);
}

// Collocation plans (reference vehicle.py:360-661 single, multi_vehicle_planner.py:343-480 joint): one NLP per workgroup of 512 threads,
// workspace in global memory, elimination from global memory a panel at a time; see cfz_colloc.inl.
// bound 512: with 64 (or 256) the register allocator may use AGPRs beyond 256 VGPRs, and every such build of this kernel died with
// HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION on gfx950 / ROCm 7.2 while the 256-VGPR builds of the same source run.
__global__ __launch_bounds__(512) void colloc_kernel(int B, const cfzc::CSpec *specs, double *X, const long long *x_off, double *slab,
                              const long long *slab_off, const int32_t *kbs, int32_t *oi, double *od, int lds_doubles, int lds_rhs) {
  const int b = blockIdx.x;
  // dynamic LDS (lds_doubles): the multipliers of a panel during the elimination; lds_rhs (<= lds_doubles, 0 = none): room for one
  // right-hand side of the fallback substitution
  if (b >= B) return;
  cfzc::solve_colloc<2>(specs[b], X + x_off[b], slab + slab_off[b], kbs[b], oi + 2 * b, od + cfzc::kOutD * b, lds_doubles, lds_rhs);
}

}  // namespace

struct cfz_plan_ws {
  int device = 0;
  hipStream_t stream = nullptr;
  CfzArena arena;
};

namespace {
// the workspace behind the handle-less entry points: one per (thread, device), created on first use, kept for the life of
// the thread (so that a caller of the plain signatures also stops paying hipMalloc/hipFree per call)
thread_local std::vector<cfz_plan_ws *> g_default_ws;  // (not destroyed at thread exit: the HIP runtime may be gone by then; cfz_plan_ws_trim(NULL) gives the memory back)
cfz_plan_ws *default_ws(int device) {
  std::vector<cfz_plan_ws *> &cache = g_default_ws;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { fail("no HIP device: libconfrez_hip has no CPU path"); return nullptr; }
  if (device < 0 || device >= ndev) { fail("device index out of range"); return nullptr; }
  if ((int)cache.size() <= device) cache.resize(device + 1, nullptr);
  if (!cache[device] && cfz_plan_ws_create(device, &cache[device]) != 0) return nullptr;
  return cache[device];
}

// ---- the host-side rules of the planning entry points, each stated once ----
// The LDS a workgroup may own.  gfx950: the whole LDS of its CU (160 KB); some runtimes report the smaller legacy figure per block.
int lds_per_workgroup(int device, int *bytes) {
  int per_cu = 0;
  HIP_OK(hipDeviceGetAttribute(bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
  if (hipDeviceGetAttribute(&per_cu, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device) == hipSuccess) *bytes = std::max(*bytes, per_cu);
  return 0;
}

// The interior-point constants the state_ws and the collocation specs share.  reg_dual, the stall exit and everything the option
// structs carry stay with the callers.
template <class Spec>
void set_ip_constants(Spec &p) {
  p.max_backtrack = 25; p.filter_cap = 16; p.dual_inf_tol = 1.0; p.compl_inf_tol = 1e-4;
  p.kappa_eps = 10.0; p.kappa_mu = 0.2; p.theta_mu = 1.5; p.tau_min = 0.99; p.bound_push = 1e-2; p.bound_frac = 1e-2; p.s_max = 100.0;
  p.kappa_sigma = 1e10; p.eta_phi = 1e-8; p.gamma_theta = 1e-5; p.gamma_phi = 1e-8; p.delta_sw = 1.0; p.s_theta = 1.1; p.s_phi = 2.3;
  p.reg_primal = 1e-8;
}

typedef std::vector<std::pair<int, int>> PairList;

// The pair rule: a separation row joins vehicles 0 <= a < b < V.
bool pair_ok(int a, int b, int V) { return 0 <= a && a < b && b < V; }

// The pair list of a joint plan of V vehicles: the n_pairs given, or every pair when pairs is NULL (multi_vehicle_planner.py:56-58).
int parse_pairs(int V, int n_pairs, const int32_t *pairs, PairList &pr) {
  if (pairs && V < 2) return fail("vehicle pairs need at least two vehicles");
  if (pairs) for (int e = 0; e < n_pairs; ++e) {
    if (!pair_ok(pairs[2 * e], pairs[2 * e + 1], V)) return fail("bad vehicle pair");
    pr.push_back({pairs[2 * e], pairs[2 * e + 1]});
  }
  else for (int a = 0; a < V; ++a) for (int b = a + 1; b < V; ++b) pr.push_back({a, b});
  return 0;
}

// The shape of a collocation problem: vehicles, intervals per vehicle, obstacles, pairs.  has_final(a): whether vehicle a ends on a given
// heading -- the solve paths ask the heading itself, the info path its argument.  Refuses what its array writes cannot hold.
template <class HasFinal>
int fill_shape(cfzc::CSpec &p, int V, const int32_t *n_sets, HasFinal has_final, int N_per_set, int n_obs, const PairList &pr) {
  if (V < 1 || V > cfzc::kMaxVeh || (int)pr.size() > cfzc::kMaxPairs) return fail("problem size outside compiled limits");
  p.V = V; p.Nps = N_per_set; p.n_obs = n_obs; p.n_pairs = (int)pr.size();
  for (int a = 0; a < V; ++a) {
    if (n_sets[a] < 2) return fail("a plan needs at least two strategy steps");
    p.n_chk[a] = n_sets[a] - 1; p.N[a] = N_per_set * p.n_chk[a]; p.has_final[a] = has_final(a);
  }
  for (int e = 0; e < p.n_pairs; ++e) {
    if (!pair_ok(pr[e].first, pr[e].second, V)) return fail("bad vehicle pair");
    p.pair_a[e] = pr[e].first; p.pair_b[e] = pr[e].second;
  }
  return 0;
}

// Which elimination a plan of this shape goes through: bit 2 of CSpec::no_prox, the structured one (cfz_struct.inl, cfz_jstruct.inl),
// unless the pivots are wanted one at a time or a vehicle has more than 255 intervals (its interval count is packed into eight bits).
// Decided on the host, where the slab is sized and the roofline is priced, not discovered on the device.
int structured_bit(int structured, int one_pivot, const cfzc::CSpec &shape) {
  if (!structured || one_pivot) return 0;
  for (int a = 0; a < shape.V; ++a) if (shape.N[a] > 255) return 0;
  return 4;
}

// half-bandwidth of a problem's ordering (51 for one vehicle); < 0: refused
int half_bandwidth_of(const cfzc::CSpec &p) {
  const cfzc::CDims d = cfzc::cdims(p);
  std::vector<int> pos((size_t)d.n + d.m);
  if (cfzc::build_order(p, pos.data(), pos.data() + d.n) != d.nk) return fail("internal: ordering does not cover the band system");
  return cfzc::half_bandwidth(p, pos.data(), pos.data() + d.n);
}
}  // namespace

extern "C" {

int cfz_plan_ws_create(int device, cfz_plan_ws **out) {
  if (!out) return fail("null argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail("no HIP device: libconfrez_hip has no CPU path");
  if (device < 0 || device >= ndev) return fail("device index out of range");
  HIP_OK(hipSetDevice(device));
  cfz_plan_ws *w = new cfz_plan_ws();
  w->device = device;
  if (hipStreamCreate(&w->stream) != hipSuccess) { delete w; return fail("hipStreamCreate"); }
  *out = w;
  return 0;
}

int cfz_plan_ws_trim(cfz_plan_ws *w) {
  if (w) { (void)hipSetDevice(w->device); HIP_OK(hipStreamSynchronize(w->stream)); arena_destroy(w->arena); return 0; }
  for (cfz_plan_ws *d : g_default_ws) if (d) { (void)hipSetDevice(d->device); HIP_OK(hipStreamSynchronize(d->stream)); arena_destroy(d->arena); }
  return 0;
}

int cfz_plan_ws_destroy(cfz_plan_ws *w) {
  if (!w) return 0;
  (void)hipSetDevice(w->device);
  if (w->stream) (void)hipStreamDestroy(w->stream);
  delete w;  // (the arena's blocks go with it)
  return 0;
}

// mean of the vertices of the cell A[4][2] p <= b[4] (pairs of non-parallel rows whose intersection satisfies every row)
static bool cell_centre(const double *cell, double c[2]) {
  const double *A = cell, *b = cell + 8;
  double sx = 0.0, sy = 0.0; int nv = 0;
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j) {
      const double det = A[2 * i] * A[2 * j + 1] - A[2 * i + 1] * A[2 * j];
      if (fabs(det) < 1e-9) continue;
      const double x = (b[i] * A[2 * j + 1] - A[2 * i + 1] * b[j]) / det, y = (A[2 * i] * b[j] - b[i] * A[2 * j]) / det;
      bool in = true;
      for (int r = 0; r < 4; ++r) if (A[2 * r] * x + A[2 * r + 1] * y > b[r] + 1e-9) in = false;
      if (in) { sx += x; sy += y; ++nv; }
    }
  if (!nv) return false;
  c[0] = sx / nv; c[1] = sy / nv;
  return true;
}

int cfz_state_ws_default_guess(int32_t n_sets, int32_t N, const double init_pose[3], double final_heading, const double *tube, double *guess) {
  if (n_sets < 2 || N < 1 || !init_pose || !tube || !guess) return fail("bad argument");
  const int S = n_sets;
  std::vector<double> cx(S), cy(S), hd(S);
  cx[0] = init_pose[0]; cy[0] = init_pose[1]; hd[0] = init_pose[2];
  const double two_pi = 6.283185307179586;
  for (int i = 1; i < S; ++i) {
    double cb[2], cf[2];
    const double *cell = tube + (size_t)(i - 1) * 24;
    const bool okb = cell_centre(cell, cb), okf = cell_centre(cell + 12, cf);
    cx[i] = okb ? cb[0] : cx[i - 1]; cy[i] = okb ? cb[1] : cy[i - 1];
    double h = (okb && okf && (cf[0] != cb[0] || cf[1] != cb[1])) ? atan2(cf[1] - cb[1], cf[0] - cb[0]) : hd[i - 1];
    h += two_pi * nearbyint((hd[i - 1] - h) / two_pi);  // the branch nearest the previous heading
    hd[i] = h;
  }
  if (final_heading == final_heading) hd[S - 1] = final_heading + two_pi * nearbyint((hd[S - 1] - final_heading) / two_pi);
  const int T = N * (S - 1);
  for (int k = 0; k <= T; ++k) {
    const int i = k / N < S - 1 ? k / N : S - 2;
    const double t = (double)(k - i * N) / N;
    guess[3 * k] = cx[i] + t * (cx[i + 1] - cx[i]); guess[3 * k + 1] = cy[i] + t * (cy[i + 1] - cy[i]); guess[3 * k + 2] = hd[i] + t * (hd[i + 1] - hd[i]);
  }
  // the terminal heading is imposed exactly: the guess ends on it (its branch was chosen above; the NLP takes the value given)
  return 0;
}

int cfz_state_ws(int device, int B, const cfz_plan_options *po, const int32_t *n_sets, const double *init_pose,
                 const double *final_heading, const double *tube, const double *guess, double *traj, int32_t *status,
                 int32_t *iters, double *cost) {
  cfz_plan_ws *w = default_ws(device);
  if (!w) return -1;
  return cfz_state_ws_w(w, B, po, n_sets, init_pose, final_heading, tube, guess, traj, status, iters, cost);
}

int cfz_state_ws_w(cfz_plan_ws *w, int B, const cfz_plan_options *po, const int32_t *n_sets, const double *init_pose,
                   const double *final_heading, const double *tube, const double *guess, double *traj, int32_t *status,
                   int32_t *iters, double *cost) {
  if (!w) return fail("null workspace");
  if (B < 1 || !po || !n_sets || !init_pose || !tube || !traj) return fail("bad argument");
  HIP_OK(hipSetDevice(w->device));
  if (arena_reset(w->arena)) return -1;
  hipStream_t st = w->stream;
  std::vector<cfzp::PSpec> specs(B);
  std::vector<long long> off((size_t)3 * B);  // per plan: where its tube, its unknowns and its workspace begin
  long long *toff = off.data(), *xoff = toff + B, *soff = xoff + B;
  long long nt = 0, nx = 0, ns = 0, npts = 0;
  for (int b = 0; b < B; ++b) {
    if (n_sets[b] < 2 || po->N < 1) return fail("a plan needs at least two strategy steps");
    if (po->kernel < CFZ_KERNEL_AUTO || po->kernel > CFZ_KERNEL_NARROW) return fail("cfz_plan_options.kernel: 0 (by batch size), 1 (wide) or 2 (narrow)");
    cfzp::PSpec &p = specs[b];
    memset(&p, 0, sizeof p);
    p.N = po->N; p.n_chk = n_sets[b] - 1; p.T = po->N * p.n_chk;
    p.has_final = final_heading && final_heading[b] == final_heading[b]; p.final_heading = p.has_final ? final_heading[b] : 0.0;
    p.bounded_input = po->bounded_input;
    set_ip_constants(p);
    p.max_iter = po->max_iter; p.stall_iters = po->stall_iters;
    p.dt = po->dt; p.wb = po->wb; p.shrink = po->shrink_tube;
    for (int i = 0; i < 3; ++i) p.init_pose[i] = init_pose[b * 3 + i];
    memcpy(p.bounds, po->bounds, sizeof p.bounds);
    p.tol = po->tol; p.constr_viol_tol = po->constr_viol_tol; p.mu_init = po->mu_init;
    p.reg_dual = 1e-9; p.curv_kappa = po->curv_kappa; p.stall_kappa = 0.9;
    toff[b] = nt; xoff[b] = nx; soff[b] = ns;
    nt += (long long)p.n_chk * 24; nx += cfzp::dims(p).n; ns += (long long)cfzp::work_doubles(p); npts += p.T + 1;
  }
  // initial guess: x, y, psi of every stage (vehicle.py:199-205), everything else zero
  std::vector<double> X((size_t)nx, 0.0);
  // no guess from the caller (spline_ws = False): the path through the tube's cells, cfz_state_ws_default_guess -- the standing start
  // (every stage at the initial pose) is rank deficient once a terminal heading is fixed and failed on every vehicle of the strategy
  std::vector<double> own;
  if (!guess) {
    own.resize((size_t)npts * 3);
    long long o = 0;
    for (int b = 0; b < B; ++b) {
      if (cfz_state_ws_default_guess(n_sets[b], po->N, init_pose + 3 * b, specs[b].has_final ? specs[b].final_heading : NAN, tube + toff[b], own.data() + o * 3)) return -1;
      o += specs[b].T + 1;
    }
    guess = own.data();
  }
  long long g0 = 0;
  for (int b = 0; b < B; ++b) {
    const int T = specs[b].T;
    {
      for (int k = 0; k <= T; ++k) for (int c = 0; c < 3; ++c) X[(size_t)xoff[b] + 7 * k + c] = guess[(size_t)(g0 + k) * 3 + c];
      // The reference seeds x, y, psi only.  With v = 0 everywhere the heading rows of the linearisation have no control
      // authority (rank deficient once a terminal heading is fixed); the signed speed along the guessed path costs
      // nothing and takes the solver from 14-150 iterations (one failure) to 8-35 on the four-vehicle strategy.
      for (int k = 1; k < T; ++k) {
        const double *p0 = guess + (size_t)(g0 + k) * 3, *p1 = p0 + 3;
        const double dx = p1[0] - p0[0], dy = p1[1] - p0[1], along = dx * cos(p0[2]) + dy * sin(p0[2]);
        X[(size_t)xoff[b] + 7 * k + 3] = (along > 0.0 ? 1.0 : (along < 0.0 ? -1.0 : 0.0)) * sqrt(dx * dx + dy * dy) / po->dt;
      }
    }
    g0 += T + 1;
  }
  cfzp::PSpec *dspec = nullptr; double *dtube = nullptr, *dX = nullptr, *dslab = nullptr, *dod = nullptr;
  long long *doff = nullptr; int32_t *doi = nullptr;
  ARENA_ALLOC(w->arena, dspec, sizeof(cfzp::PSpec) * B); ARENA_ALLOC(w->arena, dtube, (size_t)nt * 8); ARENA_ALLOC(w->arena, dX, (size_t)nx * 8);
  ARENA_ALLOC(w->arena, dslab, (size_t)ns * 8); ARENA_ALLOC(w->arena, doff, (size_t)B * 3 * 8); ARENA_ALLOC(w->arena, doi, (size_t)B * 2 * 4);
  ARENA_ALLOC(w->arena, dod, (size_t)B * 3 * 8);
  // everything on the workspace's stream (the host arrays are pageable: each copy returns when its source is free again)
  HIP_OK(hipMemcpyAsync(dspec, specs.data(), sizeof(cfzp::PSpec) * B, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(dtube, tube, (size_t)nt * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(dX, X.data(), (size_t)nx * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(doff, off.data(), (size_t)B * 3 * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(dslab, 0, (size_t)ns * 8, st));
  // cfz_plan_options.kernel: WIDE = the sweep's per-stage data in LDS (one plan per CU at a time, 15 % faster per plan), NARROW = in the
  // workspace (several plans share a CU: 1024 plans take 0.13 s instead of 0.20 s); by default LDS while the batch fits the CUs in one
  // round.  A plan too long for the LDS (376 bytes per stage: T > ~430) runs from the workspace whatever was asked.
  int Tmax = 0, lds_max = 0, cus = 0;
  for (int b = 0; b < B; ++b) Tmax = std::max(Tmax, specs[b].T);
  const size_t lds_bytes = (size_t)(cfzp::kSt + cfzp::kFb) * (Tmax + 1) * sizeof(double);
  hipFuncAttributes fa;
  HIP_OK(hipFuncGetAttributes(&fa, (const void *)state_ws_kernel<true>));
  if (lds_per_workgroup(w->device, &lds_max)) return -1;
  HIP_OK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, w->device));
  const bool want_lds = po->kernel == CFZ_KERNEL_WIDE || (po->kernel == CFZ_KERNEL_AUTO && B <= cus);
  const bool fast = want_lds && lds_bytes + fa.sharedSizeBytes <= (size_t)lds_max &&
                    hipFuncSetAttribute((const void *)state_ws_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) == hipSuccess;
  // Four wavefronts per plan in either mode (the same reductions, the same bits): the marked loops split over 256 lanes, the sweeps stay
  // one lane's.  Measured (wall, 256 / 1024 / 2048 plans): 64 threads 34 / 100 / 115 ms, 128: 30 / 70 / 132, 256: 27 / 101 / 159 -- taken for
  // BASELINE's batch of 256.
  const int swt = 256;
  if (fast) hipLaunchKernelGGL(state_ws_kernel<true>, dim3(B), dim3(swt), lds_bytes, st, B, dspec, dtube, doff, dX, doff + B, dslab, doff + 2 * B, doi, dod);
  else { (void)hipGetLastError(); hipLaunchKernelGGL(state_ws_kernel<false>, dim3(B), dim3(swt), 0, st, B, dspec, dtube, doff, dX, doff + B, dslab, doff + 2 * B, doi, dod); }
  HIP_OK(hipGetLastError());
  std::vector<int32_t> oi((size_t)B * 2); std::vector<double> od((size_t)B * 3);
  HIP_OK(hipMemcpyAsync(X.data(), dX, (size_t)nx * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(oi.data(), doi, (size_t)B * 2 * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(od.data(), dod, (size_t)B * 3 * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));  // this stream only: other streams of the process (torch's) keep running
  long long o = 0;
  for (int b = 0; b < B; ++b) {
    const int T = specs[b].T;
    for (int k = 0; k <= T; ++k) {
      const int ku = k < T ? k : T - 1;  // the last input is repeated (vehicle.py:226-229)
      for (int c = 0; c < 5; ++c) traj[(size_t)(o + k) * 7 + c] = X[(size_t)xoff[b] + 7 * k + c];
      for (int c = 5; c < 7; ++c) traj[(size_t)(o + k) * 7 + c] = X[(size_t)xoff[b] + 7 * ku + c];
    }
    o += T + 1;
    if (status) status[b] = oi[2 * b + 1];
    if (iters) iters[b] = oi[2 * b];
    if (cost) cost[b] = od[3 * b];
  }
  return 0;
}

// Lagrange basis on tau = [0, Radau IIA points of degree 5]: A[j][k] = l_j'(tau_k), B[j] = int_0^1 l_j (vehicle.py:54-97)
static void radau5_tables(double A[6][6], double B[6]) {
  const double tau[6] = {0.0, 0.05710419611451768, 0.2768430136381238, 0.5835904323689168, 0.8602401356562195, 1.0};
  for (int j = 0; j < 6; ++j) {
    double c[7] = {1.0, 0, 0, 0, 0, 0, 0};  // coefficients of l_j, ascending powers
    int deg = 0;
    for (int m = 0; m < 6; ++m) {
      if (m == j) continue;
      const double den = tau[j] - tau[m];
      for (int q = deg + 1; q >= 0; --q) c[q] = ((q > 0 ? c[q - 1] : 0.0) - tau[m] * (q <= deg ? c[q] : 0.0)) / den;
      ++deg;
    }
    B[j] = 0.0;
    for (int q = 0; q <= deg; ++q) B[j] += c[q] / (q + 1);
    for (int k = 0; k < 6; ++k) {
      double dv = 0.0, pw = 1.0;
      for (int q = 1; q <= deg; ++q) { dv += q * c[q] * pw; pw *= tau[k]; }
      A[j][k] = dv;
    }
  }
}

// B collocation problems in one launch; problem b plans nveh[b] vehicles with one shared dt (1: the single-vehicle plan).
// Vehicles are numbered through all problems: n_sets, init_pose, final_heading, tube, guess and traj are per vehicle,
// dt0, dt, status, iters, cost per problem; pairs[b]: vehicle pairs (local indices) with a separation row, per problem.
static int colloc_run(cfz_plan_ws *w, int B, const int32_t *nveh, const std::vector<PairList> &pairs, const cfz_spec *spec,
                      const cfz_colloc_options *co, const int32_t *n_sets, const double *init_pose, const double *final_heading,
                      const double *tube, const double *guess, const double *dt0, double *traj, double *dt, int32_t *status,
                      int32_t *iters, double *cost) {
  if (!w) return fail("null workspace");
  if (spec->n_obs < 0 || spec->n_obs > cfzc::kMaxObs || co->N_per_set < 1) return fail("problem size outside compiled limits");
  if (co->kernel != CFZ_KERNEL_AUTO) return fail("cfz_colloc_options.kernel: retired with the one-wavefront collocation kernel (round 4); leave it 0");
  if (co->structured != 0 && co->structured != 1) return fail("cfz_colloc_options.structured must be 0 (band) or 1 (cfz_jstruct.inl); 2, round 4's scheme, was removed in round 6");
  const bool profile = std::getenv("CFZ_COLLOC_PROFILE") != nullptr;  // per-phase clocks of every plan on stderr
  HIP_OK(hipSetDevice(w->device));
  if (arena_reset(w->arena)) return -1;
  hipStream_t st = w->stream;
  std::vector<double> tab((size_t)std::max(spec->n_obs, 1) * 20, 0.0);
  for (int j = 0; j < spec->n_obs; ++j) {
    double V[4][2];
    if (!quad_vertices(spec->A_obs[j], spec->b_obs[j], V)) return fail("obstacle is not a bounded quadrilateral");
    double *o = tab.data() + (size_t)j * 20;
    for (int i = 0; i < 4; ++i) { o[2 * i] = spec->A_obs[j][i][0]; o[2 * i + 1] = spec->A_obs[j][i][1]; o[8 + i] = spec->b_obs[j][i];
                                  o[12 + 2 * i] = V[i][0]; o[13 + 2 * i] = V[i][1]; }
  }
  std::vector<cfzc::CSpec> specs(B);
  long long nt = 0;
  for (int b = 0, v0 = 0; b < B; v0 += nveh[b++]) {  // every problem's shape first: it sizes the tube
    cfzc::CSpec &p = specs[b];
    memset(&p, 0, sizeof p);
    if (fill_shape(p, nveh[b], n_sets + v0, [&](int a) { return final_heading && final_heading[v0 + a] == final_heading[v0 + a]; },
                   co->N_per_set, spec->n_obs, pairs[b])) return -1;
    for (int a = 0; a < p.V; ++a) nt += (long long)p.n_chk[a] * 24;
  }
  double *dtab = nullptr, *dtube = nullptr;
  ARENA_ALLOC(w->arena, dtab, tab.size() * 8); ARENA_ALLOC(w->arena, dtube, (size_t)nt * 8);
  HIP_OK(hipMemcpyAsync(dtab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(dtube, tube, (size_t)nt * 8, hipMemcpyHostToDevice, st));
  std::vector<long long> off((size_t)2 * B);  // per problem: where its unknowns and its workspace begin
  long long *xoff = off.data(), *soff = xoff + B;
  std::vector<int32_t> kbs(B);
  long long nx = 0, ns = 0, to = 0;
  int v0 = 0;
  for (int b = 0; b < B; ++b) {
    cfzc::CSpec &p = specs[b];
    long long npts = 0;
    for (int a = 0; a < p.V; ++a) {
      const int v = v0 + a;
      p.final_heading[a] = p.has_final[a] ? final_heading[v] : 0.0;
      for (int i = 0; i < 3; ++i) p.init_pose[a][i] = init_pose[v * 3 + i];
      p.tube[a] = dtube + to; to += (long long)p.n_chk[a] * 24;
      npts += (long long)p.N[a] * cfzc::kPts;
    }
    set_ip_constants(p);
    p.max_iter = co->max_iter;
    p.wb = spec->wb; p.dmin = spec->dmin; p.shrink = co->shrink_tube; p.dt0 = dt0[b];
    memcpy(p.bounds, spec->bounds, sizeof p.bounds); memcpy(p.g, spec->g, sizeof p.g);
    radau5_tables(p.A, p.B);
    p.tol = co->tol; p.constr_viol_tol = co->constr_viol_tol; p.mu_init = co->mu_init;
    // delta_c = 1e-7 of proximal type (cfz_colloc.inl): while a vehicle stands still with its heading along an axis, the
    // six ODE rows of x (or y) of an interval only see the rank-5 derivative matrix and their multipliers are not
    // determined.  Measured on the synthetic strategy: IPOPT's form of delta_c needs 288 iterations at 1e-9, 38 at 1e-7
    // and 30 at 3e-6 for the vehicle that waits, and leaves three of the four joint test problems unconverged at any
    // value; the proximal form solves all of them in 26-38 iterations at 1e-7, where the rows are met to ~2e-4 and the
    // cost is 0.65 % below the delta_c = 1e-9 value (constr_viol_tol is 1e-2, vehicle.py:651).
    p.reg_dual = co->exact_rows ? 1e-9 : 1e-7; p.no_prox = (co->exact_rows ? 1 : 0) | (co->one_pivot ? 2 : 0) | structured_bit(co->structured, co->one_pivot, p);
    p.vv_rows = co->vv_rows ? 1 : 0; p.curv_kappa = co->curv_kappa;
    p.obs_tab = dtab;
    if ((kbs[b] = half_bandwidth_of(p)) < 0) return -1;
    xoff[b] = nx; nx += 7 * npts + 1;
    soff[b] = ns; ns += (long long)cfzc::work_doubles(p, kbs[b]);
    v0 += p.V;
  }
  std::vector<double> X((size_t)nx);
  long long g0 = 0;
  for (int b = 0; b < B; ++b) {  // guess: x, y, psi, v, delta, a, w at every point (:629-636), dt0 (:388-389)
    const long long np_ = (long long)cfzc::cdims(specs[b]).np;
    memcpy(X.data() + xoff[b], guess + g0 * 7, (size_t)np_ * 7 * 8);
    X[(size_t)(xoff[b] + 7 * np_)] = dt0[b];
    g0 += np_;
  }
  cfzc::CSpec *dspec = nullptr; double *dX = nullptr, *dslab = nullptr, *dod = nullptr; long long *doff = nullptr; int32_t *doi = nullptr, *dkb = nullptr;
  ARENA_ALLOC(w->arena, dspec, sizeof(cfzc::CSpec) * B); ARENA_ALLOC(w->arena, dX, (size_t)nx * 8); ARENA_ALLOC(w->arena, dslab, (size_t)ns * 8);
  ARENA_ALLOC(w->arena, doff, (size_t)B * 2 * 8); ARENA_ALLOC(w->arena, doi, (size_t)B * 2 * 4); ARENA_ALLOC(w->arena, dod, (size_t)B * cfzc::kOutD * 8);
  ARENA_ALLOC(w->arena, dkb, (size_t)B * 4);
  HIP_OK(hipMemcpyAsync(dspec, specs.data(), sizeof(cfzc::CSpec) * B, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(dX, X.data(), (size_t)nx * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(doff, off.data(), (size_t)B * 2 * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(dkb, kbs.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(dslab, 0, (size_t)ns * 8, st));
  // One kernel: 512 threads per plan, band in global memory, panel elimination (`one_pivot`: one pivot at a time, the check of the
  // panel).  Rounds 1-3 also had a one-wavefront kernel with the elimination in an LDS window for batches of more than two plans per CU
  // (cfz_colloc_options.kernel = CFZ_KERNEL_NARROW).  Round 4 retired it: its 124 KB window let one plan run per CU just as here, so it
  // was the slower one at every batch size (1024 plans: 3.25 s against 1.83 s, 2048: 5.67 s against 3.80 s), and after a recompile that
  // left its source untouched it returned, for identical plans of one batch, two or three different results (2e-5 apart in the
  // trajectory; 7 of 1024 plans no longer converged) -- a race that no placement of barriers in its elimination removed reliably
  // (docs/notebook.md).  `kernel` is still accepted (0, 1, 2) and means nothing.
  {
    // Dynamic LDS beside the kernel's static arrays (read from the code object, not assumed): the panel's multipliers
    // (kPanel x (kb + kPanel) doubles, <= 58 KB) must fit; a right-hand side of the largest instance rides along only if it
    // fits as well (it serves band_substitute_wide, the fallback substitution) -- the panel path does not depend on it.
    int nk_max = 0, kb_max = 0, lds_max = 0;
    for (int b = 0; b < B; ++b) { nk_max = std::max(nk_max, cfzc::cdims(specs[b]).nk); kb_max = std::max(kb_max, (int)kbs[b]); }
    hipFuncAttributes fa;
    HIP_OK(hipFuncGetAttributes(&fa, (const void *)colloc_kernel));
    if (lds_per_workgroup(w->device, &lds_max)) return -1;
    if (profile) fprintf(stderr, "cfz_colloc: LDS per workgroup %d B, static %zu B\n", lds_max, (size_t)fa.sharedSizeBytes);
    const long long avail = ((long long)lds_max - (long long)fa.sharedSizeBytes) / 8;
    const long long pl = kb_max <= cfzc::kWideMaxKb ? (long long)cfzc::kPanel * (kb_max + cfzc::kPanel) : 0;
    const int lds_rhs = nk_max <= avail ? nk_max : 0;
    int lds_doubles = (int)std::max<long long>(pl <= avail ? pl : 0, lds_rhs), lds_rhs_ = lds_rhs;
    // the structured eliminations' 64-row blocks on the matrix cores stage their operands in LDS: kLuLdsWave doubles for each of the eight
    // wavefronts (68 KB); no fallback (gfx950 gives a workgroup the CU's 160 KB)
    bool any_j = false;
    for (int b = 0; b < B; ++b) any_j = any_j || cfzc::jstruct_mode(specs[b]);
    if (any_j) {
      if (8LL * cfzc::kLuLdsWave > avail) return fail("the structured elimination needs 8 x kLuLdsWave doubles of LDS per workgroup");
      lds_doubles = std::max(lds_doubles, 8 * cfzc::kLuLdsWave);
    }
    if (lds_doubles && hipFuncSetAttribute((const void *)colloc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_doubles * 8) != hipSuccess) {
      // a runtime whose per-workgroup limit really is the smaller figure: the kernel also runs without dynamic LDS
      (void)hipGetLastError();
      if (any_j) return fail("hipFuncSetAttribute: the dynamic LDS of the structured elimination was refused");
      lds_doubles = 0; lds_rhs_ = 0;
    }
    hipLaunchKernelGGL(colloc_kernel, dim3(B), dim3(512), (size_t)lds_doubles * 8, st, B, dspec, dX, doff, dslab, doff + B, dkb, doi, dod, lds_doubles, lds_rhs_);
  }
  HIP_OK(hipGetLastError());
  std::vector<int32_t> oi((size_t)B * 2); std::vector<double> od((size_t)B * cfzc::kOutD);
  HIP_OK(hipMemcpyAsync(X.data(), dX, (size_t)nx * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(oi.data(), doi, (size_t)B * 2 * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(od.data(), dod, (size_t)B * cfzc::kOutD * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  g0 = 0;
  for (int b = 0; b < B; ++b) {
    const long long np_ = (long long)cfzc::cdims(specs[b]).np;
    memcpy(traj + g0 * 7, X.data() + xoff[b], (size_t)np_ * 7 * 8);
    dt[b] = X[(size_t)(xoff[b] + 7 * np_)];
    g0 += np_;
    if (status) status[b] = oi[2 * b + 1];
    if (iters) iters[b] = oi[2 * b];
    if (cost) cost[b] = od[(size_t)cfzc::kOutD * b];
    if (profile) {  // milliseconds per phase (100 MHz device clock)
      const double *t = od.data() + (size_t)cfzc::kOutD * b + 3;
      fprintf(stderr, "cfz_colloc[%d]: %d vehicle(s), half-bandwidth %d, %d iterations, evaluate %.2f assemble %.2f factor %.2f substitute %.2f line search %.2f total %.2f ms (factor: panel / pivot search %.2f test / swap %.2f trailing columns / update %.2f)\n",
              b, specs[b].V, kbs[b], oi[2 * b], t[0] * 1e-5, t[1] * 1e-5, t[2] * 1e-5, t[3] * 1e-5, t[4] * 1e-5, t[5] * 1e-5, t[6] * 1e-5, t[7] * 1e-5, t[8] * 1e-5);
      if (cfzc::jstruct_mode(specs[b]))
        fprintf(stderr, "cfz_colloc[%d]: joint structured elimination: interiors %.2f | C'W, pair blocks %.2f capacitance matrices %.2f their solves %.2f Z %.2f separator blocks %.2f Schur complements %.2f | recursion %.2f back-substitution %.2f ms\n",
                b, t[6] * 1e-5, t[9] * 1e-5, t[10] * 1e-5, t[11] * 1e-5, t[12] * 1e-5, t[13] * 1e-5, t[14] * 1e-5, t[15] * 1e-5, t[16] * 1e-5);
    }
  }
  return 0;
}

int cfz_colloc(int device, int B, const cfz_spec *spec, const cfz_colloc_options *co, const int32_t *n_sets,
               const double *init_pose, const double *final_heading, const double *tube, const double *guess,
               const double *dt0, double *traj, double *dt, int32_t *status, int32_t *iters, double *cost) {
  cfz_plan_ws *w = default_ws(device);
  if (!w) return -1;
  return cfz_colloc_w(w, B, spec, co, n_sets, init_pose, final_heading, tube, guess, dt0, traj, dt, status, iters, cost);
}

int cfz_colloc_w(cfz_plan_ws *w, int B, const cfz_spec *spec, const cfz_colloc_options *co, const int32_t *n_sets,
                 const double *init_pose, const double *final_heading, const double *tube, const double *guess,
                 const double *dt0, double *traj, double *dt, int32_t *status, int32_t *iters, double *cost) {
  if (B < 1 || !spec || !co || !n_sets || !init_pose || !tube || !guess || !dt0 || !traj || !dt) return fail("bad argument");
  std::vector<int32_t> one((size_t)B, 1);
  std::vector<PairList> none((size_t)B);
  return colloc_run(w, B, one.data(), none, spec, co, n_sets, init_pose, final_heading, tube, guess, dt0, traj, dt, status, iters, cost);
}

int cfz_joint_colloc(int device, int B, int V, const cfz_spec *spec, const cfz_colloc_options *co, const int32_t *n_sets,
                     const double *init_pose, const double *final_heading, const double *tube, const double *guess, const double *dt0,
                     int n_pairs, const int32_t *pairs, double *traj, double *dt, int32_t *status, int32_t *iters, double *cost) {
  cfz_plan_ws *w = default_ws(device);
  if (!w) return -1;
  return cfz_joint_colloc_w(w, B, V, spec, co, n_sets, init_pose, final_heading, tube, guess, dt0, n_pairs, pairs, traj, dt, status, iters, cost);
}

int cfz_joint_colloc_w(cfz_plan_ws *w, int B, int V, const cfz_spec *spec, const cfz_colloc_options *co, const int32_t *n_sets,
                       const double *init_pose, const double *final_heading, const double *tube, const double *guess, const double *dt0,
                       int n_pairs, const int32_t *pairs, double *traj, double *dt, int32_t *status, int32_t *iters, double *cost) {
  if (B < 1 || V < 1 || !spec || !co || !n_sets || !init_pose || !tube || !guess || !dt0 || !traj || !dt || n_pairs < 0) return fail("bad argument");
  PairList pr;
  if (parse_pairs(V, n_pairs, pairs, pr)) return -1;
  std::vector<PairList> all((size_t)B, pr);
  std::vector<int32_t> nv((size_t)B, V);
  return colloc_run(w, B, nv.data(), all, spec, co, n_sets, init_pose, final_heading, tube, guess, dt0, traj, dt, status, iters, cost);
}

int cfz_colloc_band_info(int V, const int32_t *n_sets, const int32_t *has_final, int N_per_set, int n_obs, int n_pairs,
                         const int32_t *pairs, int32_t *nk, int32_t *kb, int64_t *band_bytes) {
  if (V < 1 || V > cfzc::kMaxVeh || !n_sets || N_per_set < 1 || n_obs < 0 || n_obs > cfzc::kMaxObs || n_pairs < 0) return fail("bad argument");
  return cfz_colloc_elimination_info(V, n_sets, has_final, N_per_set, n_obs, n_pairs, pairs, 0, nk, kb, band_bytes, nullptr, nullptr);
}

int cfz_colloc_elimination_info(int V, const int32_t *n_sets, const int32_t *has_final, int N_per_set, int n_obs, int n_pairs, const int32_t *pairs,
                                int structured, int32_t *nk, int32_t *kb, int64_t *band_bytes, int64_t *alg_bytes, int64_t *workspace_bytes) {
  if (V < 1 || V > cfzc::kMaxVeh || !n_sets || N_per_set < 1 || n_obs < 0 || n_obs > cfzc::kMaxObs || n_pairs < 0) return fail("bad argument");
  if (structured != 0 && structured != 1) return fail("structured must be 0 (band) or 1 (cfz_jstruct.inl)");
  PairList pr;
  cfzc::CSpec p;
  memset(&p, 0, sizeof p);
  if (parse_pairs(V, n_pairs, pairs, pr) || fill_shape(p, V, n_sets, [&](int a) { return has_final ? has_final[a] != 0 : true; }, N_per_set, n_obs, pr)) return -1;
  p.no_prox = structured_bit(structured, 0, p);
  const int hb = half_bandwidth_of(p);
  if (hb < 0) return -1;
  const cfzc::CDims d = cfzc::cdims(p);
  const bool compact = cfzc::jstruct_mode(p);  // (as solve_colloc: no room for fill where nothing is factored in place)
  const size_t ld = compact ? 2 * (size_t)hb + 1 : 3 * (size_t)hb + 1;
  if (nk) *nk = d.nk;
  if (kb) *kb = hb;
  if (band_bytes) *band_bytes = (int64_t)d.nk * (int64_t)ld * 8;
  // per Newton system: the band elimination clears and assembles the band, then reads and writes it once while it eliminates;
  // the structured elimination: jstruct_alg_doubles
  if (alg_bytes) *alg_bytes = (int64_t)(compact ? cfzc::jstruct_alg_doubles(p, d.nk, ld, d.npp) : 3 * (size_t)d.nk * ld) * 8;
  if (workspace_bytes) *workspace_bytes = (int64_t)cfzc::work_doubles(p, hb) * 8;
  return 0;
}

int cfz_abi_version(void) { return CFZ_ABI_VERSION; }

void cfz_default_colloc_options(cfz_colloc_options *o) {
  memset(o, 0, sizeof *o);
  o->N_per_set = 5; o->max_iter = 3000; o->shrink_tube = 0.5; o->vv_rows = 1; o->structured = 1;
  // mu_init: IPOPT's default; 1e-3 (the MPC step's value) leaves a tail of plans that jam against a bound for 100+ iterations
  o->tol = 1e-2; o->constr_viol_tol = 1e-2; o->mu_init = 0.1; o->curv_kappa = 1e-8;
}

void cfz_default_plan_options(cfz_plan_options *o) {
  memset(o, 0, sizeof *o);
  o->N = 30; o->max_iter = 500; o->bounded_input = 0;
  o->dt = 0.1; o->wb = 2.5; o->shrink_tube = 0.5;
  const double bd[12] = {2.5, 32.5, 7.5, 27.5, -2.5, 2.5, -0.85, 0.85, -1.5, 1.5, -1.0, 1.0};
  memcpy(o->bounds, bd, sizeof bd);
  // mu_init: IPOPT's default, which the reference's state_ws runs with (vehicle.py:206-213 sets tol, constr_viol_tol, max_iter only).
  // Rounds 1-3 had the MPC step's 1e-3 here: over 256 scattered starts the same optima in 15.2 iterations on average and up to 89
  // (the long plan spends 85 iterations at mu = 1e-3 on inertia corrections) against 11.8 and up to 28 with 0.1 -- and a batch lasts as
  // long as its slowest plan.
  o->tol = 1e-2; o->constr_viol_tol = 1e-2; o->mu_init = 0.1; o->curv_kappa = 1e-8;
}

}  // extern "C"
