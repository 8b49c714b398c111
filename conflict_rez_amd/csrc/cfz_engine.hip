// cfz_engine.hip -- libconfrez_hip.so: gfx950 kernels and the C ABI of include/confrez_hip.h.
//
// Kernels
//   solve_kernel   one 128-lane workgroup (two wavefronts; four lanes of a DPP quad per stage) per MPC-step NLP; iterate,
//                  stage data and reduction scratch in LDS (cfz_solver.inl: 40,952 B per instance, four instances per CU);
//                  parameters, warm start and solution are the only algorithmic global-memory traffic
//                  (8*(5 + 3N + 3N n_nbr + 2*7N) B per instance) beside the carry record of the slot (8.8 KB)
//   loop_kernel    the persistent closed loop (cfz_loop_run): the same solver body fed from per-iteration ticket queues of
//                  (scenario, vehicle, iteration) work items, hand-offs between workgroups at agent scope
//   loop_kernel_seq  the same with the sequential exchange of cfz_loop_set_order (one body: cfz_loop_body.inl)
//   loop_kernel_dist, loop_kernel_seq_dist  the same two with the disturbances of cfz_loop_set_disturbance (cfz_disturb.inl)
//   loop_kernel_comm, loop_kernel_seq_comm  the same two with the lossy exchange of cfz_loop_set_comm (cfz_comm.inl) and disturbances
//   loop_kernel_pool, loop_kernel_seq_pool, loop_kernel_pool_comm, loop_kernel_seq_pool_comm  the disturbed and the lossy pairs with the
//                  per-scenario problem constants of cfz_loop_set_problems: an item reads the KArgs block of its scenario's problem
//   solve_kernel_pool  solve_kernel with the same selection, for the stepwise closed loop while a pool is set
//                  The per-scenario obstacle maps of cfz_loop_set_maps run through the same pool kernels: the host composes one KArgs
//                  block per (problem, map) pair in use, whose obs_tab points at that map's table (compose_pool)
//   loop_prep      stepwise closed loop (cfz_loop_step): parameters and shifted warm start of every vehicle from the
//                  previous predictions (reference vehicle_follower.py:432-476, 636-637), the measurement under a disturbance
//   loop_post      stepwise closed loop: read-back or shift fallback, plant integration, clock
//                  (reference :484-563), and the record of the realised trajectory when one is kept (:556-563)
//   vs_prep        loop_prep for the vehicle-sharded loop (cfz_vsl_step, which ends with loop_post): table, clock and neighbours
//                  from the caller; the two share the __device__ function prep_stage
//   audit_kernel   signed distances, first contact and arrivals along a recorded trajectory (cfz_audit.inl), one
//                  wavefront per scenario, each against the obstacles of its own map
//   score_kernel   what every vehicle's recorded closed loop cost against its plan (cfz_score.inl: the reference's objective
//                  :263-272 along the trajectory driven, waiting, reversals, fallback runs :501-524), one wavefront per scenario
//   conflict_kernel  the conflict map of a plan pool (cfz_conflict.inl): body clearance of every pair of plans against their relative
//                  delay, one workgroup per (set, pair), the pair's columns (conflict_columns) staged in LDS
//   delay_kernel   the start delays that make a plan set conflict-free, searched over that map (cfz_delay.inl): one workgroup per set,
//                  the windowed free mask as bits in LDS, span levels in ascending order
//   coord_kernel   the coordination diagrams of a plan pool (cfz_coord.inl): which sample of one plan is too close to which sample of
//                  another, as rows of bits, one workgroup per (set, pair, block of rows), a wavefront per row, a ballot per 64 columns
//   schedule_kernel  hold-point schedules that make a plan set conflict-free (cfz_schedule.inl): one workgroup per set, a wavefront per
//                  priority order, the reachable samples of a vehicle as one row of bits over the lanes
// The planning kernels (state_ws, collocation plans) and their entry points live in cfz_planning.hip, a translation unit
// of its own (two units compile in parallel; both at -O3 since round 3, see __graft_entry__.build).
// Host side: a handle owns all device buffers (DevBuf, cfz_devmem.h), one stream and its events; the closed loop's are cfz_handle::Loop,
// released by assigning a fresh one.  cfz_loop_step is loop_round (prep, solve, post) once for Jacobi or V times for the sequential exchange;
// cfz_loop_run picks its kernel from kLoopVariants, the one list of the persistent kernels (loop_variant maps the setting in force
// to its row).  A setting is stated once on the host side: its fields in cfz_handle::Loop, its device block through upload_setting,
// its kernel arguments through disturb_args / comm_args, its kernels as rows of kLoopVariants and lines of cfz_loop_run's chain.
// Entry points of the closed loop open with loop_ready.

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <unistd.h>
#include <cmath>
#include <map>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/confrez_hip.h"
#include "cfz_solver.inl"
#include "cfz_audit.inl"
#include "cfz_score.inl"
#include "cfz_conflict.inl"
#include "cfz_delay.inl"
#include "cfz_schedule.inl"
#include "cfz_wave.inl"
#include "cfz_disturb.inl"
#include "cfz_comm.inl"
#include "cfz_common.h"

thread_local std::string cfz_g_err;  // cfz_last_error(); shared with cfz_planning.hip (cfz_common.h)

namespace {

// Plant (vehicle_follower.py:528-543, CasADi integrator "idas"): RK4 with this many sub-steps per dt.  10 sub-steps are
// within 6e-11 of the converged solution over the whole input range, tighter than IDAS's default tolerances.
constexpr int kPlantSubsteps = 10;

struct DualPtrs { double *l, *m, *lam_ij, *lam_ji, *s; };
// spec, derived constants and workspace layout in device memory: the solver kernels read the fields where they use them
// (scalar loads, scalar cache) instead of holding all ~200 of them in scalar registers from the kernel's first instruction
struct KArgs { cfz::KSpec sp; cfz::KDer dv; cfz::Lay L; };

constexpr int kWavesPerSimd = 2;  // the second argument of every solver kernel's launch bound
// Two kernels, one body (cfz_solve_body.inl, included into both, as the persistent kernels share cfz_loop_body.inl).
__global__ __launch_bounds__(cfz::kNL, kWavesPerSimd) void solve_kernel(const KArgs *__restrict__ ka, int B, const double *x0,
                                                   const double *ref, const double *nbr, double *zu, int32_t *status,
                                                   int32_t *iters, double *stats, DualPtrs du, const int32_t *order,
                                                   double *wst, int wst_stride, const int32_t *carry, int carry_all,
                                                   const int32_t *slots) {
  constexpr bool kPool = false;
  const KArgs *const pool = nullptr; const int32_t *const problem_of = nullptr; constexpr int V = 1;
#include "cfz_solve_body.inl"
}

// solve_kernel for the stepwise closed loop under cfz_loop_set_problems: instance b = (scenario s, vehicle) of V solves the problem
// pool[problem_of[s]] (its spec and derived constants; the layout is the handle's, ka->L).  The index depends on the workgroup alone,
// so the block is read through scalar loads as ka is.  A kernel of its own: solve_kernel keeps its code.
__global__ __launch_bounds__(cfz::kNL, kWavesPerSimd) void solve_kernel_pool(const KArgs *__restrict__ ka, int B, const double *x0,
                                                   const double *ref, const double *nbr, double *zu, int32_t *status,
                                                   int32_t *iters, double *stats, DualPtrs du, const int32_t *order,
                                                   double *wst, int wst_stride, const int32_t *carry, int carry_all,
                                                   const int32_t *slots, const KArgs *__restrict__ pool,
                                                   const int32_t *__restrict__ problem_of, int V) {
  constexpr bool kPool = true;
#include "cfz_solve_body.inl"
}

// ---- closed loop ------------------------------------------------------------------------------
// pred[S][V][7][N] last predictions, state[S][V][5], kidx[S] reference sample index.  ref_table[P][V][T][7] is a pool of plan
// sets; scenario s follows set table_of[s].
// The rule of one step is stated once: cfz_loop_step (loop_prep) and cfz_vsl_step (vs_prep) differ in where the table, the clock and
// the neighbours' predictions come from and share prep_stage; both end with loop_post.

// stage k of instance b's parameters and warm start (vehicle_follower.py:432-476): the reference window from the vehicle's
// plan[T][7] at clock k0, clamped at the last sample; its own prediction own[7][N] and the neighbours' advanced one step
// (_adv_onestep, :413-426).  others[V][rows][N] holds x, y, psi of the scenario's V vehicles in the first three of `rows` rows; v is
// the instance's vehicle.  rank[V] (NULL: none) with r: the vehicles ranked before r are read as they stand.
// cm (cfz_loop_set_comm; cm.p_drop NULL: none, every neighbour's newest prediction from `others`): the lossy exchange of
// cfz_comm.inl in iteration t of scenario s.  Neighbour u is read from the message the age rule gives, in its slot of the ring
// (rows of 7), at the row comm_row gives; with no loss that is the slot and the row read without it.
__device__ inline void prep_stage(int b, int k, int N, int T, int V, int v, const double *plan, int k0, const double *own,
                                  const double *others, int rows, const int32_t *rank, int r, const cfz::CommArgs &cm, int s, int t,
                                  double *ref, double *nbr, double *zu) {
  const int ka = (k + 1 < N) ? k + 1 : N - 1;
  int kr = k0 + k; if (kr > T - 1) kr = T - 1;
  for (int c = 0; c < 3; ++c) ref[((size_t)b * 3 + c) * N + k] = plan[(size_t)kr * 7 + c];
  for (int c = 0; c < 7; ++c) zu[((size_t)b * 7 + c) * N + k] = own[c * N + ka];
  int o = 0;
  for (int u = 0; u < V; ++u) {
    if (u == v) continue;
    const bool earlier = rank && rank[u] < r;
    const double *src = others + (size_t)u * rows * N;
    int a = 0;
    if (cm.p_drop) {
      const int want = cfz::comm_want(t, earlier);
      a = cfz::comm_age(cm, s, v, u, want);
      src = cm.ring + (size_t)cfz::comm_slot(want - a, cm.max_age) * cm.slot_stride + ((size_t)s * V + u) * 7 * N;
    }
    const int ku = cfz::comm_row(k, earlier ? 0 : 1, cm.compensate, a, N);
    for (int c = 0; c < 3; ++c) nbr[(((size_t)b * (V - 1) + o) * 3 + c) * N + k] = src[(size_t)c * N + ku];
    ++o;
  }
}

// xperm / xrank [S][V] (cfz_loop_set_order): the exchange order of every scenario and its inverse.  NULL: Jacobi, one thread per
// (instance, stage) of all B instances.  Otherwise round r of a sequential step: one thread per (scenario, stage), for the vehicle
// v = xperm[s][r]; the neighbours ranked before it have already posted this step's prediction to `pred`, which starts at this
// step's time and is read as it stands; the others' (and v's own warm start) are the previous step's, advanced.
// dz (cfz_loop_set_disturbance; dz.sigma NULL: none): the solver's x0 is the measurement, state + d[0:5] of this `step`.
// cm (cfz_loop_set_comm; cm.p_drop NULL: none): the neighbours come from the ring of messages by the age rule (prep_stage).
__global__ void loop_prep(int S, int V, int N, int T, const double *ref_table, const int32_t *table_of, const int32_t *kidx,
                          const double *pred, const double *state, double *x0, double *ref, double *nbr,
                          double *zu, int r, const int32_t *xperm, const int32_t *xrank, cfz::DisturbArgs dz, int step, cfz::CommArgs cm) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (long)(xperm ? S : S * V) * N) return;
  const int k = (int)(tid % N);
  int b = (int)(tid / N);
  if (xperm) b = b * V + xperm[b * V + r];
  const int s = b / V, v = b - s * V;
  if (k < 5) x0[b * 5 + k] = dz.sigma ? cfz::disturb_add(state[b * 5 + k], cfz::disturb_value(dz, s, v, step, k)) : state[b * 5 + k];
  prep_stage(b, k, N, T, V, v, ref_table + ((size_t)table_of[s] * V + v) * T * 7, kidx[s], pred + (size_t)b * 7 * N,
             pred + (size_t)s * V * 7 * N, 7, xrank ? xrank + (size_t)s * V : nullptr, r, cm, s, step, ref, nbr, zu);
}

__global__ void advance_clock(int S, int K, int32_t *kidx) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < S) kidx[s] += K;
}

// One thread per instance: accept the solution or shift the old prediction, integrate the plant.  rec (NULL: no record) is
// this step's slice [S][V][7] of the record: state after the plant and the applied (a, w); rec_si its [2][S][V] status, iters.
// xperm NULL: all B instances.  Otherwise round r of a sequential step (loop_prep): one thread per scenario, for its vehicle of
// rank r; the clock kidx (NULL: the caller keeps it) advances with the last round, after every vehicle has read its reference.
// dz (dz.sigma NULL: none): the applied input is the prediction's first plus d[5:7], clipped to the input box [a_lo, a_hi] x
// [w_lo, w_hi]; the plant starts from the true state and d[7:12] is added to what it returns; the record keeps both.
// carry (NULL: none; cfz_vsl_step): the carry flag of the next iteration, a vehicle whose solve converged starts its next one from
// these multipliers.
// msg (NULL: none; cfz_loop_set_comm): this iteration's slot [S][V][7][N] of the ring of messages, which takes the posted prediction too.
// ka: the handle's block, which gives dt, wb and the input box (bounds[8:12]); pool, problem_of (NULL: none; cfz_loop_set_problems):
// the block of the scenario's problem instead (dt and wb are the handle's in every problem, cfz_problem_check).
__global__ void loop_post(int S, int V, int N, const KArgs *ka, const int32_t *status, const int32_t *iters, const double *zu,
                          double *pred, double *state, int32_t *kidx, double *rec, int32_t *rec_si, int r, const int32_t *xperm,
                          cfz::DisturbArgs dz, int step, int32_t *carry, double *msg, const KArgs *pool, const int32_t *problem_of) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= (xperm ? S : S * V)) return;
  if (xperm) b = b * V + xperm[b * V + r];
  double *pb = pred + (size_t)b * 7 * N;
  if (status[b] == 0) {
    for (int i = 0; i < 7 * N; ++i) pb[i] = zu[(size_t)b * 7 * N + i];
  } else {
    for (int c = 0; c < 7; ++c)
      for (int k = 0; k + 1 < N; ++k) pb[c * N + k] = pb[c * N + k + 1];
  }
  if (msg)
    for (int i = 0; i < 7 * N; ++i) msg[(size_t)b * 7 * N + i] = pb[i];
  double z[5], out[5];
  for (int i = 0; i < 5; ++i) z[i] = state[b * 5 + i];
  double a0 = pb[5 * N], w0 = pb[6 * N];
  const int s = b / V, v = b - s * V;
  const cfz::KSpec &sp = (pool ? pool + problem_of[s] : ka)->sp;
  if (dz.sigma) {
    a0 = cfz::disturb_clip(cfz::disturb_add(a0, cfz::disturb_value(dz, s, v, step, 5)), sp.bounds[8], sp.bounds[9]);
    w0 = cfz::disturb_clip(cfz::disturb_add(w0, cfz::disturb_value(dz, s, v, step, 6)), sp.bounds[10], sp.bounds[11]);
  }
  cfz::rk4_step<false>(z, a0, w0, sp.dt, sp.wb, kPlantSubsteps, out, nullptr);
  if (dz.sigma)
    for (int i = 0; i < 5; ++i) out[i] = cfz::disturb_add(out[i], cfz::disturb_value(dz, s, v, step, 7 + i));
  for (int i = 0; i < 5; ++i) state[b * 5 + i] = out[i];
  if (kidx && (xperm ? r == V - 1 : b % V == 0)) kidx[b / V] += 1;
  if (carry) carry[b] = status[b] == 0;
  if (rec) {
    double *r = rec + (size_t)b * 7;
    for (int i = 0; i < 5; ++i) r[i] = out[i];
    r[5] = a0; r[6] = w0;
    rec_si[b] = status[b]; rec_si[S * V + b] = iters[b];
  }
}

// ---- vehicle-sharded closed loop (partitioning B: a rank owns n_own vehicles of S scenarios) ------------------------
// The glue of one MPC iteration around the solve, on the caller's stream: instances are ordered [s][o] (o = index into the
// owned vehicles).  allpred[S][V][3][N] holds x, y, psi of EVERY vehicle's last prediction (gathered over RCCL by the
// caller), pred[S][n_own][7][N] this rank's own predictions, table[n_own][T][7] the owned vehicles' plans.
// vs_prep: parameters and shifted warm start (prep_stage), one thread per (instance, stage); the step ends with loop_post, which
// writes the carry flag.
__global__ void vs_prep(int S, int V, int n_own, int N, int T, const int32_t *own, const double *table, const int32_t *k0, int t,
                        const double *allpred, const double *pred, const double *state, double *x0, double *ref, double *nbr,
                        double *zu) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (long)S * n_own * N) return;
  const int k = (int)(tid % N);
  const int b = (int)(tid / N);
  const int s = b / n_own, o = b - s * n_own;
  if (k < 5) x0[b * 5 + k] = state[b * 5 + k];
  prep_stage(b, k, N, T, V, own[o], table + (size_t)o * T * 7, k0[s] + t, pred + (size_t)b * 7 * N, allpred + (size_t)s * V * 3 * N, 3,
             nullptr, 0, cfz::comm_none(), s, t, ref, nbr, zu);
}

// Longest-processing-time-first dispatch order for the next step: instances sorted by the iteration count of
// the step just finished, descending (counting sort, one workgroup).  The solve of an instance does not depend
// on where it runs, only the makespan of the launch does.
__global__ __launch_bounds__(1024) void order_by_iters(int B, const int32_t *iters, int32_t *order) {
  __shared__ int hist[1024];
  const int t = threadIdx.x;
  hist[t] = 0;
  __syncthreads();
  for (int b = t; b < B; b += 1024) atomicAdd(&hist[1023 - min(iters[b], 1023)], 1);
  __syncthreads();
  if (t == 0) { int acc = 0; for (int i = 0; i < 1024; ++i) { const int c = hist[i]; hist[i] = acc; acc += c; } }
  __syncthreads();
  for (int b = t; b < B; b += 1024) order[atomicAdd(&hist[1023 - min(iters[b], 1023)], 1)] = b;
}

// ---- persistent closed loop -----------------------------------------------------------------------
// K MPC iterations of every scenario in ONE launch.  The Jacobi exchange only couples the V vehicles of a
// scenario, so there is no reason to stop the whole GPU after every iteration: work items (scenario, vehicle,
// iteration t) sit in a queue; a wavefront pops one, builds its parameters from the scenario's predictions of
// iteration t-1, solves, writes prediction t and the new plant state, and the last of the V vehicles to finish
// iteration t publishes the V items of t+1.  Hard instances then delay only their own scenario.
//   qbuf          [head K][tail K][slots K x B]: one ticket queue per iteration t.  tail[t] = slots reserved by
//                 publishers, head[t] = tickets handed out, slot = instance id b or -1 while not yet written.
//                 Poppers serve the LOWEST iteration that has unclaimed slots first, so a scenario that is behind
//                 never waits behind scenarios that are ahead (critical path first).  A ticket can be taken a
//                 moment before its slot is written (or, in a race for the last slots, before it is reserved):
//                 the holder polls the slot; every iteration has exactly B slots, so tickets >= B are void.
//   ctrl[0] lowest iteration whose tickets are not exhausted (monotone hint; K = all work handed out)
//   ctrl[1] items completed   ctrl[2] error flag
//   done[S]       finished vehicles of the scenario (monotone: iteration t is complete at (t+1)*V)
//   pred[2][B][7][N] double-buffered by iteration parity (read t%2, write (t+1)%2)
// Hand-offs between workgroups follow the agent-scope publish/acquire recipe in its write-through form: the payload (prediction row,
// state, carry record) is stored write-through at agent scope (cfz::store_shared), every storing wavefront waits for its stores, the
// workgroup meets, one lane signals by device-scope atomics; consumer: atomic load of the slot, agent-scope acquire fence, plain
// payload loads.  No item writes the XCD's L2 back: the spill frames of the workgroups resident there stay in it.
// The pop has no lane-divergent control flow (all lanes issue the same loads; atomics add 1 from lane 0 and 0 from
// the others): a value defined under `if (lane == 0)` and broadcast afterwards was miscompiled by hipcc 7.2.
// CFZ_LOOP_TRACE (diagnostic builds, tools/build_variant.sh): CFZ_MARK leaves every workgroup's last phase for the watchdog;
// CFZ_ITEM_STAMP writes item (t, b)'s record of kLoopTraceWords 64-bit words: the constant 100 MHz clock after the pop [0], at the start [1]
// and the end [2] of the solve and after the hand-off [3], and 1 + whether the item ran prioritised [4] (0: the item never ran).
// tools/loop_priority_trace.py reads them through cfz_loop_trace_read.  Neither exists in the product build.
#ifdef CFZ_LOOP_TRACE
constexpr int kLoopTraceWords = 5;
__device__ long long *cfz_loop_trace_buf;
#define CFZ_MARK(c) do { if (threadIdx.x == 0) __hip_atomic_store(&ctrl[4 + blockIdx.x], (c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while (0)
#define CFZ_ITEM_STAMP(w, flag) do { if (threadIdx.x == 0) { long long *cfz_r = cfz_loop_trace_buf + ((size_t)t * B + b) * kLoopTraceWords;      \
                                                        cfz_r[w] = (long long)wall_clock64(); if ((w) == 0) cfz_r[4] = 1 + (flag); } } while (0)
#else
#define CFZ_MARK(c) do { } while (0)
#define CFZ_ITEM_STAMP(w, flag) do { } while (0)
#endif
//   ref_table[P][V][T][7], table_of[S]: the pool of plan sets and the one each scenario follows (as loop_prep)
//   rec[K][S][V][7], rec_si[K][2][S][V]: the record of this launch's iterations (NULL: none; as loop_post)
// kSeq (loop_kernel_seq): the sequential exchange of cfz_loop_set_order.  xperm / xrank [S][V] are the order of every scenario and
// its inverse (written by the host before the launch: plain loads, no acquire).  The V solves of a scenario's iteration t run one
// after another: the item of rank r publishes the item of rank r + 1 into the same queue t, the last rank publishes rank 0 of
// t + 1.  Every iteration still receives exactly B slots, so the ticket rules above hold unchanged.  A vehicle reads the neighbours
// ranked before it from the output parity at stage k (iteration t's predictions start at time t), the others from the input
// parity, advanced.  The new edge, rank r to rank r + 1, has the same publish / acquire pair as the edge from t to t + 1, and the
// chain of such pairs covers the ranks below r - 1 as well (their payload reached memory before their own signal).
// It cannot deadlock: a scenario has exactly one item in flight, every completion publishes exactly one item, and the workgroup
// that completed is then free to take it; the grid (at most S workgroups) never exceeds the items in flight.
// Two kernels, one body (cfz_loop_body.inl, included into both): loop_kernel keeps its symbol (profiles and bench.py name rows
// by it), takes no argument for the exchange rule and compiles to the Jacobi loop's code alone (a __device__ template with the
// `__restrict__` parameter moved the kernel's register allocation: 16 more VGPR spills).
// the arguments every persistent kernel takes, before those of its own setting
#define CFZ_LOOP_ARGS const KArgs *__restrict__ ka, int S, int V, int K, int T, const double *ref_table, const int32_t *table_of,        \
                      const int32_t *kidx0, int t_base, double *pred, double *state, double *scratch, int32_t *qbuf, int32_t *ctrl,       \
                      int32_t *done, int32_t *status, int32_t *iters, double *stats, int32_t *iter_sum, double *wst, int wst_stride,     \
                      int prio_lag, int prio_tail, double *rec, int32_t *rec_si
__global__ __launch_bounds__(cfz::kNL, kWavesPerSimd) void loop_kernel(CFZ_LOOP_ARGS) {
  constexpr bool kSeq = false, kDist = false, kComm = false, kPool = false;
  const KArgs *const pool = nullptr; const int32_t *const problem_of = nullptr; constexpr bool dz_clip = true;
  const cfz::CommArgs cm = cfz::comm_none();
  const int32_t *const xperm = nullptr, *const xrank = nullptr;
  const cfz::DisturbArgs dz = cfz::disturb_none();
  const int step0 = 0;
#include "cfz_loop_body.inl"
}

__global__ __launch_bounds__(cfz::kNL, kWavesPerSimd) void loop_kernel_seq(CFZ_LOOP_ARGS, const int32_t *xperm, const int32_t *xrank) {
  constexpr bool kSeq = true, kDist = false, kComm = false, kPool = false;
  const KArgs *const pool = nullptr; const int32_t *const problem_of = nullptr; constexpr bool dz_clip = true;
  const cfz::CommArgs cm = cfz::comm_none();
  const cfz::DisturbArgs dz = cfz::disturb_none();
  const int step0 = 0;
#include "cfz_loop_body.inl"
}

// The two kernels above with the disturbances of cfz_loop_set_disturbance (kDist): dz is the setting, step0 the MPC iterations done
// since cfz_loop_init* (iteration t of this launch is step step0 + t of the streams).  Kernels of their own, made as loop_kernel_seq
// was, so that the two undisturbed kernels keep the code they had before disturbances existed.
__global__ __launch_bounds__(cfz::kNL, kWavesPerSimd) void loop_kernel_dist(CFZ_LOOP_ARGS, cfz::DisturbArgs dz, int step0) {
  constexpr bool kSeq = false, kDist = true, kComm = false, kPool = false;
  const KArgs *const pool = nullptr; const int32_t *const problem_of = nullptr; constexpr bool dz_clip = true;
  const cfz::CommArgs cm = cfz::comm_none();
  const int32_t *const xperm = nullptr, *const xrank = nullptr;
#include "cfz_loop_body.inl"
}

__global__ __launch_bounds__(cfz::kNL, kWavesPerSimd) void loop_kernel_seq_dist(CFZ_LOOP_ARGS, const int32_t *xperm,
                                                                 const int32_t *xrank, cfz::DisturbArgs dz, int step0) {
  constexpr bool kSeq = true, kDist = true, kComm = false, kPool = false;
  const KArgs *const pool = nullptr; const int32_t *const problem_of = nullptr; constexpr bool dz_clip = true;
  const cfz::CommArgs cm = cfz::comm_none();
#include "cfz_loop_body.inl"
}

// The lossy exchange of cfz_loop_set_comm (kComm; cfz_comm.inl): cm is the setting, its ring of messages stands in for the parity
// pair `pred` (unused here), indexed by the absolute iteration step0 + t.  Compiled with kDist, so that noise and loss combine
// without further variants; with no noise set, dz is an all-zero sigma, which is bit-neutral.  Kernels of their own again: the
// four above keep their code.  The release / acquire edges are those of the kernels above: the older slots a reader may take were
// published by earlier iterations of the same scenario, which the chain of edges to this item covers.
__global__ __launch_bounds__(cfz::kNL, kWavesPerSimd) void loop_kernel_comm(CFZ_LOOP_ARGS, cfz::DisturbArgs dz, int step0,
                                                             cfz::CommArgs cm) {
  constexpr bool kSeq = false, kDist = true, kComm = true, kPool = false;
  const KArgs *const pool = nullptr; const int32_t *const problem_of = nullptr; constexpr bool dz_clip = true;
  const int32_t *const xperm = nullptr, *const xrank = nullptr;
#include "cfz_loop_body.inl"
}

__global__ __launch_bounds__(cfz::kNL, kWavesPerSimd) void loop_kernel_seq_comm(CFZ_LOOP_ARGS, const int32_t *xperm,
                                                                 const int32_t *xrank, cfz::DisturbArgs dz, int step0, cfz::CommArgs cm) {
  constexpr bool kSeq = true, kDist = true, kComm = true, kPool = false;
  const KArgs *const pool = nullptr; const int32_t *const problem_of = nullptr; constexpr bool dz_clip = true;
#include "cfz_loop_body.inl"
}

// The problem pool of cfz_loop_set_problems (kPool): pool[P] holds one KArgs block per problem, problem_of[S] the problem of every
// scenario; an item binds the spec and the derived constants of its scenario's problem and keeps the handle's layout.  Compiled as the
// comm kernels were, with kDist, so that the pool combines with noise and loss without a full cross product: with no noise set, dz is
// an all-zero sigma, which is bit-neutral once the clip of the applied input is left out as well (dz_clip 0: the undisturbed loop clips
// nothing, and a prediction seeded from the plan may lie outside a problem's tighter input box).  Kernels of their own once more: the
// six above keep their code.
__global__ __launch_bounds__(cfz::kNL, kWavesPerSimd) void loop_kernel_pool(CFZ_LOOP_ARGS, cfz::DisturbArgs dz, int step0,
                                                             const KArgs *__restrict__ pool, const int32_t *__restrict__ problem_of, int dz_clip) {
  constexpr bool kSeq = false, kDist = true, kComm = false, kPool = true;
  const cfz::CommArgs cm = cfz::comm_none();
  const int32_t *const xperm = nullptr, *const xrank = nullptr;
#include "cfz_loop_body.inl"
}

__global__ __launch_bounds__(cfz::kNL, kWavesPerSimd) void loop_kernel_seq_pool(CFZ_LOOP_ARGS, const int32_t *xperm, const int32_t *xrank,
                                                                 cfz::DisturbArgs dz, int step0, const KArgs *__restrict__ pool,
                                                                 const int32_t *__restrict__ problem_of, int dz_clip) {
  constexpr bool kSeq = true, kDist = true, kComm = false, kPool = true;
  const cfz::CommArgs cm = cfz::comm_none();
#include "cfz_loop_body.inl"
}

__global__ __launch_bounds__(cfz::kNL, kWavesPerSimd) void loop_kernel_pool_comm(CFZ_LOOP_ARGS, cfz::DisturbArgs dz, int step0, cfz::CommArgs cm,
                                                                  const KArgs *__restrict__ pool, const int32_t *__restrict__ problem_of, int dz_clip) {
  constexpr bool kSeq = false, kDist = true, kComm = true, kPool = true;
  const int32_t *const xperm = nullptr, *const xrank = nullptr;
#include "cfz_loop_body.inl"
}

__global__ __launch_bounds__(cfz::kNL, kWavesPerSimd) void loop_kernel_seq_pool_comm(CFZ_LOOP_ARGS, const int32_t *xperm, const int32_t *xrank,
                                                                      cfz::DisturbArgs dz, int step0, cfz::CommArgs cm,
                                                                      const KArgs *__restrict__ pool, const int32_t *__restrict__ problem_of, int dz_clip) {
  constexpr bool kSeq = true, kDist = true, kComm = true, kPool = true;
#include "cfz_loop_body.inl"
}
#undef CFZ_LOOP_ARGS

// The ten persistent kernels, stated once: what each was compiled with (dist: kDist, and so on).  create_fill, the occupancy query and
// the launch of cfz_loop_run all go through this table; a new kernel is one more row here and one more line in cfz_loop_run's chain.
// The built-in priority setting of cfz_loop_run, chosen by measurement (docs/notebook.md "Issue priority on the critical path"): the items
// of the oldest open iteration, and no rank condition (a divisor d > 0 would add one: the last B / d positions of an iteration's queue)
constexpr int kLoopPrioLag = 0, kLoopPrioTailDiv = 0;
#ifdef CFZ_LOOP_TRACE
long long *g_loop_trace_dev = nullptr; size_t g_loop_trace_items = 0; int g_loop_trace_grid = 0;
#endif
struct LoopVariant { const void *fn; bool seq, dist, comm, pool; };
const LoopVariant kLoopVariants[10] = {
    {(const void *)loop_kernel, false, false, false, false},          {(const void *)loop_kernel_seq, true, false, false, false},
    {(const void *)loop_kernel_dist, false, true, false, false},      {(const void *)loop_kernel_seq_dist, true, true, false, false},
    {(const void *)loop_kernel_comm, false, true, true, false},       {(const void *)loop_kernel_seq_comm, true, true, true, false},
    {(const void *)loop_kernel_pool, false, true, false, true},       {(const void *)loop_kernel_seq_pool, true, true, false, true},
    {(const void *)loop_kernel_pool_comm, false, true, true, true},   {(const void *)loop_kernel_seq_pool_comm, true, true, true, true}};

// The row that runs the setting in force.  The comm and the pool kernels exist only with kDist (no full cross product): while no
// disturbance is set they take the zero-noise block (disturb_args), so every one of the 32 settings has exactly one row.  A map pool
// (mp_on) runs on the pool rows, as a problem pool does: the two are composed into one set of blocks on the host (compose_pool).
int loop_variant(bool seq, bool dz_on, bool cm_on, bool pb_on, bool mp_on) {
  const bool pool = pb_on || mp_on, dist = dz_on || cm_on || pool;
  for (int i = 0; i < 10; ++i) {
    const LoopVariant &v = kLoopVariants[i];
    if (v.seq == seq && v.dist == dist && v.comm == cm_on && v.pool == pool) return i;
  }
  return -1;  // (not reached: the ten rows cover the 32 settings)
}

// delivered[K][S][V][V]: the delivery bits of messages [tau0, tau0 + K) (cfz_loop_comm), receiver before sender, diagonal 1; one thread
// each, through the function the loop uses
__global__ void comm_fill(cfz::CommArgs cm, int S, int V, int tau0, long n, int32_t *delivered) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int u = (int)(i % V), v = (int)((i / V) % V), s = (int)((i / ((long)V * V)) % S), k = (int)(i / ((long)V * V * S));
  delivered[i] = u == v ? 1 : (cfz::comm_delivered(cm.seed, cm.stream[s], v, u, tau0 + k, cm.p_drop[s]) ? 1 : 0);
}

// d[K][S][V][12]: the disturbances of steps [t0, t0 + K) (cfz_loop_disturbance), one thread each, through the function the loop uses
__global__ void disturb_fill(cfz::DisturbArgs dz, int S, int V, int t0, long n, double *d) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % cfz::kDisturbN);
  const long b = i / cfz::kDisturbN;
  const int v = (int)(b % V), s = (int)((b / V) % S), k = (int)(b / ((long)V * S));
  d[i] = cfz::disturb_value(dz, s, v, t0 + k, c);
}

// ---- dual warm starts: exact separation of two convex quadrilaterals and the duals that certify it ------------------
// The reference maximises d over the OBCA duals (vehicle.py:233-296, multi_vehicle_planner.py:208-341); the optimum is
// the Euclidean distance of the two polygons and the optimal duals encode the unit direction n* between their closest
// points: lam >= 0 with A'lam = n* (two faces of the polygon through its support vertex), mu >= 0 with G'mu = -R'n*
// (the body rectangle's normals are +-e_x, +-e_y, so mu is the positive/negative part).  Closest points of two disjoint
// convex polygons: a vertex of one and a point of an edge of the other (possibly its end point, the vertex-vertex case),
// so 2 x 4 x 4 point-segment distances decide.  If the polygons touch or overlap, the best face normal stands in (its
// value is then <= 0; the reference's optimum with |A'lam| <= 1 would be 0 at lam = mu = 0).
__device__ inline void point_segment(double qx, double qy, double ax, double ay, double bx, double by, double &dist2, double &nx, double &ny) {
  const double ex = bx - ax, ey = by - ay, wx = qx - ax, wy = qy - ay;
  double t = (wx * ex + wy * ey) / (ex * ex + ey * ey);
  t = fmin(fmax(t, 0.0), 1.0);
  nx = wx - t * ex; ny = wy - t * ey;  // from the segment's closest point to q
  dist2 = nx * nx + ny * ny;
}

// unit direction n from polygon P (vertices PV, counter-clockwise) towards polygon Q and their distance; false if they
// are not strictly apart
__device__ inline bool polygon_gap(const double PV[4][2], const double QV[4][2], double &nx, double &ny, double &dist) {
  double best = INFINITY, bx = 0.0, by = 0.0;
  for (int v = 0; v < 4; ++v)
    for (int e = 0; e < 4; ++e) {
      double d2, ux, uy;
      point_segment(QV[v][0], QV[v][1], PV[e][0], PV[e][1], PV[(e + 1) & 3][0], PV[(e + 1) & 3][1], d2, ux, uy);  // P's edge -> Q's vertex
      if (d2 < best) { best = d2; bx = ux; by = uy; }
      point_segment(PV[v][0], PV[v][1], QV[e][0], QV[e][1], QV[(e + 1) & 3][0], QV[(e + 1) & 3][1], d2, ux, uy);  // Q's edge -> P's vertex
      if (d2 < best) { best = d2; bx = -ux; by = -uy; }
    }
  dist = sqrt(best);
  if (!(dist > 1e-12)) return false;
  nx = bx / dist; ny = by / dist;
  return true;
}

// lam >= 0 on the faces of {A p <= b} (vertices V) with A'lam = n: the two faces through the support vertex in direction n
__device__ inline void cone_duals(const double A[4][2], const double b[4], const double V[4][2], double nx, double ny, double lam[4]) {
  int v = 0; double sup = -INFINITY;
  for (int i = 0; i < 4; ++i) { const double h = nx * V[i][0] + ny * V[i][1]; if (h > sup) { sup = h; v = i; } }
  int i0 = 0, i1 = 1; double r0 = INFINITY, r1 = INFINITY;
  for (int i = 0; i < 4; ++i) {
    const double r = fabs(A[i][0] * V[v][0] + A[i][1] * V[v][1] - b[i]);
    if (r < r0) { r1 = r0; i1 = i0; r0 = r; i0 = i; } else if (r < r1) { r1 = r; i1 = i; }
  }
  const int ia = i0 < i1 ? i0 : i1, ib = i0 < i1 ? i1 : i0;
  const double det = A[ia][0] * A[ib][1] - A[ib][0] * A[ia][1];
  for (int i = 0; i < 4; ++i) lam[i] = 0.0;
  lam[ia] = fmax((A[ib][1] * nx - A[ib][0] * ny) / det, 0.0);
  lam[ib] = fmax((-A[ia][1] * nx + A[ia][0] * ny) / det, 0.0);
}

// dual_ws (reference vehicle.py:233-296): for fixed poses, the optimal dual certificate of every (pose, obstacle) pair and
// the separation it certifies.  One thread per pair.
__global__ void dual_ws_kernel(const cfz::KSpec sp, int n, const double *poses, double *l, double *mu_out, double *d) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int no = sp.n_obs;
  if (tid >= n * no) return;
  const int k = tid / no, j = tid - k * no;
  double A[4][2], b[4], V[4][2];
  for (int i = 0; i < 4; ++i) {
    A[i][0] = sp.A_obs[j][i][0]; A[i][1] = sp.A_obs[j][i][1]; b[i] = sp.b_obs[j][i];
    V[i][0] = sp.V_obs[j][i][0]; V[i][1] = sp.V_obs[j][i][1];
  }
  const double x = poses[k * 3], y = poses[k * 3 + 1], psi = poses[k * 3 + 2];
  double s, c;
  sincos(psi, &s, &c);
  const double g0 = sp.g[0], g1 = sp.g[1], g2 = sp.g[2], g3 = sp.g[3];
  const double BV[4][2] = {{g0, g1}, {-g2, g1}, {-g2, -g3}, {g0, -g3}};
  double W[4][2];  // body vertices in the world frame, counter-clockwise
  for (int i = 0; i < 4; ++i) { W[i][0] = x + c * BV[i][0] - s * BV[i][1]; W[i][1] = y + s * BV[i][0] + c * BV[i][1]; }
  double lam[4] = {0, 0, 0, 0}, muv[4] = {0, 0, 0, 0}, nx, ny, dist;
  if (polygon_gap(V, W, nx, ny, dist)) {  // n: from the obstacle towards the vehicle
    cone_duals(A, b, V, nx, ny, lam);
    const double mx = -(c * nx + s * ny), my = -(-s * nx + c * ny);  // G'mu = -R'n
    muv[0] = fmax(mx, 0.0); muv[1] = fmax(my, 0.0); muv[2] = fmax(-mx, 0.0); muv[3] = fmax(-my, 0.0);
  } else {  // touching or overlapping: the best face normal
    double sep2[2];
    const int sel = cfz::select_rows_sep(A, b, V, x, y, c, s, sp.g, 0, sep2);
    const int kind = sel >> 6, f = (sel >> 4) & 3;
    if (kind == 1) { nx = A[f][0]; ny = A[f][1]; }
    else { const double gx = (f == 0) - (f == 2), gy = (f == 1) - (f == 3); nx = -(c * gx - s * gy); ny = -(s * gx + c * gy); }
    cone_duals(A, b, V, nx, ny, lam);
    const double mx = -(c * nx + s * ny), my = -(-s * nx + c * ny);
    muv[0] = fmax(mx, 0.0); muv[1] = fmax(my, 0.0); muv[2] = fmax(-mx, 0.0); muv[3] = fmax(-my, 0.0);
  }
  for (int i = 0; i < 4; ++i) { l[(size_t)k * 4 * no + 4 * j + i] = lam[i]; mu_out[(size_t)k * 4 * no + 4 * j + i] = muv[i]; }
  if (d) {  // the value the rows certify: -g'mu + (A t - b)'lam  (:276)
    double v = 0.0;
    for (int i = 0; i < 4; ++i) v += -sp.g[i] * muv[i] + (A[i][0] * x + A[i][1] * y - b[i]) * lam[i];
    d[(size_t)k * no + j] = v;
  }
}

// joint_dual_ws (reference multi_vehicle_planner.py:208-341): for n pairs of fixed poses of two vehicles, the duals
// lam (faces of the first), mu (faces of the second), s and the separation d of the rows
//   -b_this'lam - b_other'mu = d,  A_this'lam + s = 0,  A_other'mu - s = 0,  |s| <= 1,  lam, mu >= 0   (:292-295)
// at the optimum: d = the distance of the two bodies, s = -w with w the unit direction from this vehicle to the other.
__global__ void joint_dual_ws_kernel(const cfz::KSpec sp, int n, const double *pa, const double *pb, double *lam_o,
                                     double *mu_o, double *s_o, double *d_o) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const double x = pa[3 * k], y = pa[3 * k + 1], xo = pb[3 * k], yo = pb[3 * k + 1];
  double s, c, so, co;
  sincos(pa[3 * k + 2], &s, &c); sincos(pb[3 * k + 2], &so, &co);
  const double g0 = sp.g[0], g1 = sp.g[1], g2 = sp.g[2], g3 = sp.g[3];
  const double BV[4][2] = {{g0, g1}, {-g2, g1}, {-g2, -g3}, {g0, -g3}};
  double W[4][2], V[4][2];
  for (int i = 0; i < 4; ++i) {
    W[i][0] = x + c * BV[i][0] - s * BV[i][1]; W[i][1] = y + s * BV[i][0] + c * BV[i][1];
    V[i][0] = xo + co * BV[i][0] - so * BV[i][1]; V[i][1] = yo + so * BV[i][0] + co * BV[i][1];
  }
  double wx, wy, dist;  // w: unit direction from this vehicle towards the other
  if (!polygon_gap(W, V, wx, wy, dist)) {  // touching or overlapping: the best face normal of either body
    double A[4][2] = {{co, so}, {-so, co}, {-co, -so}, {so, -co}}, b[4], sep2[2];
    for (int i = 0; i < 4; ++i) b[i] = A[i][0] * xo + A[i][1] * yo + sp.g[i];
    const int sel = cfz::select_rows_sep(A, b, V, x, y, c, s, sp.g, 0, sep2);
    const int kind = sel >> 6, f = (sel >> 4) & 3;
    const double gx = (f == 0) - (f == 2), gy = (f == 1) - (f == 3);
    if (kind == 1) { wx = -(co * gx - so * gy); wy = -(so * gx + co * gy); }  // a face of the other body, normal towards this one
    else { wx = c * gx - s * gy; wy = s * gx + c * gy; }
  }
  double lam[4], mu[4];
  const double lx = c * wx + s * wy, ly = -s * wx + c * wy;          // R' w = G' lam
  lam[0] = fmax(lx, 0.0); lam[1] = fmax(ly, 0.0); lam[2] = fmax(-lx, 0.0); lam[3] = fmax(-ly, 0.0);
  const double mx = -(co * wx + so * wy), my = -(-so * wx + co * wy);  // Ro' (-w) = G' mu
  mu[0] = fmax(mx, 0.0); mu[1] = fmax(my, 0.0); mu[2] = fmax(-mx, 0.0); mu[3] = fmax(-my, 0.0);
  for (int i = 0; i < 4; ++i) { lam_o[4 * k + i] = lam[i]; mu_o[4 * k + i] = mu[i]; }
  s_o[2 * k] = -wx; s_o[2 * k + 1] = -wy;  // s = -A_this' lam = A_other' mu
  if (d_o) {  // -b_this'lam - b_other'mu with b = G R(-psi) t + g   (:292)
    const double tl = c * x + s * y, tm = -s * x + c * y, ol = co * xo + so * yo, om = -so * xo + co * yo;
    const double bt[4] = {tl + g0, tm + g1, -tl + g2, -tm + g3}, bo[4] = {ol + g0, om + g1, -ol + g2, -om + g3};
    double v = 0.0;
    for (int i = 0; i < 4; ++i) v -= bt[i] * lam[i] + bo[i] * mu[i];
    d_o[k] = v;
  }
}

// first prediction = the planned trajectory at the horizon times, as get_current_ref seeds it
// (:397-400); state = planned state at k0 + noise
__global__ void loop_seed(int S, int V, int N, int T, const double *ref_table, const int32_t *table_of, const int32_t *kidx,
                          const double *noise, double *pred, double *state) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (long)S * V * N) return;
  const int k = (int)(tid % N);
  const int b = (int)(tid / N);
  const int s = b / V, v = b - s * V;
  const double *tab = ref_table + (size_t)table_of[s] * V * T * 7;
  int kr = kidx[s] + k; if (kr > T - 1) kr = T - 1;
  for (int c = 0; c < 7; ++c) pred[((size_t)b * 7 + c) * N + k] = tab[((size_t)v * T + kr) * 7 + c];
  if (k == 0)
    for (int c = 0; c < 5; ++c)
      state[b * 5 + c] = tab[((size_t)v * T + kidx[s]) * 7 + c] + (noise ? noise[b * 5 + c] : 0.0);
}

// goal[S][V][3]: the last sample (x, y, psi) of the table each scenario follows.  One thread per instance.
__global__ void loop_goals(int S, int V, int T, const double *ref_table, const int32_t *table_of, double *goal) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= S * V) return;
  const int s = b / V, v = b - s * V;
  const double *last = ref_table + (((size_t)table_of[s] * V + v) * T + T - 1) * 7;
  for (int c = 0; c < 3; ++c) goal[(size_t)b * 3 + c] = last[c];
}

// ---- audit of a recorded closed loop (cfz_audit.inl) ------------------------------------------------------------------
// One wavefront per scenario; its lanes deal out the (step, item) pairs round-robin and keep the running minima in registers,
// then a butterfly over the wavefront merges them (a minimum under a total order: the same result on every run).  traj[K][S][V][7]
// from the window's first step, goal[S][V][3]; obs_in[M][n_obs] the obstacles of M maps with their normals and inverse edge lengths, il
// the body's (both formed on the host: the loop has no sqrt and no division); map_of[S] the map of every scenario (NULL: map 0), which
// its wavefront stages in LDS; clear[S][2] as audit_signed_key (the host takes the root), where[S][6] (the obstacle's index within the
// scenario's map), first_contact[S], arrive[S][V].  Plain stores, no atomics.
// cs[n][2]: cos and sin of the n = K S V headings of traj[n][7], one thread each (the audit loop itself has no transcendental)
__global__ void audit_headings(long n, const double *traj, double *cs) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s, c;
  sincos(traj[i * 7 + 2], &s, &c);
  cs[i * 2] = c; cs[i * 2 + 1] = s;
}

__global__ __launch_bounds__(64) void audit_kernel(const KArgs *__restrict__ ka, int K, int S, int V, const double *traj,
                                                   const double *cs, const double *goal, const cfz::AuditPoly *obs_in,
                                                   const int32_t *map_of, double il0, double il1, double pos_tol, double psi_tol,
                                                   double v_tol, double *clear, int32_t *where, int32_t *first_contact, int32_t *arrive) {
  __shared__ cfz::AuditPoly obs[cfz::kMaxObs];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int no = ka->sp.n_obs;
  const cfz::AuditPoly *mine = obs_in + (size_t)(map_of ? map_of[s] : 0) * no;
  if (lane < no) obs[lane] = mine[lane];
  double g[4];
  for (int i = 0; i < 4; ++i) g[i] = ka->sp.g[i];
  const double il[2] = {il0, il1};
  __syncthreads();
  cfz::AuditAcc acc;
  cfz::audit_lane(acc, lane, 64, K, V, traj + (size_t)s * V * 7, (long)S * V * 7, goal + (size_t)s * V * 3, cs + (size_t)s * V * 2, no,
                  obs, g, il, pos_tol, psi_tol, v_tol);
  cfz::wave_merge<cfz::AuditAcc, cfz::audit_merge>(acc, 64);
  if (lane == 0) cfz::audit_store(acc, V, clear + (size_t)s * 2, where + (size_t)s * 6, first_contact + s, arrive + (size_t)s * V);
}

// ---- score of a recorded closed loop (cfz_score.inl) -----------------------------------------------------------------
// One wavefront per scenario.  Vehicle v owns the L = score_group(V) lanes [v L, (v + 1) L), lane j of them the contiguous steps
// [j C, min((j + 1) C, K)), C = ceil(K / L); lanes past V L and lanes with an empty chunk hold the identity and take part in every
// shuffle.  Pass 1: the arrival, a minimum over the group.  Pass 2: every lane summarises its chunk cut at upto; the ordered butterfly of
// cfz_wave.inl merges the summaries in one fixed tree: the same bits in every lane and on every run.  traj[K][S][V][7] from the window's
// first step, cs its headings (audit_headings); status / iters point at the window's first step, steps si_stride apart (NULL: all 0);
// tables[P][V][T][7], table_of[S]; the window's k0 of scenario s is k0[s] - back.  val[S][V][kScoreNVal], cnt[S][V][kScoreNCnt],
// stored by the group's first lane with plain stores.
__global__ __launch_bounds__(64) void score_kernel(const KArgs *__restrict__ ka, int K, int S, int V, const double *traj, const double *cs,
                                                   const int32_t *status, const int32_t *iters, long si_stride, int T,
                                                   const double *tables, const int32_t *table_of, const int32_t *k0, int back, double il0,
                                                   double il1, double pos_tol, double psi_tol, double v_tol, double near2, double *val,
                                                   int32_t *cnt) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const int L = cfz::score_group(V);
  int v = 0;
  while ((v + 1) * L <= lane) ++v;
  const int j = lane - v * L;
  const bool active = v < V;
  const double il[2] = {il0, il1};
  cfz::ScoreIn in;
  cfz::score_in(in, s, active ? v : 0, K, S, V, traj, cs, status, iters, si_stride, T, tables, table_of, k0, back, ka->sp.g, il, pos_tol, psi_tol,
                v_tol, near2);
  int t0, t1;
  cfz::score_lane_chunk(K, L, j, t0, t1);
  if (!active) t0 = t1 = K;
  int arrive = cfz::score_arrive_chunk(in, t0, t1);
  for (int off = 1; off < L; off <<= 1) {
    const int o = __shfl_xor(arrive, off, 64);
    arrive = o < arrive ? o : arrive;
  }
  if (arrive == INT32_MAX) arrive = -1;
  cfz::ScoreSeg a;
  cfz::score_chunk(a, in, t0, t1, arrive);
  cfz::wave_merge_ordered<cfz::ScoreSeg, cfz::score_merge>(a, lane, L);
  if (active && j == 0)
    cfz::score_store(a, K, arrive, val + ((size_t)s * V + v) * cfz::kScoreNVal, cnt + ((size_t)s * V + v) * cfz::kScoreNCnt);
}

// ---- conflict map of a plan pool (cfz_conflict.inl) ------------------------------------------------------------------
// cols[n / T][4][T]: x, y, cos psi, sin psi of the n = P V T samples of tables[n][7] as columns, one thread per sample (the one place
// where the conflict map takes a sin / cos: P V T of them, not one per evaluation)
__global__ void conflict_columns(long n, int T, const double *tables, double *cols) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long v = i / T, t = i - v * T;
  double s, c;
  sincos(tables[i * 7 + 2], &s, &c);
  double *col = cols + v * 4 * T + t;
  col[0] = tables[i * 7]; col[T] = tables[i * 7 + 1]; col[2 * (long)T] = c; col[3 * (long)T] = s;
}

// What conflict_kernel and coord_kernel do first: one workgroup of 256 lanes per (set p, pair q = (u, w)), blockIdx.x = p npair + q; U, W
// the pair's columns in cols[P][V][4][T].  staged (T <= kConflictLdsT, 64 T bytes of dynamic LDS): copied into LDS once and read there,
// else read from global memory.  body, an always_inline lambda, is invoked once per branch: each instantiation reads U, W where they lie.
template <class Body>
__device__ __forceinline__ void pair_columns(const KArgs *__restrict__ ka, int V, int T, int staged, const double *cols, double il0, double il1,
                                             Body body) {
  extern __shared__ __attribute__((aligned(16))) double pair_lds[];
  const int npair = V * (V - 1) / 2, p = blockIdx.x / npair, q = blockIdx.x - p * npair;
  int u, w;
  cfz::conflict_pair(V, q, u, w);
  const double *U = cols + ((size_t)p * V + u) * 4 * T, *W = cols + ((size_t)p * V + w) * 4 * T;
  double g[4];
  for (int i = 0; i < 4; ++i) g[i] = ka->sp.g[i];
  const double il[2] = {il0, il1};
  if (staged) {
    for (int i = threadIdx.x; i < 4 * T; i += 256) { pair_lds[i] = U[i]; pair_lds[4 * T + i] = W[i]; }
    __syncthreads();
    body(p, q, u, w, pair_lds, pair_lds + 4 * T, g, il);
  } else {
    body(p, q, u, w, U, W, g, il);
  }
}

// the lags of one wavefront: wave k of the workgroup's four takes lags k, k + 4, ... of the 2 D + 1, its lanes the steps lane, lane + 64, ...
// of a lag; wave_merge merges the lanes (conflict_merge: the same result however the steps are dealt out), lane 0 stores with plain stores.
__device__ __forceinline__ void conflict_lags(int T, int D, const double *U, const double *W, const double g[4], const double il[2],
                                              double margin, double margin2, double *clear, int32_t *info) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int j = wave; j < 2 * D + 1; j += 4) {
    cfz::ConflictAcc acc;
    cfz::conflict_lane(acc, lane, 64, T, j - D, U, W, g, il, margin, margin2);
    cfz::wave_merge<cfz::ConflictAcc, cfz::conflict_merge>(acc, 64);
    if (lane == 0) cfz::conflict_store(acc, clear + j, info + (size_t)j * cfz::kConflictNInfo);
  }
}

// A workgroup per (set, pair) over pair_columns.  clear[P][npair][2D+1] as keys (the host takes the root), info[P][npair][2D+1][3].
__global__ __launch_bounds__(256) void conflict_kernel(const KArgs *__restrict__ ka, int V, int T, int D, int staged, const double *cols,
                                                       double il0, double il1, double margin, double margin2, double *clear, int32_t *info) {
  const size_t out = (size_t)blockIdx.x * (2 * D + 1);
  pair_columns(ka, V, T, staged, cols, il0, il1, [&](int, int, int, int, const double *U, const double *W, const double *g, const double *il) __attribute__((always_inline)) {
    conflict_lags(T, D, U, W, g, il, margin, margin2, clear + out, info + out * cfz::kConflictNInfo);
  });
}

// ---- start delays that resolve a conflict map (cfz_delay.inl) ---------------------------------------------------------
// ints per set of delay_kernel's output block: delays[V], info[3], a pad to an even count, rclear as two ints
__host__ __device__ constexpr int delay_out_ints(int V) { return ((V + cfz::kDelayNInfo + 1) & ~1) + 2; }

// One workgroup of 256 lanes per plan set; blockIdx.x = p.  count[P][npair][2D+1] with entries cs ints apart (1: a caller's map; 3 and the
// pointer at column 2: conflict_kernel's info), clear[P][npair][2D+1] or NULL (as conflict_kernel leaves it or as the caller holds it: only
// finiteness and order are read), cap[P][V] or NULL.  npair delay_words(D) words of dynamic LDS: under (D+1)^V <= 2^31 at most 11,588 B.
//   staging  a lane per (pair, lag) evaluates the window of slack r, a __ballot packs 32 lanes into a word of the pair's row;
//   shells   spans m = 0, 1, ... up to the largest cap, the candidates of a shell dealt round-robin over the lanes, merged by
//            wave_merge per wavefront and block_merge over the four (cfz_wave.inl): the decision to stop is workgroup-uniform;
//   stores   lane 0, plain stores, into one block of outputs: out[P][delay_out_ints(V)], per set the delays, info[3], a pad where V is even
//            and rclear as a double (an even number of ints per set: every rclear is aligned).
__global__ __launch_bounds__(256) void delay_kernel(int V, int D, int r, const int32_t *count, int cs, const double *clear, const int32_t *cap,
                                                    int32_t *out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t delay_lds[];
  __shared__ int xch[2][4][sizeof(cfz::DelayAcc) / 4];  // block_merge's slots
  const int p = blockIdx.x, npair = V * (V - 1) / 2, L = 2 * D + 1, nw = cfz::delay_words(D), tid = threadIdx.x;
  const int32_t *cnt = count + (size_t)p * npair * L * cs;
  const double *clr = clear ? clear + (size_t)p * npair * L : nullptr;
  const int nbit = npair * nw * 32;
  for (int base = 0; base < nbit; base += 256) {  // (every lane takes every round: the ballot is over whole wavefronts)
    const int i = base + tid, q = i / (nw * 32), j = i - q * (nw * 32);
    const bool f = i < nbit && j < L && cfz::delay_window_free(cnt + (size_t)q * L * cs, cs, clr ? clr + (size_t)q * L : nullptr, D, r, j);
    const unsigned long long b = __ballot(f);
    if ((tid & 31) == 0 && i < nbit) delay_lds[i >> 5] = (uint32_t)(b >> (tid & 32));
  }
  cfz::DelayVec capv;
  cfz::delay_pack(V, cap ? cap + (size_t)p * V : nullptr, D, capv);
  int maxcap = 0;
  for (int v = 0; v < V; ++v) maxcap = max(maxcap, cfz::delay_digit(capv, v));
  __syncthreads();
  cfz::DelayAcc best;
  cfz::delay_clear(best);
  int m = 0;
  for (; m <= maxcap; ++m) {
    cfz::DelayShell sh;
    cfz::delay_shell(V, m, sh);
    cfz::DelayAcc acc;
    cfz::delay_lane(acc, tid, 256, V, D, m, sh, capv, delay_lds, nw);
    cfz::wave_merge<cfz::DelayAcc, cfz::delay_merge>(acc, 64);
    cfz::block_merge<cfz::DelayAcc, cfz::delay_merge, 4>(best, acc, xch, m);  // (one barrier per shell)
    if (best.total != INT32_MAX) break;  // (the same for every lane)
  }
  if (tid == 0) {
    int32_t *o = out + (size_t)p * delay_out_ints(V);
    cfz::delay_store(best, V, D, m, clr, o, o + V, (double *)(o + delay_out_ints(V) - 2));
  }
}

// ---- coordination diagrams of a plan pool (cfz_coord.inl) -------------------------------------------------------------
constexpr int kCoordRows = 32;  // rows of either side that one workgroup of coord_kernel writes

// the rows blockIdx.y kCoordRows ... of both sides of one pair: a wavefront takes a row, a lane a column, a __ballot packs 64 predicates,
// lane 0 stores the row's words with plain stores (every word of every row is written: out, the pair's [2][T][words], needs no clearing).
__device__ __forceinline__ void coord_rows(int T, int lu, int lw, const double *U, const double *W, const double g[4], const double il[2],
                                           double margin, double margin2, uint32_t *out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = cfz::coord_words(T);
  const int r0 = blockIdx.y * kCoordRows, r1 = min(r0 + kCoordRows, T);
  for (int side = 0; side < 2; ++side)
    for (int row = r0 + wave; row < r1; row += 4)
      for (int c = 0; c * 64 < T; ++c) {  // (the same trip count for every lane: the ballot is over the whole wavefront)
        const bool b = cfz::coord_entry(side, T, lu, lw, row, c * 64 + lane, U, W, g, il, margin, margin2);
        const unsigned long long m = __ballot(b);
        if (lane == 0) cfz::coord_store(out + ((size_t)side * T + row) * nw, nw, c, m);
      }
}

// A workgroup per (set, pair, block of kCoordRows rows) over pair_columns.  length[P][V] or NULL (T).  diag[P][npair][2][T][words].
__global__ __launch_bounds__(256) void coord_kernel(const KArgs *__restrict__ ka, int V, int T, int staged, const double *cols,
                                                    const int32_t *length, double il0, double il1, double margin, double margin2,
                                                    uint32_t *diag) {
  pair_columns(ka, V, T, staged, cols, il0, il1, [&](int p, int q, int u, int w, const double *U, const double *W, const double *g, const double *il) __attribute__((always_inline)) {
    const int lu = length ? length[(size_t)p * V + u] : T, lw = length ? length[(size_t)p * V + w] : T;
    coord_rows(T, lu, lw, U, W, g, il, margin, margin2, diag + cfz::coord_offset(V * (V - 1) / 2, T, p, q, 0));
  });
}

// ---- hold-point schedules over the diagrams (cfz_schedule.inl) --------------------------------------------------------
// One order by one wavefront: its vehicles in turn, lane l holding word l of the reachable row.  The free words of kScheduleAhead steps
// are loaded before those steps' dependent chain (one __shfl_up, four bit operations and a store per step) runs.  hist[H][words] and
// sched[V][H] (by position in the order) are the wavefront's own, in LDS or in global memory: forced inline, so that each call reads them
// in the address space they lie in.  holdw[64] (LDS): the vehicle's hold words, for the walk back, which every lane runs alike (its
// reads are of addresses the lanes share) and lane 0 writes.  arr[16] (LDS): arrival and waits by vehicle.  -> feasible.
__device__ __forceinline__ bool schedule_order(int V, int T, int H, int r, uint32_t order, const uint32_t *diag, const int *lens,
                                               const uint8_t *hold, uint32_t *hist, uint16_t *sched, uint32_t *holdw, int *arr, int &makespan,
                                               int &total) {
  const int lane = threadIdx.x & 63, nw = cfz::coord_words(T);
  makespan = 0; total = 0;
  for (int k = 0; k < V; ++k) {
    const int v = cfz::schedule_digit(order, k), len = lens[v], g = len - 1;
    const uint32_t valid = cfz::schedule_valid_word(len, lane), hw = cfz::schedule_hold_word(hold + (size_t)v * T, len, lane);
    holdw[lane] = hw;
    auto fw = [&](int t) { return lane < nw ? cfz::schedule_free_word(diag, V, T, nw, H, r, order, k, sched, t, lane, valid) : 0u; };
    uint32_t R = cfz::schedule_first(lane, fw(0));
    if (lane < nw) hist[lane] = R;
    bool alive = true;
    for (int t0 = 1; t0 < H && alive; t0 += cfz::kScheduleAhead) {
      uint32_t fr[cfz::kScheduleAhead];
#pragma unroll
      for (int j = 0; j < cfz::kScheduleAhead; ++j) fr[j] = t0 + j < H ? fw(t0 + j) : 0u;
#pragma unroll
      for (int j = 0; j < cfz::kScheduleAhead; ++j)
        if (t0 + j < H) {
          uint32_t prev = __shfl_up(R, 1, 64);
          if (lane == 0) prev = 0u;
          R = cfz::schedule_step(R, prev, hw, fr[j]);
          if (lane < nw) hist[(size_t)(t0 + j) * nw + lane] = R;
        }
      alive = __ballot(R != 0u) != 0ull;  // (the same for every lane; an empty row stays empty)
    }
    if (!alive) return false;
    __threadfence_block();  // the rows were written by their lanes, the walk reads them from every lane
    const int a = cfz::schedule_walk(hist, nw, holdw, g, H, sched + (size_t)k * H, lane == 0);
    __threadfence_block();  // and the schedule by lane 0
    if (a < 0) return false;
    if (lane == 0) { arr[v] = a; arr[cfz::kScheduleMaxV + v] = a - g; }
    makespan = max(makespan, a); total += a;
  }
  return true;
}

// ints per set of schedule_kernel's small outputs: arrival[V], waits[V], info[5]
__host__ __device__ constexpr int schedule_out_ints(int V) { return 2 * V + cfz::kScheduleNInfo; }

// One workgroup of four wavefronts per plan set; blockIdx.x = p.  Pass 0: wavefront k takes orders k, k + 4, ... of orders[O] (packed,
// schedule_pack) and keeps its best (makespan, total, index); the four are merged by block_merge (cfz_wave.inl; schedule_merge, a total
// order: the decision is workgroup-uniform).
// Pass 1: wavefront 0 runs the winning order once more and writes schedule[P][V][H] and small[P][schedule_out_ints(V)] with plain
// stores.  in_lds: schedule_wave_words(V, T, H) words per wavefront of dynamic LDS; else ws[P][4][that many] in global memory.
// No floating point.
__global__ __launch_bounds__(256) void schedule_kernel(int V, int T, int H, int r, int O, const uint32_t *orders, const uint32_t *diag,
                                                       const int32_t *length, const uint8_t *hold, int in_lds, uint32_t *ws,
                                                       int32_t *schedule, int32_t *small) {
  extern __shared__ __attribute__((aligned(16))) uint32_t schedule_lds[];
  __shared__ uint32_t holdw[4][64];
  __shared__ int arr[4][2 * cfz::kScheduleMaxV], lens[cfz::kScheduleMaxV], xch[2][4][sizeof(cfz::ScheduleBest) / 4];  // xch: block_merge's slots
  const int p = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, npair = V * (V - 1) / 2, nw = cfz::coord_words(T);
  if (threadIdx.x < V) lens[threadIdx.x] = length ? length[(size_t)p * V + threadIdx.x] : T;
  __syncthreads();
  const size_t per = cfz::schedule_wave_words(V, T, H);
  const uint32_t *dg = diag + cfz::coord_offset(npair, T, p, 0, 0);
  const uint8_t *hd = hold + (size_t)p * V * T;
  uint32_t *gbase = in_lds ? nullptr : ws + ((size_t)p * 4 + wave) * per;
  int32_t *sm = small + (size_t)p * schedule_out_ints(V);
  cfz::ScheduleBest best;
  cfz::schedule_clear(best);
  for (int pass = 0; pass < 2; ++pass) {
    const bool found = best.makespan != INT32_MAX;  // (pass 1: the merged best, the same for every lane)
    const int first = pass == 0 ? wave : (wave == 0 && found ? best.index : O), stride = pass == 0 ? 4 : O;
    for (int o = first; o < O; o += stride) {
      int mk, tot;
      // one order over the wavefront's rows at b, written out in pass 1; forced inline, so that either call reads b where it lies
      auto run = [&](uint32_t *b) __attribute__((always_inline)) {
        uint16_t *sched = (uint16_t *)(b + (size_t)H * nw);
        const bool ok = schedule_order(V, T, H, r, orders[o], dg, lens, hd, b, sched, holdw[wave], arr[wave], mk, tot);
        if (pass == 1 && ok)
          for (int k = 0; k < V; ++k) {
            int32_t *out = schedule + ((size_t)p * V + cfz::schedule_digit(orders[o], k)) * H;
            for (int t = lane; t < H; t += 64) out[t] = sched[(size_t)k * H + t];
          }
        return ok;
      };
      const bool ok = in_lds ? run(schedule_lds + (size_t)wave * per) : run(gbase);
      if (pass == 0 && ok) cfz::schedule_take(best, mk, tot, o);
      if (pass == 1 && lane < V) { sm[lane] = arr[0][lane]; sm[V + lane] = arr[0][cfz::kScheduleMaxV + lane]; }
    }
    if (pass == 0) {
      const cfz::ScheduleBest mine = best;
      cfz::schedule_clear(best);
      cfz::block_merge<cfz::ScheduleBest, cfz::schedule_merge, 4>(best, mine, xch, 0);
    } else if (wave == 0) {
      if (!found) {
        for (int i = lane; i < V * H; i += 64) schedule[(size_t)p * V * H + i] = -1;
        if (lane < V) { sm[lane] = -1; sm[V + lane] = -1; }
      }
      if (lane == 0) cfz::schedule_info(best, sm + 2 * V);
    }
  }
}

}  // namespace

// Ownership and the commit rule.  Every device block is a DevBuf member: it goes with its owner, and a handle or a Loop that is assigned
// from a fresh one has released everything.  An entry point that allocates follows one rule:
//   Build into locals, check every step, move into the handle last.  A refused or failed call leaves the handle as it was.
// (cfz_loop_init_tables releases the old loop first, to keep peak memory: a failed init leaves no loop.  cfz_loop_run's buffers are
// work space without contents between calls: each is reserved on its own, and a call after a failure completes the set.)
struct cfz_handle {
  int device = 0, max_batch = 0;
  cfz::KSpec ks;
  cfz::Lay lay;
  cfz_spec spec0;    // what cfz_create was given: the base a pool entry is checked against and the default of its options
  cfz_options opt0;
  size_t lds_bytes = 0;
  int blocks_per_cu = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float last_ms = 0.f;
  DevBuf<double> obs_tab;  // n_obs x 20: A[4][2], b[4], V[4][2] (KSpec::obs_tab)
  DevBuf<KArgs> kargs;     // device copy of {ks, derive(ks), lay}
  // carry records (multipliers handed from one MPC iteration to the next), one per slot; per-solve flags
  DevBuf<double> wst;
  DevBuf<int32_t> carry, slots;                 // device: per-solve flags and slot ids
  DevBuf<int32_t, HipHostMem> stage_host;       // pinned staging for both (2 x max_batch): no blocking copy per solve
  hipEvent_t ev_stage = nullptr;                // the staged copy, for solves launched on a caller's stream
  int wst_stride = 0, carry_duals = 1;
  bool carry_set = false, slots_set = false, ms_pending = false;
  const int32_t *carry_ext = nullptr;           // cfz_mpc_set_carry_device: the caller's device array, for one solve
  // per-instance buffers
  DevBuf<double> x0, ref, nbr, zu, stats;
  DevBuf<int32_t> status, iters;
  DevBuf<double> l, m, lam_ij, lam_ji, s;
  // closed loop: everything cfz_loop_init_tables sets up; loop_release returns it to these defaults
  struct Loop {
    // ref_table[P][V][T][7] the pool of plan sets, table_of[S] the set of each scenario
    int S = 0, T = 0, P = 0;
    DevBuf<double> ref_table, pred, state;
    DevBuf<int32_t> kidx, order, table_of;
    bool have_order = false;
    // exchange order (cfz_loop_set_order; NULL: Jacobi): xperm[S][V] the order of every scenario, xrank[S][V] its inverse,
    // xlist[V][S] the instance ids s * V + xperm[s][r] of round r (the dispatch list of a stepwise round)
    DevBuf<int32_t> xperm, xrank, xlist;
    std::vector<int32_t> xperm_host;
    // record of the realised trajectory (cfz_loop_record): rec[rec_cap][S][V][7], rec_si[rec_cap][2][S][V]; rec_used steps written
    DevBuf<double> rec;
    DevBuf<int32_t> rec_si;
    int rec_cap = 0, rec_used = 0;  // (steps; rec_cap is set once both buffers exist)
    // disturbances (cfz_loop_set_disturbance; dz_on false: none): one device buffer dz_buf = sigma[12] | level[S] | stream[S] (uint32);
    // steps_done below is the step count of the streams.  dz_zero: the same block, all zero, from cfz_loop_init_tables on: what the kernels
    // compiled with kDist take for dz while no disturbance is set (disturb_args).  Zero sigma and level make every d a signed zero
    // whatever the stream id, and x + (+-0) is x for every x (only the sign of a zero x can follow the stream), so one block with
    // zero ids serves the comm and the pool kernels alike.
    DevBuf<double> dz_buf, dz_zero;
    uint64_t dz_seed = 0;
    bool dz_on = false;
    // lossy exchange (cfz_loop_set_comm; cm_on false: none): one device buffer cm_buf = p_drop[S] | stream[S] (uint32);
    // cm_ring[D][S][V][7][N] the ring of messages, D = cm_max_age + 2; cm_tau_on the message history starts at
    DevBuf<double> cm_buf, cm_ring;
    uint64_t cm_seed = 0;
    int cm_max_age = 0, cm_compensate = 0, cm_tau_on = 0;
    bool cm_on = false;
    // problem pool (cfz_loop_set_problems; pb_on false: none) as the user gave it: pb_user[P] the block {ks_p, derive(ks_p), lay} of every
    // problem (obs_tab the handle's), pb_user_of[S] the problem of each scenario
    std::vector<KArgs> pb_user;
    std::vector<int32_t> pb_user_of;
    bool pb_on = false;
    // map pool (cfz_loop_set_maps; mp_on false: none): mp_tab[mp_M][n_obs][20] the maps' tables in the layout of cfz_handle::obs_tab,
    // mp_poly[mp_M][n_obs] their polygons as the audit reads them, mp_of[S] the map of each scenario (device), mp_user_of the same (host)
    DevBuf<double> mp_tab;
    DevBuf<cfz::AuditPoly> mp_poly;
    DevBuf<int32_t> mp_of;
    std::vector<int32_t> mp_user_of;
    int mp_M = 0;
    bool mp_on = false;
    // what the pool kernels take while either setting is on (compose_pool): pb_pool one block per (problem, map) pair that some
    // scenario uses, its obs_tab that map's table; pb_of[S] the block of each scenario
    DevBuf<KArgs> pb_pool;
    DevBuf<int32_t> pb_of;
    // persistent loop
    DevBuf<double> pred2, scratch;
    DevBuf<int32_t> queue, ctrl, done, iter_sum;
    int steps_done = 0;
  } lp;
  long last_iter_sum = 0, last_converged = 0, last_status[6] = {0, 0, 0, 0, 0, 0};
  CfzArena arena;  // device buffers of cfz_dual_ws / cfz_joint_dual_ws, kept between calls
};

namespace {

// grid (0: B) workgroups solve the instances order[0 .. grid) of the B (order NULL: 0 .. B)
int launch_solve(cfz_handle *h, int B, const double *x0, const double *ref, const double *nbr, double *zu,
                 int32_t *status, int32_t *iters, double *stats, bool duals, hipStream_t st,
                 const int32_t *order = nullptr, int carry_all = 0, int grid = 0, bool pool = false) {
  DualPtrs du = {nullptr, nullptr, nullptr, nullptr, nullptr};
  if (duals) du = {h->l, h->m, h->lam_ij, h->lam_ji, h->s};
  if ((h->carry_set || h->slots_set) && st != h->stream) HIP_OK(hipStreamWaitEvent(st, h->ev_stage, 0));  // staged on the handle's stream
  HIP_OK(hipEventRecord(h->ev0, st));
  const int32_t *carry = h->carry_ext ? h->carry_ext : (h->carry_set ? h->carry : nullptr);
  auto launch = [&](auto kernel, auto... tail) {
    hipLaunchKernelGGL(kernel, dim3(grid ? grid : B), dim3(cfz::kNL), h->lds_bytes, st, h->kargs, B, x0, ref, nbr, zu, status, iters, stats, du,
                       order, h->carry_duals ? h->wst : nullptr, h->wst_stride, carry, carry_all, h->slots_set ? h->slots : nullptr, tail...);
  };
  if (pool)  // the stepwise closed loop under cfz_loop_set_problems / cfz_loop_set_maps: instance b solves the block of scenario b / V
    launch(solve_kernel_pool, h->lp.pb_pool.get(), h->lp.pb_of.get(), h->ks.n_nbr + 1);
  else
    launch(solve_kernel);
  h->carry_set = false; h->slots_set = false; h->carry_ext = nullptr;  // the flags of cfz_mpc_set_carry / cfz_mpc_set_slots hold for one solve
  h->ms_pending = true;
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(h->ev1, st));
  return 0;
}

int create_fill(cfz_handle *h, const cfz_spec *spec, const cfz_options *opt);

// the value checks of cfz_create on a spec's sizes and on the options (cfz_problem_check makes the same ones)
int spec_shape_ok(const cfz_spec *spec) {
  if (spec->N < 2 || spec->N > CFZ_MAX_N) return fail("N out of range");
  if (spec->n_obs < 0 || spec->n_obs > CFZ_MAX_OBS || spec->n_nbr < 0 || spec->n_nbr > CFZ_MAX_NBR)
    return fail("n_obs / n_nbr out of range");
  if (spec->N > cfz::kMaxN) return fail("N exceeds the four-lanes-per-stage kernel");
  return 0;
}

int options_ok(const cfz_options *opt) {
  if (opt->filter_cap < 1 || opt->filter_cap > 32) return fail("filter_cap must be in 1..32");
  if (opt->restoration < 0 || !(opt->reg_dual_rows >= 0.0) || !(opt->resto_first >= 0.0)) return fail("restoration, reg_dual_rows, resto_first must not be negative");
  return 0;
}

// one obstacle's 20 doubles of KSpec::obs_tab: A[4][2], b[4], V[4][2]
void obs_tab_entry(double *o, const double A[4][2], const double b[4], const double V[4][2]) {
  for (int i = 0; i < 4; ++i) { o[2 * i] = A[i][0]; o[2 * i + 1] = A[i][1]; o[8 + i] = b[i];
                                o[12 + 2 * i] = V[i][0]; o[13 + 2 * i] = V[i][1]; }
}

// the vertices V[n_obs][4][2] of a map A[n_obs][4][2], b[n_obs][4], as cfz_create forms them (quad_vertices); refused, naming the
// obstacle: an entry that is not finite, an obstacle that is no bounded quadrilateral (cfz_map_check)
int map_vertices(int n_obs, const double *A, const double *b, double (*V)[4][2]) {
  for (int j = 0; j < n_obs; ++j) {
    const double *Aj = A + (size_t)j * 8, *bj = b + (size_t)j * 4;
    bool finite = true;
    for (int i = 0; i < 8; ++i) finite = finite && std::isfinite(Aj[i]);
    for (int i = 0; i < 4; ++i) finite = finite && std::isfinite(bj[i]);
    if (!finite) return fail(("obstacle " + std::to_string(j) + " has an entry that is not finite").c_str());
    if (!quad_vertices(reinterpret_cast<const double(*)[2]>(Aj), bj, V[j]))
      return fail(("obstacle " + std::to_string(j) + " is not a bounded quadrilateral").c_str());
  }
  return 0;
}

// the kernel's form of (spec, opt), obs_tab left NULL; refused: an obstacle that is no bounded quadrilateral
int fill_kspec(cfz::KSpec &k, const cfz_spec *spec, const cfz_options *opt) {
  memset(&k, 0, sizeof k);
  k.N = spec->N; k.n_obs = spec->n_obs; k.n_nbr = spec->n_nbr; k.rk_substeps = spec->rk_substeps;
  k.max_iter = opt->max_iter; k.max_backtrack = opt->max_backtrack; k.filter_cap = opt->filter_cap;
  k.dt = spec->dt; k.wb = spec->wb; k.dmin = spec->dmin;
  memcpy(k.g, spec->g, sizeof k.g); memcpy(k.bounds, spec->bounds, sizeof k.bounds);
  memcpy(k.weights, spec->weights, sizeof k.weights);
  for (int j = 0; j < spec->n_obs; ++j) {
    memcpy(k.A_obs[j], spec->A_obs[j], sizeof k.A_obs[j]); memcpy(k.b_obs[j], spec->b_obs[j], sizeof k.b_obs[j]);
    if (!quad_vertices(spec->A_obs[j], spec->b_obs[j], k.V_obs[j])) return fail("obstacle is not a bounded quadrilateral");
  }
  k.tol = opt->tol; k.constr_viol_tol = opt->constr_viol_tol; k.dual_inf_tol = opt->dual_inf_tol;
  k.compl_inf_tol = opt->compl_inf_tol; k.mu_init = opt->mu_init; k.kappa_eps = opt->kappa_eps;
  k.kappa_mu = opt->kappa_mu; k.theta_mu = opt->theta_mu; k.tau_min = opt->tau_min; k.bound_push = opt->bound_push;
  k.bound_frac = opt->bound_frac; k.s_max = opt->s_max; k.kappa_sigma = opt->kappa_sigma; k.eta_phi = opt->eta_phi;
  k.gamma_theta = opt->gamma_theta; k.gamma_phi = opt->gamma_phi; k.delta_sw = opt->delta_sw;
  k.s_theta = opt->s_theta; k.s_phi = opt->s_phi; k.reg_primal = opt->reg_primal;
  k.stall_iters = opt->stall_iters; k.stall_kappa = opt->stall_kappa; k.row_curvature = opt->row_curvature; k.vv_rows = opt->vv_rows; k.shift_after = opt->shift_after; k.resto = opt->restoration; k.stag_win = opt->shift_stagnation; k.err_stall = opt->err_stall_iters; k.carry_shift = opt->carry_shift ? 1 : 0; k.pad_ks = 0; k.warm_push = opt->warm_push; k.reg_dual_rows = opt->reg_dual_rows; k.resto_first = opt->resto_first;
  return 0;
}

int check(cfz_handle *h, int B) {
  if (!h) return fail("null handle");
  if (B < 1 || B > h->max_batch) return fail("batch size out of range");
  HIP_OK(hipSetDevice(h->device));
  return 0;
}

// `count` elements of the caller's host array on the device: from the handle's arena, copied on its stream (nothing is waited for)
template <class T>
int arena_upload(cfz_handle *h, T *&dptr, const T *host, size_t count) {
  ARENA_ALLOC(h->arena, dptr, count * sizeof(T));
  HIP_OK(hipMemcpyAsync(dptr, host, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
  return 0;
}

}  // namespace

extern "C" {

const char *cfz_last_error(void) { return cfz_g_err.c_str(); }

#ifndef CFZ_SRC_HASH
#define CFZ_SRC_HASH "unknown"
#endif
const char *cfz_source_hash(void) { return CFZ_SRC_HASH; }

void cfz_default_spec(cfz_spec *s) {
  memset(s, 0, sizeof *s);
  s->N = 30; s->n_obs = 0; s->n_nbr = 0; s->rk_substeps = 4;
  s->dt = 0.1; s->wb = 2.5; s->dmin = 0.05;
  const double g[4] = {3.3, 0.9, 0.6, 0.9};
  const double bd[12] = {2.5, 32.5, 7.5, 27.5, -2.5, 2.5, -0.85, 0.85, -1.5, 1.5, -1.0, 1.0};
  const double w[6] = {100, 100, 100, 1, 1, 1};
  memcpy(s->g, g, sizeof g); memcpy(s->bounds, bd, sizeof bd); memcpy(s->weights, w, sizeof w);
}

void cfz_default_options(cfz_options *o) {
  memset(o, 0, sizeof *o);
  o->max_iter = 600; o->max_backtrack = 25; o->filter_cap = 16;
  o->tol = 1e-2; o->constr_viol_tol = 1e-2; o->dual_inf_tol = 1.0; o->compl_inf_tol = 1e-4;
  o->mu_init = 1e-3; o->kappa_eps = 10.0; o->kappa_mu = 0.2; o->theta_mu = 1.5; o->tau_min = 0.99;
  o->bound_push = 1e-2; o->bound_frac = 1e-2; o->s_max = 100.0; o->kappa_sigma = 1e10;
  o->eta_phi = 1e-8; o->gamma_theta = 1e-5; o->gamma_phi = 1e-8; o->delta_sw = 1.0; o->s_theta = 1.1; o->s_phi = 2.3;
  o->reg_primal = 1e-8;
  o->stall_iters = 10; o->stall_kappa = 0.9; o->row_curvature = 1; o->carry_duals = 1; o->vv_rows = 1; o->shift_after = 60; o->restoration = 2; o->shift_stagnation = 10; o->err_stall_iters = 150; o->carry_shift = 1; o->warm_push = 1e-6;
  o->reg_dual_rows = 1e-8; o->resto_first = 0.3;
}

int cfz_create(const cfz_spec *spec, const cfz_options *opt, int device, int max_batch, cfz_handle **out) {
  if (!spec || !out) return fail("null argument");
  cfz_options od;
  if (!opt) { cfz_default_options(&od); opt = &od; }
  if (spec_shape_ok(spec)) return -1;
  if (max_batch < 1) return fail("max_batch must be positive");
  if (options_ok(opt)) return -1;
  int ndev = 0;
  HIP_OK(hipGetDeviceCount(&ndev));
  if (ndev == 0) return fail("no HIP device: libconfrez_hip has no CPU path");
  if (device < 0 || device >= ndev) return fail("device index out of range");
  HIP_OK(hipSetDevice(device));

  cfz_handle *h = new cfz_handle();
  h->device = device; h->max_batch = max_batch;
  if (create_fill(h, spec, opt) != 0) { cfz_destroy(h); return -1; }  // g_err is set; everything allocated so far is released
  *out = h;
  return 0;
}

}  // extern "C"

namespace {
int create_fill(cfz_handle *h, const cfz_spec *spec, const cfz_options *opt) {
  const int max_batch = h->max_batch;
  cfz::KSpec &k = h->ks;
  if (fill_kspec(k, spec, opt)) return -1;
  h->spec0 = *spec; h->opt0 = *opt;
  h->lay = cfz::make_layout(k.N, k.n_obs + k.n_nbr, k.n_nbr);
  h->lds_bytes = (size_t)h->lay.total * sizeof(double);
  if (h->lds_bytes > 160 * 1024) return fail("problem does not fit the 160 KiB LDS of one CU");
  if (h->lds_bytes > 64 * 1024) {
    // (a guard: no shape the ABI admits gets here -- the widest, N 32 with 8 obstacles and 7 neighbours, takes 60,216 B
    // (tools/src/loop_variant_check.hip prints it) -- and nothing else changes lds_bytes)
    std::vector<const void *> kerns = {(const void *)solve_kernel, (const void *)solve_kernel_pool};
    for (const LoopVariant &v : kLoopVariants) kerns.push_back(v.fn);
    for (const void *kern : kerns) {
      const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_bytes);
      if (e != hipSuccess) return fail("hipFuncSetAttribute(MaxDynamicSharedMemorySize)", e);
    }
  }
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&h->blocks_per_cu, (const void *)solve_kernel, cfz::kNL, h->lds_bytes);
  {
    // The runtime's answer ignores that gfx950 hands out LDS in 2 KiB granules (measured with tools/src/occupancy_test.hip:
    // 54,208 B per workgroup -> the query says 3 per CU, 2 run); report what the hardware does.
    const int granules = (int)((h->lds_bytes + 2047) / 2048);
    const int by_lds = granules ? (160 * 1024 / 2048) / granules : h->blocks_per_cu;
    if (by_lds < h->blocks_per_cu) h->blocks_per_cu = by_lds;
  }
  const size_t B = (size_t)max_batch, N = (size_t)k.N, no = (size_t)k.n_obs, nn = (size_t)k.n_nbr;
  HIP_OK(hipStreamCreate(&h->stream));
  {
    std::vector<double> tab((size_t)std::max(k.n_obs, 1) * 20, 0.0);
    for (int j = 0; j < k.n_obs; ++j) obs_tab_entry(tab.data() + (size_t)j * 20, k.A_obs[j], k.b_obs[j], k.V_obs[j]);
    if (h->obs_tab.alloc(tab.size()) || h->kargs.alloc(1)) return -1;
    HIP_OK(hipMemcpy(h->obs_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
    h->ks.obs_tab = h->obs_tab;
    KArgs host_args = {h->ks, cfz::derive(h->ks), h->lay};
    HIP_OK(hipMemcpy(h->kargs, &host_args, sizeof(KArgs), hipMemcpyHostToDevice));
  }
  h->carry_duals = opt->carry_duals;
  h->wst_stride = cfz::carry_layout(k.N, k.n_obs + k.n_nbr).stride;
  if (h->wst.alloc((size_t)max_batch * h->wst_stride)) return -1;
  HIP_OK(hipMemset(h->wst, 0, (size_t)max_batch * h->wst_stride * 8));
  if (h->carry.alloc(B) || h->slots.alloc(B) || h->stage_host.alloc(B * 2)) return -1;
  HIP_OK(hipEventCreate(&h->ev0)); HIP_OK(hipEventCreate(&h->ev1)); HIP_OK(hipEventCreateWithFlags(&h->ev_stage, hipEventDisableTiming));
  if (h->x0.alloc(B * 5) || h->ref.alloc(B * 3 * N) || h->nbr.alloc(B * nn * 3 * N + 1) || h->zu.alloc(B * 7 * N)) return -1;
  // stats: 3 doubles per instance (+ 24 phase counters per instance for the -DCFZ_STAMPS diagnostic build)
  if (h->stats.alloc(B * (3 + 24)) || h->status.alloc(B) || h->iters.alloc(B)) return -1;
  if (h->l.alloc(B * N * 4 * no + 1) || h->m.alloc(B * N * 4 * no + 1)) return -1;
  if (h->lam_ij.alloc(B * nn * N * 4 + 1) || h->lam_ji.alloc(B * nn * N * 4 + 1) || h->s.alloc(B * nn * N * 2 + 1)) return -1;
  HIP_OK(hipMemset(h->status, 0, B * 4)); HIP_OK(hipMemset(h->iters, 0, B * 4));
  return 0;
}
}  // namespace

extern "C" {

int cfz_destroy(cfz_handle *h) {
  if (!h) return 0;
  hipSetDevice(h->device);
  if (h->ev0) hipEventDestroy(h->ev0);
  if (h->ev1) hipEventDestroy(h->ev1);
  if (h->ev_stage) hipEventDestroy(h->ev_stage);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;  // (the buffers, the loop's and the arena's go with it)
  return 0;
}

int cfz_max_batch(const cfz_handle *h) { return h ? h->max_batch : 0; }

int cfz_kernel_info(const cfz_handle *h, int32_t *lds_bytes_per_instance, int32_t *instances_per_cu) {
  if (!h) return fail("null handle");
  if (lds_bytes_per_instance) *lds_bytes_per_instance = (int32_t)h->lds_bytes;
  if (instances_per_cu) *instances_per_cu = h->blocks_per_cu;
  return 0;
}

int cfz_mpc_set_params(cfz_handle *h, int B, const double *x0, const double *ref, const double *nbr) {
  if (check(h, B)) return -1;
  if (!x0 || !ref || (h->ks.n_nbr && !nbr)) return fail("null parameter array");
  const size_t N = h->ks.N, nn = h->ks.n_nbr;
  HIP_OK(hipMemcpyAsync(h->x0, x0, (size_t)B * 5 * 8, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(h->ref, ref, (size_t)B * 3 * N * 8, hipMemcpyHostToDevice, h->stream));
  if (nn) HIP_OK(hipMemcpyAsync(h->nbr, nbr, (size_t)B * nn * 3 * N * 8, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int cfz_mpc_set_warm(cfz_handle *h, int B, const double *zu) {
  if (check(h, B)) return -1;
  if (!zu) return fail("null warm start");
  HIP_OK(hipMemcpyAsync(h->zu, zu, (size_t)B * 7 * h->ks.N * 8, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int cfz_mpc_set_carry(cfz_handle *h, int B, const int32_t *carry) {
  if (check(h, B)) return -1;
  if (!carry) { h->carry_set = false; return 0; }
  // staged through pinned memory and copied on the handle's stream, so the caller's array is free at once and no
  // device-wide synchronisation happens; the stream is drained first because the staging buffer may still be feeding
  // the previous copy (free after cfz_mpc_solve, which ends synchronised).  Device-resident loops that cannot afford
  // the drain pass their flags with cfz_mpc_set_carry_device.
  HIP_OK(hipStreamSynchronize(h->stream));
  memcpy(h->stage_host, carry, (size_t)B * 4);
  HIP_OK(hipMemcpyAsync(h->carry, h->stage_host, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipEventRecord(h->ev_stage, h->stream));
  h->carry_set = true;
  return 0;
}

int cfz_mpc_set_carry_device(cfz_handle *h, int B, const int32_t *d_carry) {
  if (check(h, B)) return -1;
  h->carry_ext = d_carry;  // read by the next solve kernel on whatever stream it is launched on; nothing is copied
  return 0;
}

int cfz_mpc_set_slots(cfz_handle *h, int B, const int32_t *slots) {
  if (check(h, B)) return -1;
  if (!slots) { h->slots_set = false; return 0; }
  for (int b = 0; b < B; ++b) if (slots[b] < 0 || slots[b] >= h->max_batch) return fail("slot index out of range");
  {  // two instances of one launch on the same carry record would race on it (and mix two vehicles' multipliers)
    std::vector<char> seen((size_t)h->max_batch, 0);
    for (int b = 0; b < B; ++b) { if (seen[slots[b]]) return fail("duplicate carry slot within one solve"); seen[slots[b]] = 1; }
  }
  HIP_OK(hipStreamSynchronize(h->stream));
  int32_t *stage = h->stage_host + h->max_batch;
  memcpy(stage, slots, (size_t)B * 4);
  HIP_OK(hipMemcpyAsync(h->slots, stage, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipEventRecord(h->ev_stage, h->stream));
  h->slots_set = true;
  return 0;
}

int cfz_mpc_solve(cfz_handle *h, int B) {
  if (check(h, B)) return -1;
  if (launch_solve(h, B, h->x0, h->ref, h->nbr, h->zu, h->status, h->iters, h->stats, true, h->stream)) return -1;
  HIP_OK(hipStreamSynchronize(h->stream));
  HIP_OK(hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
  h->ms_pending = false;
  return 0;
}

int cfz_mpc_get(cfz_handle *h, int B, double *zu, double *l, double *m, double *lam_ij, double *lam_ji, double *s) {
  if (check(h, B)) return -1;
  const size_t N = h->ks.N, no = h->ks.n_obs, nn = h->ks.n_nbr, b = (size_t)B;
  if (zu) HIP_OK(hipMemcpy(zu, h->zu, b * 7 * N * 8, hipMemcpyDeviceToHost));
  if (l && no) HIP_OK(hipMemcpy(l, h->l, b * N * 4 * no * 8, hipMemcpyDeviceToHost));
  if (m && no) HIP_OK(hipMemcpy(m, h->m, b * N * 4 * no * 8, hipMemcpyDeviceToHost));
  if (lam_ij && nn) HIP_OK(hipMemcpy(lam_ij, h->lam_ij, b * nn * N * 4 * 8, hipMemcpyDeviceToHost));
  if (lam_ji && nn) HIP_OK(hipMemcpy(lam_ji, h->lam_ji, b * nn * N * 4 * 8, hipMemcpyDeviceToHost));
  if (s && nn) HIP_OK(hipMemcpy(s, h->s, b * nn * N * 2 * 8, hipMemcpyDeviceToHost));
  return 0;
}

int cfz_mpc_stats(cfz_handle *h, int B, int32_t *status, int32_t *iters, double *cost, double *kkt_err, double *min_sep) {
  if (check(h, B)) return -1;
  if (status) HIP_OK(hipMemcpy(status, h->status, (size_t)B * 4, hipMemcpyDeviceToHost));
  if (iters) HIP_OK(hipMemcpy(iters, h->iters, (size_t)B * 4, hipMemcpyDeviceToHost));
  if (cost || kkt_err || min_sep) {
    std::vector<double> st((size_t)B * 3);
    HIP_OK(hipMemcpy(st.data(), h->stats, (size_t)B * 3 * 8, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b) {
      if (cost) cost[b] = st[b * 3];
      if (kkt_err) kkt_err[b] = st[b * 3 + 1];
      if (min_sep) min_sep[b] = st[b * 3 + 2];
    }
  }
  return 0;
}

double cfz_last_solve_ms(const cfz_handle *h_) {
  cfz_handle *h = const_cast<cfz_handle *>(h_);
  if (!h) return -1.0;
  if (h->ms_pending) {  // launched through cfz_mpc_solve_device: the events have not been read yet
    if (hipSetDevice(h->device) == hipSuccess && hipEventSynchronize(h->ev1) == hipSuccess)
      (void)hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1);
    h->ms_pending = false;
  }
  return (double)h->last_ms;
}

#ifdef CFZ_STAMPS
// diagnostic build only: the 24 phase counters of every instance of the last solve_kernel launch
int cfz_debug_stamps(cfz_handle *h, int B, unsigned long long *out) {
  if (check(h, B)) return -1;
  HIP_OK(hipMemcpy(out, h->stats + (size_t)B * 3, (size_t)B * 24 * 8, hipMemcpyDeviceToHost));
  return 0;
}
#endif

int cfz_mpc_solve_device(cfz_handle *h, int B, const double *d_x0, const double *d_ref, const double *d_nbr,
                         double *d_zu, int32_t *d_status, int32_t *d_iters, double *d_stats, void *stream) {
  if (check(h, B)) return -1;
  if (!d_x0 || !d_ref || !d_zu || !d_status || !d_iters || !d_stats) return fail("null device pointer");
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  return launch_solve(h, B, d_x0, d_ref, d_nbr ? d_nbr : h->nbr, d_zu, d_status, d_iters, d_stats, false, st);
}

int cfz_vsl_step(cfz_handle *h, int S, int V, int n_own, const int32_t *d_own, int T, const double *d_table, const int32_t *d_k0,
                 int t, const double *d_allpred, double *d_pred, double *d_state, int32_t *d_status, int32_t *d_iters,
                 double *d_stats, int32_t *d_carry, void *stream) {
  if (S < 1 || n_own < 1 || check(h, S * n_own)) return fail("S * n_own outside the handle's batch");
  if (V != h->ks.n_nbr + 1) return fail("V must be n_nbr + 1 of the handle's spec");
  if (!d_own || !d_table || !d_k0 || !d_allpred || !d_pred || !d_state || !d_status || !d_iters || !d_stats || !d_carry)
    return fail("null device pointer");
  hipStream_t st = stream ? (hipStream_t)stream : h->stream;
  const int N = h->ks.N, B = S * n_own;
  const long nt = (long)B * N;
  hipLaunchKernelGGL(vs_prep, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, S, V, n_own, N, T, d_own, d_table, d_k0, t, d_allpred,
                     d_pred, d_state, h->x0, h->ref, h->nbr, h->zu);
  HIP_OK(hipGetLastError());
  h->carry_ext = t > 0 ? d_carry : nullptr;  // iteration 0 has nothing to carry
  if (launch_solve(h, B, h->x0, h->ref, h->nbr, h->zu, d_status, d_iters, d_stats, false, st)) return -1;
  hipLaunchKernelGGL(loop_post, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, S, n_own, N, h->kargs, d_status, nullptr, h->zu, d_pred,
                     d_state, nullptr, nullptr, nullptr, 0, nullptr, cfz::disturb_none(), 0, d_carry, nullptr, nullptr, nullptr);
  HIP_OK(hipGetLastError());
  return 0;
}

int cfz_dual_ws(cfz_handle *h, int n, const double *poses, double *l, double *m, double *d) {
  if (!h) return fail("null handle");
  if (n < 1 || !poses || !l || !m) return fail("bad argument");
  HIP_OK(hipSetDevice(h->device));
  const size_t no = h->ks.n_obs;
  if (no == 0) return 0;
  double *dp = nullptr, *dl = nullptr, *dm = nullptr, *dd = nullptr;
  if (arena_reset(h->arena)) return -1;
  ARENA_ALLOC(h->arena, dp, (size_t)n * 3 * 8); ARENA_ALLOC(h->arena, dl, (size_t)n * 4 * no * 8);
  ARENA_ALLOC(h->arena, dm, (size_t)n * 4 * no * 8); ARENA_ALLOC(h->arena, dd, (size_t)n * no * 8);
  HIP_OK(hipMemcpyAsync(dp, poses, (size_t)n * 3 * 8, hipMemcpyHostToDevice, h->stream));
  const int nt = n * (int)no;
  hipLaunchKernelGGL(dual_ws_kernel, dim3((nt + 127) / 128), dim3(128), 0, h->stream, h->ks, n, dp, dl, dm, dd);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(l, dl, (size_t)n * 4 * no * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipMemcpyAsync(m, dm, (size_t)n * 4 * no * 8, hipMemcpyDeviceToHost, h->stream));
  if (d) HIP_OK(hipMemcpyAsync(d, dd, (size_t)n * no * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int cfz_joint_dual_ws(cfz_handle *h, int n, const double *poses_this, const double *poses_other, double *lam, double *mu,
                      double *s, double *d) {
  if (!h) return fail("null handle");
  if (n < 1 || !poses_this || !poses_other || !lam || !mu || !s) return fail("bad argument");
  HIP_OK(hipSetDevice(h->device));
  double *dpa = nullptr, *dpb = nullptr, *dout = nullptr;
  if (arena_reset(h->arena)) return -1;
  ARENA_ALLOC(h->arena, dpa, (size_t)n * 3 * 8); ARENA_ALLOC(h->arena, dpb, (size_t)n * 3 * 8); ARENA_ALLOC(h->arena, dout, (size_t)n * 11 * 8);
  HIP_OK(hipMemcpyAsync(dpa, poses_this, (size_t)n * 3 * 8, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(dpb, poses_other, (size_t)n * 3 * 8, hipMemcpyHostToDevice, h->stream));
  double *dl = dout, *dm = dout + (size_t)n * 4, *ds = dout + (size_t)n * 8, *dd = dout + (size_t)n * 10;
  hipLaunchKernelGGL(joint_dual_ws_kernel, dim3((n + 127) / 128), dim3(128), 0, h->stream, h->ks, n, dpa, dpb, dl, dm, ds, dd);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(lam, dl, (size_t)n * 4 * 8, hipMemcpyDeviceToHost, h->stream)); HIP_OK(hipMemcpyAsync(mu, dm, (size_t)n * 4 * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipMemcpyAsync(s, ds, (size_t)n * 2 * 8, hipMemcpyDeviceToHost, h->stream));
  if (d) HIP_OK(hipMemcpyAsync(d, dd, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

}  // extern "C"

namespace {
// the pool kernels run (solve_kernel_pool, the pool rows of kLoopVariants, loop_post on the pool) whenever either setting is on
bool pool_on(const cfz_handle *h) { return h->lp.pb_on || h->lp.mp_on; }

// every closed-loop buffer, setting, size and counter goes back to the defaults of cfz_handle::Loop
void loop_release(cfz_handle *h) { h->lp = cfz_handle::Loop(); }

// the disturbance in force as the kernels take it (sigma NULL: none).  zero_if_off: for a kernel compiled with kDist that stands in
// for one without (the comm and the pool kernels): the all-zero block instead of none
cfz::DisturbArgs disturb_args(const cfz_handle *h, bool zero_if_off = false) {
  if (!h->lp.dz_on && !zero_if_off) return cfz::disturb_none();
  const double *f = h->lp.dz_on ? h->lp.dz_buf : h->lp.dz_zero;
  return {h->lp.dz_on ? h->lp.dz_seed : 0, f, f + cfz::kDisturbN, reinterpret_cast<const uint32_t *>(f + cfz::kDisturbN + h->lp.S)};
}

// the comm setting in force as the kernels take it (p_drop NULL: none)
cfz::CommArgs comm_args(const cfz_handle *h) {
  if (!h->lp.cm_on) return cfz::comm_none();
  const double *f = h->lp.cm_buf;
  const size_t S = (size_t)h->lp.S;
  return {h->lp.cm_seed, f, reinterpret_cast<const uint32_t *>(f + S), h->lp.cm_ring, h->lp.cm_max_age, h->lp.cm_compensate, h->lp.cm_tau_on,
          S * (h->ks.n_nbr + 1) * 7 * h->ks.N};
}

// what opens the closed loop's entry points: a handle whose loop is set up, its device current and (drain) its stream idle
int loop_ready(cfz_handle *h, bool drain = false) {
  if (!h || !h->lp.pred) return fail("cfz_loop_init has not been called");
  HIP_OK(hipSetDevice(h->device));
  if (drain) HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

// the device block of a setting, f | stream[S] (uint32; NULL: scenario s draws from stream s), in a block of its own: the caller moves
// it into the handle once its call is complete
int upload_setting(const cfz_handle *h, DevBuf<double> &buf, const std::vector<double> &f, const uint32_t *stream) {
  std::vector<uint32_t> id((size_t)h->lp.S);
  for (size_t s = 0; s < id.size(); ++s) id[s] = stream ? stream[s] : (uint32_t)s;
  if (buf.alloc(f.size() + (id.size() + 1) / 2)) return -1;
  HIP_OK(hipMemcpy(buf, f.data(), f.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(buf + f.size(), id.data(), id.size() * 4, hipMemcpyHostToDevice));
  return 0;
}

// the slot of message tau in the ring (comm on)
double *comm_message(const cfz_handle *h, int tau) {
  return h->lp.cm_ring + (size_t)cfz::comm_slot(tau, h->lp.cm_max_age) * comm_args(h).slot_stride;
}

// room for `steps` more steps in the record (or no record at all)
int record_room(cfz_handle *h, int steps) {
  if (h->lp.rec_cap && h->lp.rec_used + steps > h->lp.rec_cap) return fail("the step(s) would overflow the record (cfz_loop_record)");
  return 0;
}

// the slice of the step about to be written in rec and rec_si (NULL: no record is kept)
void record_slice(const cfz_handle *h, double *&rec, int32_t *&rec_si) {
  const size_t B = (size_t)h->lp.S * (h->ks.n_nbr + 1);
  rec = h->lp.rec ? h->lp.rec + (size_t)h->lp.rec_used * B * 7 : nullptr;
  rec_si = h->lp.rec ? h->lp.rec_si + (size_t)h->lp.rec_used * 2 * B : nullptr;
}

// One round of a stepwise iteration (cfz_loop_step): loop_prep, solve_kernel (solve_kernel_pool while a problem pool or a map pool is set), loop_post for n_inst instances.  Jacobi: all B of them,
// xperm and xrank NULL; round r of the sequential exchange: the S vehicles of rank r.  dispatch (NULL: index order) lists the instance
// ids in the order the solve's workgroups take them; the carry slot of instance b is b either way.
int loop_round(cfz_handle *h, int r, int n_inst, const int32_t *dispatch, const int32_t *xperm, const int32_t *xrank) {
  const int V = h->ks.n_nbr + 1, N = h->ks.N, S = h->lp.S;
  double *rec; int32_t *rec_si;
  record_slice(h, rec, rec_si);
  const cfz::DisturbArgs dz = disturb_args(h);
  const cfz::CommArgs cm = comm_args(h);
  const long nt = (long)n_inst * N;
  hipLaunchKernelGGL(loop_prep, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, h->stream, S, V, N, h->lp.T, h->lp.ref_table,
                     h->lp.table_of, h->lp.kidx, h->lp.pred, h->lp.state, h->x0, h->ref, h->nbr, h->zu, r, xperm, xrank, dz, h->lp.steps_done, cm);
  HIP_OK(hipGetLastError());
  const bool pool = pool_on(h);  // the scenario's own problem on its own map: solve_kernel_pool, and its input box in loop_post
  if (launch_solve(h, S * V, h->x0, h->ref, h->nbr, h->zu, h->status, h->iters, h->stats, false, h->stream, dispatch, 1, n_inst, pool)) return -1;
  hipLaunchKernelGGL(loop_post, dim3((unsigned)((n_inst + 63) / 64)), dim3(64), 0, h->stream, S, V, N, h->kargs, h->status, h->iters, h->zu,
                     h->lp.pred, h->lp.state, h->lp.kidx, rec, rec_si, r, xperm, dz, h->lp.steps_done, nullptr,
                     h->lp.cm_on ? comm_message(h, h->lp.steps_done) : nullptr, pool ? h->lp.pb_pool : nullptr, pool ? h->lp.pb_of : nullptr);
  HIP_OK(hipGetLastError());
  return 0;
}

// the obstacles of one map (vertices V[n_obs][4][2], counter-clockwise as quad_vertices leaves them) with their face normals and
// inverse edge lengths, as audit_kernel reads them
void audit_polys(int no, const double (*V)[4][2], cfz::AuditPoly *ob) {
  for (int j = 0; j < no; ++j) {
    memcpy(ob[j].v, V[j], sizeof ob[j].v);
    cfz::audit_poly_prepare(ob[j]);
  }
}

// d_obs[M][n_obs] the prepared polygons of the maps and d_map_of[S] (device; both NULL: every scenario against the handle's map, whose
// polygons are formed here); d_map_of NULL with d_obs set: every scenario against map 0 of d_obs
int audit_launch(cfz_handle *h, int K, int S, int V, const double *d_traj, const double *d_goal, const cfz::AuditPoly *d_obs,
                 const int32_t *d_map_of, double pos_tol, double psi_tol, double v_tol, double *clear, int32_t *where,
                 int32_t *first_contact, int32_t *arrive) {
  const int no = h->ks.n_obs;
  std::vector<cfz::AuditPoly> ob((size_t)std::max(no, 1));
  const double *g = h->ks.g;  // the body's edge lengths are formed here as well
  double *dc = nullptr, *dcs = nullptr;
  int32_t *di = nullptr;
  const long n = (long)K * S * V;
  ARENA_ALLOC(h->arena, dc, (size_t)S * 2 * 8); ARENA_ALLOC(h->arena, di, (size_t)S * (7 + V) * 4);
  ARENA_ALLOC(h->arena, dcs, (size_t)n * 2 * 8);
  if (!d_obs) {
    cfz::AuditPoly *dob = nullptr;
    audit_polys(no, h->ks.V_obs, ob.data());
    if (arena_upload(h, dob, ob.data(), ob.size())) return -1;
    d_obs = dob;
  }
  int32_t *dw = di, *df = di + (size_t)S * 6, *da = di + (size_t)S * 7;
  hipLaunchKernelGGL(audit_headings, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, d_traj, dcs);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(audit_kernel, dim3(S), dim3(64), 0, h->stream, h->kargs, K, S, V, d_traj, dcs, d_goal, d_obs, d_map_of,
                     cfz::audit_body_il(g, 0), cfz::audit_body_il(g, 1), pos_tol, psi_tol, v_tol, dc, dw, df, da);
  HIP_OK(hipGetLastError());
  if (clear) HIP_OK(hipMemcpyAsync(clear, dc, (size_t)S * 2 * 8, hipMemcpyDeviceToHost, h->stream));
  if (where) HIP_OK(hipMemcpyAsync(where, dw, (size_t)S * 6 * 4, hipMemcpyDeviceToHost, h->stream));
  if (first_contact) HIP_OK(hipMemcpyAsync(first_contact, df, (size_t)S * 4, hipMemcpyDeviceToHost, h->stream));
  if (arrive) HIP_OK(hipMemcpyAsync(arrive, da, (size_t)S * V * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));  // (also keeps `ob` alive until its copy is done)
  if (clear)
    for (int i = 0; i < 2 * S; ++i) clear[i] = cfz::audit_key_distance(clear[i]);
  return 0;
}

// the score of K steps of S scenarios x V vehicles that lie on the device (score_kernel); val, cnt are the caller's host arrays
int score_launch(cfz_handle *h, int K, int S, int V, const double *d_traj, const int32_t *d_status, const int32_t *d_iters, long si_stride,
                 int T, const double *d_tables, const int32_t *d_table_of, const int32_t *d_k0, int back, double pos_tol, double psi_tol,
                 double v_tol, double near, double *val, int32_t *cnt) {
  static_assert(cfz::kScoreNVal == CFZ_SCORE_NVAL && cfz::kScoreNCnt == CFZ_SCORE_NCNT, "cfz_score.inl and confrez_hip.h disagree");
  const double *g = h->ks.g;
  const long n = (long)K * S * V;
  const size_t B = (size_t)S * V;
  double *dcs = nullptr, *dv = nullptr;
  int32_t *dc = nullptr;
  ARENA_ALLOC(h->arena, dcs, (size_t)n * 2 * 8); ARENA_ALLOC(h->arena, dv, B * CFZ_SCORE_NVAL * 8); ARENA_ALLOC(h->arena, dc, B * CFZ_SCORE_NCNT * 4);
  hipLaunchKernelGGL(audit_headings, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, d_traj, dcs);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(score_kernel, dim3(S), dim3(64), 0, h->stream, h->kargs, K, S, V, d_traj, dcs, d_status, d_iters, si_stride, T, d_tables,
                     d_table_of, d_k0, back, cfz::audit_body_il(g, 0), cfz::audit_body_il(g, 1), pos_tol, psi_tol, v_tol, near * near, dv, dc);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(val, dv, B * CFZ_SCORE_NVAL * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipMemcpyAsync(cnt, dc, B * CFZ_SCORE_NCNT * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

// what cfz_loop_history, cfz_loop_audit and cfz_loop_score ask of the handle: a loop that is set up and the window [t0, t0 + K) in its record
int record_window(cfz_handle *h, int t0, int K) {
  if (loop_ready(h)) return -1;
  return t0 < 0 || K < 1 || t0 + K > h->lp.rec_used ? fail("steps [t0, t0 + K) are not in the record") : 0;
}

// a caller's trajectory traj[K][S][V][7] (cfz_audit_maps, cfz_score): its sizes, and that every index of the kernels fits an int.  Two
// functions: both entry points refuse null pointers between the two, each in its own words.
int traj_dims(int K, int S, int V) { return K < 1 || S < 1 || V < 1 || V > CFZ_MAX_NBR + 1 ? fail("K, S must be positive and V in 1..CFZ_MAX_NBR+1") : 0; }
int traj_fits(int K, int S, int V) { return (size_t)K * S * V * 7 > ((size_t)1 << 31) ? fail("trajectory too large") : 0; }

// what both score entry points refuse before they look at the handle
int score_args(double near, const double *val, const int32_t *cnt) {
  if (!(near >= 0.0) || !std::isfinite(near)) return fail("near must be finite and not negative");
  if (!val || !cnt) return fail("null val or cnt");
  return 0;
}

// The columns of a pool on the device (conflict_columns, from the arena) and what a kernel over pair_columns is launched with.
struct PairLaunch { double *cols; size_t lds; double il0, il1; };  // lds: bytes of dynamic LDS, 0: not staged
int pair_launch(cfz_handle *h, int P, int V, int T, const double *d_tables, PairLaunch &pl) {
  const long n = (long)P * V * T;
  pl = {nullptr, T <= cfz::kConflictLdsT ? (size_t)T * 64 : 0, cfz::audit_body_il(h->ks.g, 0), cfz::audit_body_il(h->ks.g, 1)};
  ARENA_ALLOC(h->arena, pl.cols, (size_t)n * 4 * 8);
  hipLaunchKernelGGL(conflict_columns, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, n, T, d_tables, pl.cols);
  HIP_OK(hipGetLastError());
  return 0;
}

// the conflict map of P plan sets x V vehicles x T samples (V > 1) that lie on the device (conflict_kernel), left on the device:
// dc[P][npair][2D+1] as keys, di[P][npair][2D+1][3], from the arena, which the caller has reset.  Nothing is waited for.
int conflict_device(cfz_handle *h, int P, int V, int T, const double *d_tables, int D, double margin, double *&dc, int32_t *&di) {
  static_assert(cfz::kConflictNInfo == CFZ_CONFLICT_NINFO, "cfz_conflict.inl and confrez_hip.h disagree");
  const int npair = V * (V - 1) / 2;
  const size_t no = (size_t)P * npair * (2 * (size_t)D + 1);
  PairLaunch pl;
  if (pair_launch(h, P, V, T, d_tables, pl)) return -1;
  ARENA_ALLOC(h->arena, dc, no * 8); ARENA_ALLOC(h->arena, di, no * CFZ_CONFLICT_NINFO * 4);
  hipLaunchKernelGGL(conflict_kernel, dim3((unsigned)(P * npair)), dim3(256), pl.lds, h->stream, h->kargs, V, T, D, pl.lds != 0, pl.cols, pl.il0,
                     pl.il1, margin, margin * margin, dc, di);
  HIP_OK(hipGetLastError());
  return 0;
}

// the same map into the caller's host arrays clear, info (either NULL: not wanted), clear as signed distances.  The arena is reset by
// the caller.
int conflict_launch(cfz_handle *h, int P, int V, int T, const double *d_tables, int D, double margin, double *clear, int32_t *info) {
  const int npair = V * (V - 1) / 2;
  if (npair == 0) return 0;
  const size_t no = (size_t)P * npair * (2 * (size_t)D + 1);
  double *dc = nullptr;
  int32_t *di = nullptr;
  if (conflict_device(h, P, V, T, d_tables, D, margin, dc, di)) return -1;
  if (clear) HIP_OK(hipMemcpyAsync(clear, dc, no * 8, hipMemcpyDeviceToHost, h->stream));
  if (info) HIP_OK(hipMemcpyAsync(info, di, no * CFZ_CONFLICT_NINFO * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  if (clear)
    for (size_t i = 0; i < no; ++i) clear[i] = cfz::audit_key_distance(clear[i]);
  return 0;
}

// What the plan-set entry points refuse of a margin and of a pool tables[P][V][T][7]; separate: they refuse other things in between.
int margin_arg(double margin) { return !(margin >= 0.0) || !std::isfinite(margin) ? fail("margin must be finite and not negative") : 0; }
int pool_dims(int P, int V, int T) {
  return P < 1 || T < 1 ? fail("P, T must be positive") : V < 1 || V > CFZ_MAX_NBR + 1 ? fail("V must be in 1..CFZ_MAX_NBR+1") : 0;
}
int pool_tables(const double *tables) { return tables ? 0 : fail("null tables"); }
int pool_fits(int P, int V, int T) { return (size_t)P * V * T * 7 > ((size_t)1 << 31) ? fail("pool of plan sets too large") : 0; }

// what both conflict entry points refuse before they look at the handle
int conflict_args(int D, double margin) { return D < 0 ? fail("D must not be negative") : margin_arg(margin); }

// the sizes of a conflict map
int conflict_sizes(int P, int V, int T, int D) {
  if (pool_fits(P, V, T)) return -1;
  return (size_t)P * (V * (V - 1) / 2) * (2 * (size_t)D + 1) * CFZ_CONFLICT_NINFO > ((size_t)1 << 31) ? fail("conflict map too large") : 0;
}

// a caller's pool of plan sets tables[P][V][T][7] with the map asked of it (cfz_plan_conflicts, cfz_plan_delays): what both refuse first,
// in this order, and its upload once the call has got as far as the device
int plan_pool_args(int P, int V, int T, const double *tables, int D, double margin) {
  return conflict_args(D, margin) || pool_dims(P, V, T) || pool_tables(tables) || conflict_sizes(P, V, T, D) ? -1 : 0;
}
int plan_pool_upload(cfz_handle *h, int P, int V, int T, const double *tables, double *&d_tables) {
  HIP_OK(hipSetDevice(h->device));
  if (arena_reset(h->arena)) return -1;
  return arena_upload(h, d_tables, tables, (size_t)P * V * T * 7);
}

// what the three delay entry points refuse before they look at the handle: the slack, the outputs, the box of the search and the caps
// cap[P][V] (NULL: D for every vehicle)
int delay_args(int P, int V, int D, int slack, const int32_t *cap, const int32_t *delays) {
  static_assert(cfz::kDelayNInfo == CFZ_DELAY_NINFO && cfz::kDelayMaxV == CFZ_MAX_NBR + 1, "cfz_delay.inl and confrez_hip.h disagree");
  if (slack < 0) return fail("slack must not be negative");
  if (!delays) return fail("null delays");
  double box = 1.0;
  for (int v = 0; v < V; ++v) box *= D + 1.0;
  if (box > 2147483648.0) return fail("search space too large: (D+1)^V must not exceed 2^31");
  if (cap)
    for (size_t i = 0; i < (size_t)P * V; ++i)
      if (cap[i] < 0 || cap[i] > D) return fail("a cap lies outside [0, D]");
  return 0;
}

// the answer of a set without pairs (V = 1): found, delay 0; rclear +inf where a map of clearances is given
void delay_single(int P, bool with_clear, int32_t *delays, int32_t *info, double *rclear) {
  for (int p = 0; p < P; ++p) {
    delays[p] = 0;
    if (info) { info[3 * p] = 1; info[3 * p + 1] = info[3 * p + 2] = 0; }
    if (with_clear && rclear) rclear[p] = INFINITY;
  }
}

// A kernel's block of small outputs rows[P][no] ints read back on the handle's stream, and slices of every row copied into the caller's
// arrays: ints [at, at + n) of row p to dst + p n ints; a dst that is NULL is not wanted.  Ends synchronised.
struct RowSlice { void *dst; int at, n; };
int read_rows(cfz_handle *h, const int32_t *d_rows, int P, int no, std::initializer_list<RowSlice> slices) {
  std::vector<int32_t> rows((size_t)P * no);
  HIP_OK(hipMemcpyAsync(rows.data(), d_rows, rows.size() * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  for (const RowSlice &s : slices)
    for (int p = 0; s.dst && p < P; ++p) memcpy((int32_t *)s.dst + (size_t)p * s.n, rows.data() + (size_t)p * no + s.at, (size_t)s.n * 4);
  return 0;
}

// delay_kernel over a map on the device (V > 1): d_count with entries cs ints apart, d_clear or NULL (keys: the caller's rclear is
// converted to a signed distance as conflict_launch converts the map), cap the caller's host array or NULL; the outputs are the caller's
// host arrays (info, rclear may be NULL).  The arena is reset by the caller.  Ends synchronised.
int delay_launch(cfz_handle *h, int P, int V, int D, const int32_t *d_count, int cs, const double *d_clear, bool keys, int slack,
                 const int32_t *cap, int32_t *delays, int32_t *info, double *rclear) {
  const int npair = V * (V - 1) / 2, no = delay_out_ints(V);
  int32_t *dcap = nullptr, *dout = nullptr;
  ARENA_ALLOC(h->arena, dout, (size_t)P * no * 4);
  if (cap && arena_upload(h, dcap, cap, (size_t)P * V)) return -1;
  hipLaunchKernelGGL(delay_kernel, dim3((unsigned)P), dim3(256), (size_t)npair * cfz::delay_words(D) * 4, h->stream, V, D, slack, d_count, cs,
                     d_clear, dcap, dout);
  HIP_OK(hipGetLastError());
  if (!d_clear) rclear = nullptr;  // (written only where a map of clearances is given)
  if (read_rows(h, dout, P, no, {{delays, 0, V}, {info, V, CFZ_DELAY_NINFO}, {rclear, no - 2, 2}})) return -1;  // (rclear: a double as two ints)
  for (int p = 0; rclear && keys && p < P; ++p) rclear[p] = cfz::audit_key_distance(rclear[p]);
  return 0;
}

// the conflict map of a pool on the device, searched there: what cfz_plan_delays and cfz_loop_plan_delays share
int plan_delays_launch(cfz_handle *h, int P, int V, int T, const double *d_tables, int D, double margin, int slack, const int32_t *cap,
                       int32_t *delays, int32_t *info, double *rclear) {
  double *dc = nullptr;
  int32_t *di = nullptr;
  if (conflict_device(h, P, V, T, d_tables, D, margin, dc, di)) return -1;
  return delay_launch(h, P, V, D, di + 2, CFZ_CONFLICT_NINFO, dc, true, slack, cap, delays, info, rclear);
}

// what the coordination and the schedule entry points refuse, after the margin, of a pool's sizes and its lengths length[P][V] (NULL: T)
int coord_args(int P, int V, int T, const int32_t *length) {
  static_assert(cfz::kScheduleMaxT == CFZ_SCHEDULE_MAX_T && cfz::kScheduleMaxH == CFZ_SCHEDULE_MAX_H && cfz::kScheduleNInfo == CFZ_SCHEDULE_NINFO &&
                    cfz::kScheduleMaxV == CFZ_MAX_NBR + 1, "cfz_schedule.inl and confrez_hip.h disagree");
  if (pool_dims(P, V, T) || pool_fits(P, V, T)) return -1;
  if ((size_t)P * (V * (V - 1) / 2) * 2 * T * cfz::coord_words(T) > ((size_t)1 << 31)) return fail("coordination diagram too large");
  if (length)
    for (size_t i = 0; i < (size_t)P * V; ++i)
      if (length[i] < 1 || length[i] > T) return fail("a length lies outside [1, T]");
  return 0;
}

// what both schedule entry points refuse next: the horizon, the slack, the orders orders[O][V], the hold mask and the outputs
int schedule_args(int P, int V, int T, const uint8_t *hold, int H, int slack, int O, const int32_t *orders, const int32_t *schedule) {
  if (H < 1 || O < 1) return fail("H, O must be positive");
  if (T > CFZ_SCHEDULE_MAX_T) return fail("T must not exceed CFZ_SCHEDULE_MAX_T");
  if (H > CFZ_SCHEDULE_MAX_H) return fail("H must not exceed CFZ_SCHEDULE_MAX_H");
  if (H < T) return fail("H must not be below T");
  if (slack < 0) return fail("slack must not be negative");
  if (!hold) return fail("null hold");
  if (!orders) return fail("null orders");
  if (!schedule) return fail("null schedule");
  for (int o = 0; o < O; ++o)
    if (!cfz::schedule_is_permutation(V, orders + (size_t)o * V)) return fail("an order is not a permutation of the vehicles");
  if ((size_t)P * V * H > ((size_t)1 << 31)) return fail("schedule too large");
  if ((size_t)P * 4 * cfz::schedule_wave_words(V, T, H) > ((size_t)1 << 29)) return fail("schedule workspace too large");
  return 0;
}

// the coordination diagrams of P plan sets x V vehicles x T samples (V > 1) that lie on the device (coord_kernel), left on the device:
// diag[P][npair][2][T][words], from the arena, which the caller has reset.  length: the caller's host array or NULL; dlen its copy on
// the device.  Nothing is waited for.
int coord_device(cfz_handle *h, int P, int V, int T, const double *d_tables, const int32_t *length, double margin, uint32_t *&diag,
                 int32_t *&dlen) {
  const int npair = V * (V - 1) / 2;
  dlen = nullptr;
  PairLaunch pl;
  if (pair_launch(h, P, V, T, d_tables, pl)) return -1;
  ARENA_ALLOC(h->arena, diag, (size_t)P * npair * 2 * T * cfz::coord_words(T) * 4);
  if (length && arena_upload(h, dlen, length, (size_t)P * V)) return -1;
  hipLaunchKernelGGL(coord_kernel, dim3((unsigned)(P * npair), (unsigned)((T + kCoordRows - 1) / kCoordRows)), dim3(256), pl.lds, h->stream,
                     h->kargs, V, T, pl.lds != 0, pl.cols, dlen, pl.il0, pl.il1, margin, margin * margin, diag);
  HIP_OK(hipGetLastError());
  return 0;
}

// side 0 of the diagrams of a pool on the device into the caller's blocked[P][npair][T][words]: what cfz_plan_coordination returns.  The
// arena is reset by the caller.  Ends synchronised.
int coord_launch(cfz_handle *h, int P, int V, int T, const double *d_tables, const int32_t *length, double margin, uint32_t *blocked) {
  uint32_t *diag = nullptr;
  int32_t *dlen = nullptr;
  if (coord_device(h, P, V, T, d_tables, length, margin, diag, dlen)) return -1;
  const size_t row = (size_t)T * cfz::coord_words(T) * 4;
  HIP_OK(hipMemcpy2DAsync(blocked, row, diag, 2 * row, row, (size_t)P * (V * (V - 1) / 2), hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

// the answer of a set of one vehicle: nothing to avoid, it drives through; every order of the list is feasible and the first one wins
void schedule_single(int P, int T, const int32_t *length, int H, int O, int32_t *schedule, int32_t *arrival, int32_t *waits, int32_t *info) {
  for (int p = 0; p < P; ++p) {
    const int g = (length ? length[p] : T) - 1;
    for (int t = 0; t < H; ++t) schedule[(size_t)p * H + t] = t < g ? t : g;
    if (arrival) arrival[p] = g;
    if (waits) waits[p] = 0;
    if (info) { int32_t *o = info + (size_t)p * CFZ_SCHEDULE_NINFO; o[0] = 1; o[1] = 0; o[2] = g; o[3] = g; o[4] = O; }
  }
}

// the diagrams of a pool on the device, searched there by schedule_kernel (V > 1): what cfz_plan_schedule and cfz_loop_plan_schedule
// share.  length, hold, orders and the outputs are the caller's host arrays (arrival, waits, info may be NULL).  The arena is reset by the
// caller.  Ends synchronised.
int schedule_launch(cfz_handle *h, int P, int V, int T, const double *d_tables, const int32_t *length, const uint8_t *hold, int H, double margin,
                    int slack, int O, const int32_t *orders, int32_t *schedule, int32_t *arrival, int32_t *waits, int32_t *info) {
  uint32_t *diag = nullptr, *dord = nullptr, *ws = nullptr;
  int32_t *dlen = nullptr, *dsched = nullptr, *dsmall = nullptr;
  uint8_t *dhold = nullptr;
  if (coord_device(h, P, V, T, d_tables, length, margin, diag, dlen)) return -1;
  std::vector<uint32_t> packed((size_t)O);
  for (int o = 0; o < O; ++o) packed[o] = cfz::schedule_pack(V, orders + (size_t)o * V);
  const int no = schedule_out_ints(V);
  const size_t per = cfz::schedule_wave_words(V, T, H), lds = 4 * per * 4;
  const int in_lds = lds <= (size_t)cfz::kScheduleLdsBytes;
  if (arena_upload(h, dhold, hold, (size_t)P * V * T) || arena_upload(h, dord, packed.data(), packed.size())) return -1;
  ARENA_ALLOC(h->arena, dsched, (size_t)P * V * H * 4); ARENA_ALLOC(h->arena, dsmall, (size_t)P * no * 4);
  if (!in_lds) ARENA_ALLOC(h->arena, ws, (size_t)P * 4 * per * 4);
  if (in_lds)  // (beyond 64 KB of dynamic LDS a kernel has to be told)
    HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(schedule_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, cfz::kScheduleLdsBytes));
  hipLaunchKernelGGL(schedule_kernel, dim3((unsigned)P), dim3(256), in_lds ? lds : 0, h->stream, V, T, H, slack, O, dord, diag, dlen, dhold, in_lds,
                     ws, dsched, dsmall);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(schedule, dsched, (size_t)P * V * H * 4, hipMemcpyDeviceToHost, h->stream));
  return read_rows(h, dsmall, P, no, {{arrival, 0, V}, {waits, V, V}, {info, 2 * V, CFZ_SCHEDULE_NINFO}});  // (packed lives until it has synchronised)
}

// What the pool kernels take, composed from the two per-scenario settings: one KArgs block per (problem, map) pair that some scenario
// uses, in the order of first use, and the block of every scenario.  probs[P], problem_of[S] as cfz_loop_set_problems fills them (probs
// NULL: the handle's problem for every scenario); map_tab[M][n_obs][20] (device), map_of[S] as cfz_loop_set_maps does (map_tab NULL: the
// handle's map).  A block is its problem's {sp, dv, L} with sp.obs_tab pointing at its map's table; dv and L do not depend on the
// obstacles, and the obstacle arrays inside sp stay the handle's (no loop kernel reads them).  The blocks are device allocations of
// their own, handed back in out (both settings off: none): the caller swaps them in (pool_swap) once its call can no longer fail.
struct PoolBufs { DevBuf<KArgs> pool; DevBuf<int32_t> of; };
int compose_pool(const cfz_handle *h, const std::vector<KArgs> *probs, const int32_t *problem_of, const double *map_tab, const int32_t *map_of,
                 PoolBufs &out) {
  out = PoolBufs();
  if (!probs && !map_tab) return 0;
  const int S = h->lp.S;
  const size_t tab = (size_t)std::max(h->ks.n_obs, 1) * 20;
  const KArgs own = {h->ks, cfz::derive(h->ks), h->lay};  // (what cfz_create wrote to h->kargs)
  std::vector<KArgs> blocks;
  std::vector<int32_t> block_of((size_t)S);
  std::map<std::pair<int, int>, int> seen;
  for (int s = 0; s < S; ++s) {
    const std::pair<int, int> key(probs ? problem_of[s] : 0, map_tab ? map_of[s] : 0);
    auto it = seen.find(key);
    if (it == seen.end()) {
      KArgs b = probs ? (*probs)[key.first] : own;
      b.sp.obs_tab = map_tab ? map_tab + (size_t)key.second * tab : h->obs_tab;
      it = seen.emplace(key, (int)blocks.size()).first;
      blocks.push_back(b);
    }
    block_of[s] = it->second;
  }
  if (out.pool.alloc(blocks.size()) || out.of.alloc((size_t)S)) return -1;
  HIP_OK(hipMemcpy(out.pool, blocks.data(), blocks.size() * sizeof(KArgs), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(out.of, block_of.data(), (size_t)S * 4, hipMemcpyHostToDevice));
  return 0;
}

void pool_swap(cfz_handle *h, PoolBufs &p) { h->lp.pb_pool = std::move(p.pool); h->lp.pb_of = std::move(p.of); }
}  // namespace

extern "C" {

int cfz_loop_init_tables(cfz_handle *h, int S, int P, int T, const double *tables, const int32_t *table_of, const int32_t *k0,
                         const double *noise) {
  if (!h) return fail("null handle");
  const int V = h->ks.n_nbr + 1, N = h->ks.N;
  if (S < 1 || (long)S * V > h->max_batch) return fail("S * (n_nbr+1) exceeds max_batch");
  if (T < 1 || !tables || !k0) return fail("bad reference table");
  if (P < 1) return fail("the pool needs at least one plan set (P >= 1)");
  if (!table_of && P != S) return fail("table_of is NULL (scenario s follows set s), which needs P == S");
  if ((size_t)P * V * T * 7 > ((size_t)1 << 31)) return fail("pool of plan sets too large");
  std::vector<int32_t> tof((size_t)S);
  for (int s = 0; s < S; ++s) {
    tof[s] = table_of ? table_of[s] : s;
    if (tof[s] < 0 || tof[s] >= P) return fail("table_of[s] outside [0, P)");
  }
  HIP_OK(hipSetDevice(h->device));
  loop_release(h);  // record, exchange order, disturbance and comm setting included: back to the undisturbed, lossless Jacobi loop at step 0
  cfz_handle::Loop lp;  // the new loop, the handle's once it is seeded
  lp.S = S; lp.T = T; lp.P = P;
  const size_t B = (size_t)S * V;
  if (lp.ref_table.alloc((size_t)P * V * T * 7) || lp.pred.alloc(B * 7 * N) || lp.state.alloc(B * 5)) return -1;
  if (lp.kidx.alloc((size_t)S) || lp.order.alloc(B) || lp.table_of.alloc((size_t)S)) return -1;
  if (lp.dz_zero.alloc((size_t)cfz::kDisturbN + S + ((size_t)S + 1) / 2)) return -1;  // zero sigma[12] | zero level[S] | zero stream[S]
  HIP_OK(hipMemset(lp.dz_zero, 0, lp.dz_zero.size() * 8));
  HIP_OK(hipMemset(h->wst, 0, (size_t)h->max_batch * h->wst_stride * 8));  // first iteration: cold multipliers
  HIP_OK(hipMemcpy(lp.ref_table, tables, (size_t)P * V * T * 7 * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(lp.table_of, tof.data(), (size_t)S * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(lp.kidx, k0, (size_t)S * 4, hipMemcpyHostToDevice));
  double *dn = nullptr;
  if (noise) { if (arena_reset(h->arena)) return -1; ARENA_ALLOC(h->arena, dn, B * 5 * 8); HIP_OK(hipMemcpy(dn, noise, B * 5 * 8, hipMemcpyHostToDevice)); }
  const long nt = (long)B * N;
  hipLaunchKernelGGL(loop_seed, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, h->stream, S, V, N, T, lp.ref_table,
                     lp.table_of, lp.kidx, dn, lp.pred, lp.state);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(h->stream));
  h->lp = std::move(lp);
  return 0;
}

int cfz_loop_init(cfz_handle *h, int S, int T, const double *ref_table, const int32_t *k0, const double *noise) {
  if (!h) return fail("null handle");
  if (S < 1 || (long)S * (h->ks.n_nbr + 1) > h->max_batch) return fail("S * (n_nbr+1) exceeds max_batch");
  const std::vector<int32_t> zero((size_t)S, 0);  // one plan set, followed by every scenario
  return cfz_loop_init_tables(h, S, 1, T, ref_table, zero.data(), k0, noise);
}

int cfz_loop_record(cfz_handle *h, int K) {
  if (loop_ready(h, true)) return -1;
  if (K < 0) return fail("K must not be negative");
  const size_t B = (size_t)h->lp.S * (h->ks.n_nbr + 1);
  if ((size_t)K * B * 7 > ((size_t)1 << 31)) return fail("record too large");
  DevBuf<double> rec;
  DevBuf<int32_t> rec_si;
  if (rec.alloc((size_t)K * B * 7) || rec_si.alloc((size_t)K * 2 * B)) return -1;  // (K = 0: none)
  h->lp.rec = std::move(rec); h->lp.rec_si = std::move(rec_si);
  h->lp.rec_cap = K; h->lp.rec_used = 0;
  return 0;
}

int cfz_loop_history(cfz_handle *h, int t0, int K, double *traj, int32_t *status, int32_t *iters) {
  if (record_window(h, t0, K)) return -1;
  const size_t B = (size_t)h->lp.S * (h->ks.n_nbr + 1);
  if (traj) HIP_OK(hipMemcpy(traj, h->lp.rec + (size_t)t0 * B * 7, (size_t)K * B * 7 * 8, hipMemcpyDeviceToHost));
  if (status || iters) {
    std::vector<int32_t> si((size_t)K * 2 * B);
    HIP_OK(hipMemcpy(si.data(), h->lp.rec_si + (size_t)t0 * 2 * B, si.size() * 4, hipMemcpyDeviceToHost));
    for (int k = 0; k < K; ++k) {
      if (status) memcpy(status + (size_t)k * B, si.data() + (size_t)k * 2 * B, B * 4);
      if (iters) memcpy(iters + (size_t)k * B, si.data() + ((size_t)k * 2 + 1) * B, B * 4);
    }
  }
  return 0;
}

int cfz_loop_audit(cfz_handle *h, int t0, int K, double pos_tol, double psi_tol, double v_tol, double *clear, int32_t *where,
                   int32_t *first_contact, int32_t *arrive) {
  if (record_window(h, t0, K)) return -1;
  const int S = h->lp.S, V = h->ks.n_nbr + 1;
  const size_t B = (size_t)S * V;
  if (arena_reset(h->arena)) return -1;
  double *dg = nullptr;
  ARENA_ALLOC(h->arena, dg, B * 3 * 8);
  hipLaunchKernelGGL(loop_goals, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream, S, V, h->lp.T, h->lp.ref_table, h->lp.table_of, dg);
  HIP_OK(hipGetLastError());
  // every scenario against its own map under the mapping in force now (cfz_loop_set_maps)
  return audit_launch(h, K, S, V, h->lp.rec + (size_t)t0 * B * 7, dg, h->lp.mp_on ? h->lp.mp_poly : nullptr, h->lp.mp_on ? h->lp.mp_of : nullptr,
                      pos_tol, psi_tol, v_tol, clear, where, first_contact, arrive);
}

int cfz_audit(cfz_handle *h, int K, int S, int V, const double *traj, const double *goal, double pos_tol, double psi_tol, double v_tol,
              double *clear, int32_t *where, int32_t *first_contact, int32_t *arrive) {
  return cfz_audit_maps(h, K, S, V, traj, goal, 0, nullptr, nullptr, nullptr, pos_tol, psi_tol, v_tol, clear, where, first_contact, arrive);
}

int cfz_audit_maps(cfz_handle *h, int K, int S, int V, const double *traj, const double *goal, int M, const double *A_obs,
                   const double *b_obs, const int32_t *map_of, double pos_tol, double psi_tol, double v_tol, double *clear, int32_t *where,
                   int32_t *first_contact, int32_t *arrive) {
  if (!h) return fail("null handle");
  if (traj_dims(K, S, V)) return -1;
  if (!traj || !goal) return fail("null trajectory or goal");
  if (traj_fits(K, S, V)) return -1;
  if (M < 0) return fail("M must not be negative");
  const bool maps = M > 0 && A_obs;  // else: the handle's map for every scenario
  const int no = h->ks.n_obs;
  std::vector<cfz::AuditPoly> poly;
  if (maps) {
    if (!b_obs || !map_of) return fail("null b_obs or map_of");
    for (int s = 0; s < S; ++s)
      if (map_of[s] < 0 || map_of[s] >= M) return fail("map_of[s] outside [0, M)");
    poly.resize(std::max((size_t)M * no, (size_t)1));
    for (int m = 0; m < M; ++m) {
      double Vx[CFZ_MAX_OBS][4][2];
      if (map_vertices(no, A_obs + (size_t)m * no * 8, b_obs + (size_t)m * no * 4, Vx)) { cfz_g_err = "map " + std::to_string(m) + ": " + cfz_g_err; return -1; }
      audit_polys(no, Vx, poly.data() + (size_t)m * no);
    }
  }
  HIP_OK(hipSetDevice(h->device));
  if (arena_reset(h->arena)) return -1;
  double *dt_ = nullptr, *dg = nullptr;
  cfz::AuditPoly *dpoly = nullptr;
  int32_t *dof = nullptr;
  if (arena_upload(h, dt_, traj, (size_t)K * S * V * 7) || arena_upload(h, dg, goal, (size_t)S * V * 3)) return -1;
  if (maps && (arena_upload(h, dpoly, poly.data(), poly.size()) || arena_upload(h, dof, map_of, (size_t)S))) return -1;
  return audit_launch(h, K, S, V, dt_, dg, dpoly, dof, pos_tol, psi_tol, v_tol, clear, where, first_contact, arrive);  // (ends synchronised: `poly` outlives its copy)
}

int cfz_loop_score(cfz_handle *h, int t0, int K, double pos_tol, double psi_tol, double v_tol, double near, double *val, int32_t *cnt) {
  if (score_args(near, val, cnt)) return -1;
  if (record_window(h, t0, K)) return -1;
  const int S = h->lp.S, V = h->ks.n_nbr + 1;
  const size_t B = (size_t)S * V;
  if (arena_reset(h->arena)) return -1;
  // the clock stands rec_used - t0 steps after the state before step t0 (every recorded step advanced it by one)
  const int32_t *si = h->lp.rec_si + (size_t)t0 * 2 * B;
  return score_launch(h, K, S, V, h->lp.rec + (size_t)t0 * B * 7, si, si + B, (long)(2 * B), h->lp.T, h->lp.ref_table, h->lp.table_of, h->lp.kidx,
                      h->lp.rec_used - t0, pos_tol, psi_tol, v_tol, near, val, cnt);
}

int cfz_score(cfz_handle *h, int K, int S, int V, const double *traj, const int32_t *status, const int32_t *iters, int P, int T,
              const double *tables, const int32_t *table_of, const int32_t *k0, double pos_tol, double psi_tol, double v_tol, double near,
              double *val, int32_t *cnt) {
  if (score_args(near, val, cnt)) return -1;
  if (traj_dims(K, S, V)) return -1;
  if (P < 1 || T < 1) return fail("P, T must be positive");
  if (!traj || !tables || !table_of || !k0) return fail("null trajectory, tables, table_of or k0");
  if (traj_fits(K, S, V)) return -1;
  if ((size_t)P * V * T * 7 > ((size_t)1 << 31)) return fail("pool of plan sets too large");
  for (int s = 0; s < S; ++s) {
    if (table_of[s] < 0 || table_of[s] >= P) return fail("table_of[s] outside [0, P)");
    if (k0[s] < 0) return fail("k0[s] must not be negative");
  }
  if (!h) return fail("null handle");
  HIP_OK(hipSetDevice(h->device));
  if (arena_reset(h->arena)) return -1;
  const size_t B = (size_t)S * V;
  double *dt_ = nullptr, *dp = nullptr;
  int32_t *dof = nullptr, *dk = nullptr, *dst = nullptr, *dit = nullptr;
  if (arena_upload(h, dt_, traj, (size_t)K * B * 7) || arena_upload(h, dp, tables, (size_t)P * V * T * 7)) return -1;
  if (arena_upload(h, dof, table_of, (size_t)S) || arena_upload(h, dk, k0, (size_t)S)) return -1;
  if (status && arena_upload(h, dst, status, (size_t)K * B)) return -1;
  if (iters && arena_upload(h, dit, iters, (size_t)K * B)) return -1;
  return score_launch(h, K, S, V, dt_, dst, dit, (long)B, T, dp, dof, dk, 0, pos_tol, psi_tol, v_tol, near, val, cnt);  // (ends synchronised)
}

int cfz_plan_conflicts(cfz_handle *h, int P, int V, int T, const double *tables, int D, double margin, double *clear, int32_t *info) {
  if (plan_pool_args(P, V, T, tables, D, margin)) return -1;
  if (!h) return fail("null handle");
  if (V == 1) return 0;  // no pairs: nothing to launch, nothing to write
  double *dt_ = nullptr;
  if (plan_pool_upload(h, P, V, T, tables, dt_)) return -1;
  return conflict_launch(h, P, V, T, dt_, D, margin, clear, info);  // (ends synchronised)
}

int cfz_loop_plan_conflicts(cfz_handle *h, int D, double margin, double *clear, int32_t *info) {
  if (conflict_args(D, margin)) return -1;
  if (loop_ready(h)) return -1;
  const int V = h->ks.n_nbr + 1;
  if (conflict_sizes(h->lp.P, V, h->lp.T, D)) return -1;
  if (arena_reset(h->arena)) return -1;
  return conflict_launch(h, h->lp.P, V, h->lp.T, h->lp.ref_table, D, margin, clear, info);
}

int cfz_delay_search(cfz_handle *h, int P, int V, int D, const int32_t *count, const double *clear, int slack, const int32_t *cap,
                     int32_t *delays, int32_t *info, double *rclear) {
  if (P < 1 || V < 1) return fail("P, V must be positive");
  if (V > CFZ_MAX_NBR + 1) return fail("V must be in 1..CFZ_MAX_NBR+1");
  if (D < 0) return fail("D must not be negative");
  if (!count) return fail("null count");
  if (delay_args(P, V, D, slack, cap, delays)) return -1;
  const size_t no = (size_t)P * (V * (V - 1) / 2) * (2 * (size_t)D + 1);
  if (no > ((size_t)1 << 31)) return fail("conflict map too large");
  if (!h) return fail("null handle");
  if (V == 1) { delay_single(P, clear != nullptr, delays, info, rclear); return 0; }  // no pairs: nothing to launch
  HIP_OK(hipSetDevice(h->device));
  if (arena_reset(h->arena)) return -1;
  int32_t *dn = nullptr;
  double *dc = nullptr;
  if (arena_upload(h, dn, count, no) || (clear && arena_upload(h, dc, clear, no))) return -1;
  return delay_launch(h, P, V, D, dn, 1, dc, false, slack, cap, delays, info, rclear);  // (ends synchronised)
}

int cfz_plan_delays(cfz_handle *h, int P, int V, int T, const double *tables, int D, double margin, int slack, const int32_t *cap,
                    int32_t *delays, int32_t *info, double *rclear) {
  if (plan_pool_args(P, V, T, tables, D, margin)) return -1;
  if (delay_args(P, V, D, slack, cap, delays)) return -1;
  if (!h) return fail("null handle");
  if (V == 1) { delay_single(P, true, delays, info, rclear); return 0; }
  double *dt_ = nullptr;
  if (plan_pool_upload(h, P, V, T, tables, dt_)) return -1;
  return plan_delays_launch(h, P, V, T, dt_, D, margin, slack, cap, delays, info, rclear);  // (ends synchronised)
}

int cfz_loop_plan_delays(cfz_handle *h, int D, double margin, int slack, const int32_t *cap, int32_t *delays, int32_t *info, double *rclear) {
  if (conflict_args(D, margin)) return -1;
  if (slack < 0) return fail("slack must not be negative");
  if (loop_ready(h)) return -1;  // (the caps, the box and the outputs are P x V, the pool's: checked below)
  const int V = h->ks.n_nbr + 1;
  if (conflict_sizes(h->lp.P, V, h->lp.T, D)) return -1;
  if (delay_args(h->lp.P, V, D, slack, cap, delays)) return -1;
  if (V == 1) { delay_single(h->lp.P, true, delays, info, rclear); return 0; }
  if (arena_reset(h->arena)) return -1;
  return plan_delays_launch(h, h->lp.P, V, h->lp.T, h->lp.ref_table, D, margin, slack, cap, delays, info, rclear);
}

int cfz_plan_coordination(cfz_handle *h, int P, int V, int T, const double *tables, const int32_t *length, double margin, uint32_t *blocked) {
  if (margin_arg(margin) || coord_args(P, V, T, length) || pool_tables(tables)) return -1;
  if (!blocked) return fail("null blocked");
  if (!h) return fail("null handle");
  if (V == 1) return 0;  // no pairs: nothing to launch, nothing to write
  double *dt_ = nullptr;
  if (plan_pool_upload(h, P, V, T, tables, dt_)) return -1;
  return coord_launch(h, P, V, T, dt_, length, margin, blocked);  // (ends synchronised)
}

int cfz_plan_schedule(cfz_handle *h, int P, int V, int T, const double *tables, const int32_t *length, const uint8_t *hold, int H, double margin,
                      int slack, int O, const int32_t *orders, int32_t *schedule, int32_t *arrival, int32_t *waits, int32_t *info) {
  if (margin_arg(margin) || coord_args(P, V, T, length) || pool_tables(tables)) return -1;
  if (schedule_args(P, V, T, hold, H, slack, O, orders, schedule)) return -1;
  if (!h) return fail("null handle");
  if (V == 1) { schedule_single(P, T, length, H, O, schedule, arrival, waits, info); return 0; }  // no pairs: nothing to launch
  double *dt_ = nullptr;
  if (plan_pool_upload(h, P, V, T, tables, dt_)) return -1;
  return schedule_launch(h, P, V, T, dt_, length, hold, H, margin, slack, O, orders, schedule, arrival, waits, info);  // (ends synchronised)
}

int cfz_loop_plan_schedule(cfz_handle *h, const int32_t *length, const uint8_t *hold, int H, double margin, int slack, int O,
                           const int32_t *orders, int32_t *schedule, int32_t *arrival, int32_t *waits, int32_t *info) {
  if (margin_arg(margin)) return -1;
  if (slack < 0) return fail("slack must not be negative");
  if (loop_ready(h)) return -1;  // (the lengths, the mask, the orders and the outputs have the pool's sizes: checked below)
  const int P = h->lp.P, V = h->ks.n_nbr + 1, T = h->lp.T;
  if (coord_args(P, V, T, length)) return -1;
  if (schedule_args(P, V, T, hold, H, slack, O, orders, schedule)) return -1;
  if (V == 1) { schedule_single(P, T, length, H, O, schedule, arrival, waits, info); return 0; }
  if (arena_reset(h->arena)) return -1;
  return schedule_launch(h, P, V, T, h->lp.ref_table, length, hold, H, margin, slack, O, orders, schedule, arrival, waits, info);
}

int cfz_loop_set_order(cfz_handle *h, const int32_t *order) {
  if (loop_ready(h, true)) return -1;
  if (!order) { h->lp.xperm.reset(); h->lp.xrank.reset(); h->lp.xlist.reset(); h->lp.xperm_host.clear(); return 0; }
  const int S = h->lp.S, V = h->ks.n_nbr + 1;
  std::vector<int32_t> rank((size_t)S * V), list((size_t)V * S);
  for (int s = 0; s < S; ++s) {
    std::vector<char> seen((size_t)V, 0);
    for (int r = 0; r < V; ++r) {
      const int32_t v = order[(size_t)s * V + r];
      if (v < 0 || v >= V || seen[v]) return fail("order[s] is not a permutation of 0..V-1");
      seen[v] = 1;
      rank[(size_t)s * V + v] = r; list[(size_t)r * S + s] = s * V + v;
    }
  }
  DevBuf<int32_t> xperm, xrank, xlist;
  if (xperm.alloc((size_t)S * V) || xrank.alloc((size_t)S * V) || xlist.alloc((size_t)S * V)) return -1;
  HIP_OK(hipMemcpy(xperm, order, (size_t)S * V * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(xrank, rank.data(), (size_t)S * V * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(xlist, list.data(), (size_t)S * V * 4, hipMemcpyHostToDevice));
  std::vector<int32_t> host(order, order + (size_t)S * V);
  h->lp.xperm = std::move(xperm); h->lp.xrank = std::move(xrank); h->lp.xlist = std::move(xlist);
  h->lp.xperm_host.swap(host);
  return 0;
}

int cfz_loop_set_disturbance(cfz_handle *h, uint64_t seed, const double sigma_meas[5], const double sigma_act[2],
                             const double sigma_proc[5], const double *level, const uint32_t *stream) {
  if (loop_ready(h, true)) return -1;
  if (!sigma_meas && !sigma_act && !sigma_proc) { h->lp.dz_on = false; return 0; }  // off: the plain kernels
  const int S = h->lp.S;
  std::vector<double> f((size_t)cfz::kDisturbN + S, 0.0);
  for (int i = 0; i < 5; ++i) { if (sigma_meas) f[i] = sigma_meas[i]; if (sigma_proc) f[7 + i] = sigma_proc[i]; }
  for (int i = 0; i < 2; ++i) if (sigma_act) f[5 + i] = sigma_act[i];
  for (int i = 0; i < cfz::kDisturbN; ++i)
    if (!(f[i] >= 0.0) || !std::isfinite(f[i])) return fail("a sigma is negative or not finite");
  for (int s = 0; s < S; ++s) {
    f[cfz::kDisturbN + s] = level ? level[s] : 1.0;
    if (!(f[cfz::kDisturbN + s] >= 0.0) || !std::isfinite(f[cfz::kDisturbN + s])) return fail("a level is negative or not finite");
  }
  DevBuf<double> buf;
  if (upload_setting(h, buf, f, stream)) return -1;
  h->lp.dz_buf = std::move(buf); h->lp.dz_seed = seed; h->lp.dz_on = true;
  return 0;
}

int cfz_loop_disturbance(cfz_handle *h, int t0, int K, double *d) {
  if (loop_ready(h)) return -1;
  if (!h->lp.dz_on) return fail("no disturbance is set (cfz_loop_set_disturbance)");
  if (t0 < 0 || K < 1 || !d) return fail("t0 must not be negative, K must be positive and d not NULL");
  const int S = h->lp.S, V = h->ks.n_nbr + 1;
  const size_t n = (size_t)K * S * V * cfz::kDisturbN;
  if (n > ((size_t)1 << 31)) return fail("window too large");
  if (arena_reset(h->arena)) return -1;
  double *dd = nullptr;
  ARENA_ALLOC(h->arena, dd, n * 8);
  hipLaunchKernelGGL(disturb_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, disturb_args(h), S, V, t0, (long)n, dd);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(d, dd, n * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int cfz_loop_set_comm(cfz_handle *h, uint64_t seed, const double *p_drop, int max_age, int compensate, const uint32_t *stream) {
  if (loop_ready(h, true)) return -1;
  if (!p_drop) { h->lp.cm_on = false; return 0; }  // off: the kernels without it
  if (max_age < 1 || max_age > CFZ_MAX_AGE) return fail("max_age outside 1..CFZ_MAX_AGE");
  if (compensate != 0 && compensate != 1) return fail("compensate must be 0 or 1");
  const int S = h->lp.S, V = h->ks.n_nbr + 1, N = h->ks.N;
  for (int s = 0; s < S; ++s)
    if (!(p_drop[s] >= 0.0 && p_drop[s] <= 1.0)) return fail("a p_drop is outside [0, 1] or not finite");
  const size_t slot = (size_t)S * V * 7 * N;
  DevBuf<double> ring, buf;
  if (ring.alloc((size_t)(max_age + 2) * slot)) return -1;
  if (upload_setting(h, buf, std::vector<double>(p_drop, p_drop + S), stream)) return -1;  // p_drop[S] | stream[S]
  // history restarts at the message standing in pred, that of the last iteration done
  const int tau_on = h->lp.steps_done - 1;
  HIP_OK(hipMemcpy(ring + (size_t)cfz::comm_slot(tau_on, max_age) * slot, h->lp.pred, slot * 8, hipMemcpyDeviceToDevice));
  h->lp.cm_ring = std::move(ring); h->lp.cm_buf = std::move(buf);
  h->lp.cm_seed = seed; h->lp.cm_max_age = max_age; h->lp.cm_compensate = compensate; h->lp.cm_tau_on = tau_on; h->lp.cm_on = true;
  return 0;
}

int cfz_problem_check(const cfz_spec *base, const cfz_options *base_opt, const cfz_spec *spec, const cfz_options *opt) {
  if (!base || !spec) return fail("null argument");
  cfz_options bd;
  if (!base_opt) { cfz_default_options(&bd); base_opt = &bd; }
  if (!opt) opt = base_opt;
  if (spec_shape_ok(spec) || options_ok(opt)) return -1;
  // geometry and time base are the handle's: the plant, the audit, the layout and the carry records are built from them
  if (spec->N != base->N) return fail("problem differs from the handle in N");
  if (spec->n_obs != base->n_obs) return fail("problem differs from the handle in n_obs");
  if (spec->n_nbr != base->n_nbr) return fail("problem differs from the handle in n_nbr");
  if (spec->rk_substeps != base->rk_substeps) return fail("problem differs from the handle in rk_substeps");
  if (spec->dt != base->dt) return fail("problem differs from the handle in dt");
  if (spec->wb != base->wb) return fail("problem differs from the handle in wb");
  if (memcmp(spec->g, base->g, sizeof spec->g)) return fail("problem differs from the handle in g");
  for (int j = 0; j < spec->n_obs; ++j) {
    if (memcmp(spec->A_obs[j], base->A_obs[j], sizeof spec->A_obs[j])) return fail(("problem differs from the handle in A_obs[" + std::to_string(j) + "]").c_str());
    if (memcmp(spec->b_obs[j], base->b_obs[j], sizeof spec->b_obs[j])) return fail(("problem differs from the handle in b_obs[" + std::to_string(j) + "]").c_str());
  }
  if ((opt->carry_duals != 0) != (base_opt->carry_duals != 0)) return fail("problem differs from the handle in carry_duals");
  static const char *const box[6] = {"x", "y", "v", "delta", "a", "w"};
  for (int i = 0; i < 6; ++i)
    if (!(spec->bounds[2 * i] <= spec->bounds[2 * i + 1]) || !std::isfinite(spec->bounds[2 * i]) || !std::isfinite(spec->bounds[2 * i + 1]))
      return fail((std::string("bounds: the box of ") + box[i] + " has lo > hi or is not finite").c_str());
  cfz::KSpec k;
  return fill_kspec(k, spec, opt);
}

int cfz_loop_set_problems(cfz_handle *h, int P, const cfz_spec *specs, const cfz_options *opts, const int32_t *problem_of) {
  if (loop_ready(h, true)) return -1;
  if (P < 0) return fail("P must not be negative");
  const bool off = P == 0 || !specs;  // off: the kernels without it (the map pool's, if one is set)
  const int S = h->lp.S;
  std::vector<KArgs> pool;
  std::vector<int32_t> pool_of;
  if (!off) {
    if (!problem_of) return fail("null problem_of");
    for (int s = 0; s < S; ++s)
      if (problem_of[s] < 0 || problem_of[s] >= P) return fail("problem_of[s] outside [0, P)");
    pool.resize((size_t)P);
    pool_of.assign(problem_of, problem_of + S);
    for (int p = 0; p < P; ++p) {
      const cfz_options *o = opts ? &opts[p] : &h->opt0;
      if (cfz_problem_check(&h->spec0, &h->opt0, &specs[p], o)) { cfz_g_err = "problem " + std::to_string(p) + ": " + cfz_g_err; return -1; }
      if (fill_kspec(pool[p].sp, &specs[p], o)) return -1;
      pool[p].sp.obs_tab = h->obs_tab;
      pool[p].dv = cfz::derive(pool[p].sp); pool[p].L = h->lay;
    }
  }
  // the new setting, composed with the map pool in force, is written into blocks of its own and swapped in once it is complete: a
  // failure leaves the one in force as it was
  PoolBufs d;
  if (compose_pool(h, off ? nullptr : &pool, pool_of.data(), h->lp.mp_on ? h->lp.mp_tab.get() : nullptr, h->lp.mp_user_of.data(), d)) return -1;
  pool_swap(h, d);
  h->lp.pb_user.swap(pool); h->lp.pb_user_of.swap(pool_of);
  h->lp.pb_on = !off;
  return 0;
}

int cfz_map_check(const cfz_spec *base, const double *A_obs, const double *b_obs) {
  if (!base) return fail("null argument");
  if (spec_shape_ok(base)) return -1;
  if (base->n_obs > 0 && (!A_obs || !b_obs)) return fail("null A_obs or b_obs");
  double V[CFZ_MAX_OBS][4][2];
  return map_vertices(base->n_obs, A_obs, b_obs, V);
}

int cfz_loop_set_maps(cfz_handle *h, int M, const double *A_obs, const double *b_obs, const int32_t *map_of) {
  if (loop_ready(h, true)) return -1;
  if (M < 0) return fail("M must not be negative");
  const int S = h->lp.S, no = h->ks.n_obs;
  const std::vector<KArgs> *probs = h->lp.pb_on ? &h->lp.pb_user : nullptr;
  PoolBufs d;
  if (M == 0 || !A_obs) {  // off: the kernels without it (the problem pool's, if one is set)
    if (compose_pool(h, probs, h->lp.pb_user_of.data(), nullptr, nullptr, d)) return -1;
    pool_swap(h, d);
    h->lp.mp_tab.reset(); h->lp.mp_poly.reset(); h->lp.mp_of.reset();
    h->lp.mp_user_of.clear(); h->lp.mp_on = false; h->lp.mp_M = 0;
    return 0;
  }
  if (!b_obs || !map_of) return fail("null b_obs or map_of");
  for (int s = 0; s < S; ++s)
    if (map_of[s] < 0 || map_of[s] >= M) return fail("map_of[s] outside [0, M)");
  const size_t stride = (size_t)std::max(no, 1) * 20;
  std::vector<double> tab((size_t)M * stride, 0.0);
  std::vector<cfz::AuditPoly> poly(std::max((size_t)M * no, (size_t)1));
  for (int m = 0; m < M; ++m) {
    const double *A = A_obs + (size_t)m * no * 8, *b = b_obs + (size_t)m * no * 4;
    double V[CFZ_MAX_OBS][4][2];
    if (map_vertices(no, A, b, V)) { cfz_g_err = "map " + std::to_string(m) + ": " + cfz_g_err; return -1; }
    for (int j = 0; j < no; ++j)
      obs_tab_entry(tab.data() + (size_t)m * stride + (size_t)j * 20, reinterpret_cast<const double(*)[2]>(A + (size_t)j * 8), b + (size_t)j * 4, V[j]);
    audit_polys(no, V, poly.data() + (size_t)m * no);
  }
  // as in cfz_loop_set_problems: blocks of its own, swapped in once the new setting is complete
  DevBuf<double> dtab;
  DevBuf<cfz::AuditPoly> dpoly;
  DevBuf<int32_t> dof;
  if (dtab.alloc(tab.size()) || dpoly.alloc(poly.size()) || dof.alloc((size_t)S)) return -1;
  HIP_OK(hipMemcpy(dtab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dpoly, poly.data(), poly.size() * sizeof(cfz::AuditPoly), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dof, map_of, (size_t)S * 4, hipMemcpyHostToDevice));
  if (compose_pool(h, probs, h->lp.pb_user_of.data(), dtab, map_of, d)) return -1;
  std::vector<int32_t> of_host(map_of, map_of + S);
  pool_swap(h, d);
  h->lp.mp_tab = std::move(dtab); h->lp.mp_poly = std::move(dpoly); h->lp.mp_of = std::move(dof); h->lp.mp_M = M;
  h->lp.mp_user_of.swap(of_host);
  h->lp.mp_on = true;
  return 0;
}

int cfz_loop_comm(cfz_handle *h, int tau0, int K, int32_t *delivered) {
  if (loop_ready(h)) return -1;
  if (!h->lp.cm_on) return fail("no lossy exchange is set (cfz_loop_set_comm)");
  if (tau0 < 0 || K < 1 || !delivered) return fail("tau0 must not be negative, K must be positive and delivered not NULL");
  const int S = h->lp.S, V = h->ks.n_nbr + 1;
  const size_t n = (size_t)K * S * V * V;
  if (n > ((size_t)1 << 31)) return fail("window too large");
  if (arena_reset(h->arena)) return -1;
  int32_t *dd = nullptr;
  ARENA_ALLOC(h->arena, dd, n * 4);
  hipLaunchKernelGGL(comm_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, comm_args(h), S, V, tau0, (long)n, dd);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(delivered, dd, n * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

int cfz_loop_step(cfz_handle *h) {
  if (loop_ready(h) || record_room(h, 1)) return -1;
  const int V = h->ks.n_nbr + 1, S = h->lp.S, B = S * V;
  float total_ms = 0.f;
  if (h->lp.xperm) {
    // sequential exchange: V rounds; round r prepares, solves (S instances, dispatch list xlist[r]) and posts the vehicle of rank r
    // of every scenario.  The solve time is the sum of the V launches: launch_solve records ev0 / ev1 anew, so each round's pair is
    // read before the next round is queued.
    for (int r = 0; r < V; ++r) {
      if (r > 0) {
        HIP_OK(hipEventSynchronize(h->ev1));
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, h->ev0, h->ev1)); total_ms += ms;
      }
      if (loop_round(h, r, S, h->lp.xlist + (size_t)r * S, h->lp.xperm, h->lp.xrank)) return -1;
    }
    h->lp.have_order = false;  // the LPT list is the Jacobi steps' own
  } else {
    if (loop_round(h, 0, B, h->lp.have_order ? h->lp.order : nullptr, nullptr, nullptr)) return -1;
    hipLaunchKernelGGL(order_by_iters, dim3(1), dim3(1024), 0, h->stream, B, h->iters, h->lp.order);
    HIP_OK(hipGetLastError());
    h->lp.have_order = true;
  }
  if (h->lp.rec) h->lp.rec_used += 1;
  h->lp.steps_done += 1;
  HIP_OK(hipStreamSynchronize(h->stream));
  float ms = 0.f;
  HIP_OK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->last_ms = total_ms + ms;
  h->ms_pending = false;
  return 0;
}

int cfz_loop_run(cfz_handle *h, int K) {
  if (loop_ready(h)) return -1;
  if (K < 1) return fail("K must be positive");
  if (record_room(h, K)) return -1;
  const int V = h->ks.n_nbr + 1, N = h->ks.N, S = h->lp.S, B = S * V;
  const size_t total = (size_t)B * K;
  if (total > (size_t)1 << 30) return fail("too many work items");
  int ncu = 0;
  HIP_OK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, h->device));
  int per_cu = 0;
  const bool seq = h->lp.xperm != nullptr, comm = h->lp.cm_on;
  const int variant = loop_variant(seq, h->lp.dz_on, comm, h->lp.pb_on, h->lp.mp_on);
  if (variant < 0) return fail("no persistent kernel for this setting");
  const LoopVariant &var = kLoopVariants[variant];
  HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, var.fn, cfz::kNL, h->lds_bytes));
  per_cu = std::min(per_cu, h->blocks_per_cu);  // the 2 KiB LDS granules (cfz_create): what the hardware really keeps resident
  if (per_cu < 1) return fail("loop kernel does not fit on a CU");
  // one workgroup per resident slot: more would only queue behind them (any workgroup can serve any item, so a surplus
  // is harmless, just useless)
  if (const char *cap = std::getenv("CFZ_LOOP_BLOCKS_PER_CU")) per_cu = std::max(1, std::min(per_cu, std::atoi(cap)));  // experiments
  // the sequential exchange has at most S items in flight (one per scenario): workgroups beyond S would never win one and
  // would end the launch through the idle give-up
  const int grid = std::min(seq ? S : B, per_cu * ncu);
  const size_t per_block = 5 + 3 * (size_t)N + (size_t)h->ks.n_nbr * 3 * N + 7 * (size_t)N;
  const size_t qwords = 2 * (size_t)K + total;  // [head K][tail K][slots K x B]
  if (h->lp.pred2.reserve((size_t)2 * B * 7 * N) || h->lp.ctrl.reserve(4 + 1024) || h->lp.done.reserve((size_t)S) || h->lp.iter_sum.reserve(8)) return -1;
  if (h->lp.scratch.reserve((size_t)grid * per_block) || h->lp.queue.reserve(qwords)) return -1;
  // parity 0 of the double buffer <- current predictions (the ring of messages already holds them); queue <- all items of iteration 0
  if (!comm) HIP_OK(hipMemcpyAsync(h->lp.pred2, h->lp.pred, (size_t)B * 7 * N * 8, hipMemcpyDeviceToDevice, h->stream));
  HIP_OK(hipMemsetAsync(h->lp.queue, 0, 2 * (size_t)K * 4, h->stream));
  HIP_OK(hipMemsetAsync(h->lp.queue + 2 * K, 0xff, total * 4, h->stream));
  {
    // Jacobi: all B items; sequential: the S items (s, xperm[s][0])
    const int n0 = seq ? S : B;
    std::vector<int32_t> first(n0);
    for (int i = 0; i < n0; ++i) first[i] = seq ? i * V + h->lp.xperm_host[(size_t)i * V] : i;
    HIP_OK(hipMemcpyAsync(h->lp.queue + 2 * K, first.data(), (size_t)n0 * 4, hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipMemcpyAsync(h->lp.queue + K, &n0, 4, hipMemcpyHostToDevice, h->stream));  // tail[0]
    const int32_t ctrl0[4] = {0, 0, 0, 0};
    HIP_OK(hipMemcpyAsync(h->lp.ctrl, ctrl0, sizeof ctrl0, hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipMemsetAsync(h->lp.done, 0, (size_t)S * 4, h->stream));
    HIP_OK(hipMemsetAsync(h->lp.iter_sum, 0, 32, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));  // `first` and `ctrl0` are host temporaries
  }
  HIP_OK(hipEventRecord(h->ev0, h->stream));
  double *rec; int32_t *rec_si;
  record_slice(h, rec, rec_si);
  // Issue priority for the items on the launch's critical path (cfz_loop_body.inl).  CFZ_LOOP_PRIO_LAG: an item of iteration t
  // qualifies while t <= lowest open iteration + lag (negative: no item is ever prioritised).  CFZ_LOOP_PRIO_TAIL: from iteration 1 on
  // it must also hold one of the last `tail` positions of its iteration's queue (0: the iteration alone decides; unset: the built-in
  // setting, kLoopPrioTailDiv).  Overrides for experiments, read at every call; the results do not depend on either.
  const int prio_lag = std::getenv("CFZ_LOOP_PRIO_LAG") ? std::atoi(std::getenv("CFZ_LOOP_PRIO_LAG")) : kLoopPrioLag;
  const int prio_tail = std::getenv("CFZ_LOOP_PRIO_TAIL") ? std::max(0, std::atoi(std::getenv("CFZ_LOOP_PRIO_TAIL")))
                                                          : (kLoopPrioTailDiv > 0 ? std::max(V, B / kLoopPrioTailDiv) : 0);
#ifdef CFZ_LOOP_TRACE
  {
    static DevBuf<long long> trace_dev;
    if (trace_dev.size() < total * kLoopTraceWords) {
      if (trace_dev.reserve(total * kLoopTraceWords)) return -1;
      long long *const p = trace_dev;
      HIP_OK(hipMemcpyToSymbol(HIP_SYMBOL(cfz_loop_trace_buf), &p, sizeof p));
    }
    HIP_OK(hipMemsetAsync(trace_dev, 0, total * kLoopTraceWords * 8, h->stream));
    g_loop_trace_dev = trace_dev; g_loop_trace_items = total; g_loop_trace_grid = grid;
  }
#endif
  // The ten kernels share their arguments up to the record; what follows is the tail groups of the settings a kernel was compiled
  // with, in this order.  One line per row of kLoopVariants, in its order; `launch` refuses a line that names another kernel than its row.
  const auto xo = std::make_tuple((const int32_t *)h->lp.xperm, (const int32_t *)h->lp.xrank);
  const auto dz = std::make_tuple(disturb_args(h, true), h->lp.steps_done);  // (dz, step0)
  const auto cm = std::make_tuple(comm_args(h));
  const auto pb = std::make_tuple((const KArgs *)h->lp.pb_pool, (const int32_t *)h->lp.pb_of, h->lp.dz_on ? 1 : 0);  // (pool, problem_of, clip)
  auto launch = [&](auto kernel, const auto &...groups) {
    if ((const void *)kernel != var.fn) return fail("cfz_loop_run: the launch chain and kLoopVariants name different kernels");
    std::apply([&](auto... tail) {
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(cfz::kNL), h->lds_bytes, h->stream, h->kargs, S, V, K, h->lp.T, h->lp.ref_table, h->lp.table_of,
                         h->lp.kidx, 0, h->lp.pred2, h->lp.state, h->lp.scratch, h->lp.queue, h->lp.ctrl, h->lp.done, h->status, h->iters, h->stats,
                         h->lp.iter_sum, h->carry_duals ? h->wst : nullptr, h->wst_stride, prio_lag, prio_tail, rec, rec_si, tail...);
    }, std::tuple_cat(groups...));
    return 0;
  };
  int bad = 0;
  switch (variant) {
    case 0: bad = launch(loop_kernel); break;
    case 1: bad = launch(loop_kernel_seq, xo); break;
    case 2: bad = launch(loop_kernel_dist, dz); break;
    case 3: bad = launch(loop_kernel_seq_dist, xo, dz); break;
    case 4: bad = launch(loop_kernel_comm, dz, cm); break;
    case 5: bad = launch(loop_kernel_seq_comm, xo, dz, cm); break;
    case 6: bad = launch(loop_kernel_pool, dz, pb); break;
    case 7: bad = launch(loop_kernel_seq_pool, xo, dz, pb); break;
    case 8: bad = launch(loop_kernel_pool_comm, dz, cm, pb); break;
    case 9: bad = launch(loop_kernel_seq_pool_comm, xo, dz, cm, pb); break;
  }
  if (bad) return -1;
  HIP_OK(hipGetLastError());
  if (h->lp.rec) h->lp.rec_used += K;
  h->lp.steps_done += K;
  HIP_OK(hipEventRecord(h->ev1, h->stream));
  // predictions after K iterations live in parity K%2 (comm: in the newest message's slot); advance the scenario clocks by K
  HIP_OK(hipMemcpyAsync(h->lp.pred, comm ? comm_message(h, h->lp.steps_done - 1) : h->lp.pred2 + (size_t)(K & 1) * B * 7 * N, (size_t)B * 7 * N * 8, hipMemcpyDeviceToDevice, h->stream));
  hipLaunchKernelGGL(advance_clock, dim3((S + 255) / 256), dim3(256), 0, h->stream, S, K, h->lp.kidx);
  HIP_OK(hipGetLastError());
  if (const char *dbg = std::getenv("CFZ_LOOP_WATCHDOG")) {
    // diagnostic: watch the queue counters from a second stream while the kernel runs; stop it if it stalls
    const double limit_s = std::atof(dbg) > 0 ? std::atof(dbg) : 10.0;
    hipStream_t s2; HIP_OK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
    int32_t last_head = -1; double stalled = 0.0;
    while (hipEventQuery(h->ev1) == hipErrorNotReady) {
      usleep(100000);
      int32_t c[4] = {0, 0, 0, 0};
      HIP_OK(hipMemcpyAsync(c, h->lp.ctrl, sizeof c, hipMemcpyDeviceToHost, s2)); HIP_OK(hipStreamSynchronize(s2));
      std::fprintf(stderr, "[cfz watchdog] lowest open iteration %d, completed %d of %zu, err %d (grid %d)", c[0], c[1], total, c[2], grid);
#ifdef CFZ_LOOP_TRACE
      int32_t mk[8];
      HIP_OK(hipMemcpyAsync(mk, h->lp.ctrl + 4, sizeof mk, hipMemcpyDeviceToHost, s2)); HIP_OK(hipStreamSynchronize(s2));
      for (int i = 0; i < 8 && i < grid; ++i) std::fprintf(stderr, " m%d=%d", i, mk[i]);
#endif
      std::fprintf(stderr, "\n");
      stalled = (c[1] == last_head) ? stalled + 0.1 : 0.0; last_head = c[1];
      if (stalled > limit_s) {
        const int32_t one = 1;
        HIP_OK(hipMemcpyAsync(h->lp.ctrl + 2, &one, 4, hipMemcpyHostToDevice, s2)); HIP_OK(hipStreamSynchronize(s2));
        stalled = -1e9;
      }
    }
    (void)hipStreamDestroy(s2);
  }
  HIP_OK(hipStreamSynchronize(h->stream));
  HIP_OK(hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1));
  h->ms_pending = false;
  int32_t ctrl[4] = {0, 0, 0, 0}, isum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  HIP_OK(hipMemcpy(ctrl, h->lp.ctrl, sizeof ctrl, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(isum, h->lp.iter_sum, 32, hipMemcpyDeviceToHost));
  h->last_iter_sum = isum[0]; h->last_converged = isum[1];
  for (int i = 0; i < 6; ++i) h->last_status[i] = isum[2 + i];
  h->lp.have_order = false;
  if (ctrl[2]) return fail("persistent loop kernel timed out waiting for a work item");
  return 0;
}

#ifdef CFZ_LOOP_TRACE
// diagnostic build only: the trace of the last cfz_loop_run, out[K * B][kLoopTraceWords] in item order (t, b); returns the grid of
// that launch (the resident workgroups), -1 when n is not K * B
extern "C" int cfz_loop_trace_read(long long *out, long n) {
  if (!out || !g_loop_trace_dev || (size_t)n != g_loop_trace_items) return fail("cfz_loop_trace_read: no trace of that many items");
  HIP_OK(hipMemcpy(out, g_loop_trace_dev, g_loop_trace_items * kLoopTraceWords * 8, hipMemcpyDeviceToHost));
  return g_loop_trace_grid;
}
#endif

long cfz_loop_last_iterations(const cfz_handle *h) { return h ? h->last_iter_sum : -1; }
long cfz_loop_last_converged(const cfz_handle *h) { return h ? h->last_converged : -1; }
int cfz_loop_last_status_counts(const cfz_handle *h, long counts[6]) {
  if (!h || !counts) return fail("null argument");
  for (int i = 0; i < 6; ++i) counts[i] = h->last_status[i];
  return 0;
}

int cfz_loop_get(cfz_handle *h, double *state, double *pred, int32_t *status, int32_t *iters) {
  if (loop_ready(h)) return -1;
  const size_t B = (size_t)h->lp.S * (h->ks.n_nbr + 1), N = h->ks.N;
  if (state) HIP_OK(hipMemcpy(state, h->lp.state, B * 5 * 8, hipMemcpyDeviceToHost));
  if (pred) HIP_OK(hipMemcpy(pred, h->lp.pred, B * 7 * N * 8, hipMemcpyDeviceToHost));
  if (status) HIP_OK(hipMemcpy(status, h->status, B * 4, hipMemcpyDeviceToHost));
  if (iters) HIP_OK(hipMemcpy(iters, h->iters, B * 4, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
