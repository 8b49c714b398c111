/* confrez_hip.h -- C ABI of libconfrez_hip.so, the MI355X (gfx950) engine behind the
 * collision-free planning hot path of XuShenLZ/conflict_rez.
 *
 * The reference has no FFI: its seam is the CasADi call `opti.solve()` inside
 * `VehicleFollower.step` (confrez/control/vehicle_follower.py:428-563).  Every entry point
 * below names the reference statements it stands in for.  All arrays are contiguous fp64
 * (int32 where stated), instance-major: the leading index is the problem instance
 * b in [0, B).  Host-pointer calls copy in/out during the call and retain nothing;
 * `_device` calls take HIP device pointers and enqueue on the handle's stream.
 *
 * Return value: 0 on success, <0 on an API error (cfz_last_error() explains).  Solver
 * outcomes are per instance, in `status`:
 *   0 converged | 1 iteration limit | 2 line search failed | 3 non-finite iterate |
 *   4 measured state already violates a collision row (NLP infeasible, nothing iterated) |
 *   5 constraint violation stalled above constr_viol_tol (locally infeasible; IPOPT: restoration failed)
 * The reference turns any non-zero outcome into a Python exception that `step()` catches
 * to apply its shift fallback (vehicle_follower.py:478-524); the Python shim does the same.
 *
 * A handle is not thread-safe (the reference is single-threaded).
 */
#ifndef CONFREZ_HIP_H
#define CONFREZ_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFZ_MAX_OBS 8   /* static obstacles (reference: 6, compute_sets.py:259-330) */
#define CFZ_MAX_NBR 7   /* neighbouring vehicles (reference: 3) */
#define CFZ_MAX_N 32    /* horizon stages (reference: 30, vehicle_follower.py:146); four lanes of a 128-lane workgroup per stage */

/* Constants of the MPC-step NLP: what `setup_controller(dt, N, dmin)` bakes into the CasADi
 * graph (vehicle_follower.py:146-368). */
typedef struct cfz_spec {
  int32_t N;           /* horizon stages                       :146 */
  int32_t n_obs;       /* static obstacles, 4 half-planes each :152-156 */
  int32_t n_nbr;       /* other vehicles                       :303 */
  int32_t rk_substeps; /* RK4 sub-steps M of dynamic_model.py:30 (reference 4) */
  double dt;           /*                                      :146 */
  double wb;           /* wheelbase, vehicle_types.py:19 */
  double dmin;         /* clearance                            :146 */
  double g[4];         /* body rectangle lf, w/2, lr, w/2 (rows +x,+y,-x,-y), vehicle_types.py:65-71 */
  double bounds[12];   /* lo,hi of x, y, v, delta, a, w        :204-240 */
  double weights[6];   /* (x-xr)^2,(y-yr)^2,(psi-psir)^2,a^2,(v w)^2,delta^2   :263-271 */
  double A_obs[CFZ_MAX_OBS][4][2]; /* unit outward normals     :280-290 */
  double b_obs[CFZ_MAX_OBS][4];
} cfz_spec;

/* Stopping rule and interior-point constants: `opti.solver("ipopt", p_opts, s_opts)`
 * (vehicle_follower.py:356-368) plus the IPOPT defaults that call leaves untouched. */
typedef struct cfz_options {
  int32_t max_iter;       /* :364 600 */
  int32_t max_backtrack;  /* line-search halvings before status 2 */
  int32_t filter_cap;     /* filter entries kept per barrier problem */
  int32_t stall_iters;    /* 10: iterations without progress of the constraint violation (those that changed the working set
                           *     of the separation rows count a quarter) before status 5; 0 = off */
  int32_t row_curvature;  /* 1: Hessian = Gauss-Newton objective part + multiplier-weighted curvature of the separation rows */
  int32_t carry_duals;    /* 1: keep one carry record per slot (multipliers of the last converged solve); 0: never */
  int32_t vv_rows;        /* 1: a block whose closest features are two vertices is constrained by their Euclidean distance
                           *    (exactly the reference's OBCA rows there); 0: face-normal certificates only (a restriction) */
  int32_t shift_after;    /* 60: from this iteration on a stage whose row curvature the convexity safeguard would scale keeps it
                           *     whole and is shifted by the smallest multiple of the identity instead (a scaled model can
                           *     cycle for hundreds of iterations on a vehicle pressed into a corner); 0 = never */
  int32_t restoration;    /* 2: restoration phases a solve may go through (IPOPT's answer to a failed line search, paper sec. 3.3):
                           *    Levenberg-Marquardt on the squared violations of the separation rows and the boxes, on the solver's own
                           *    stage recursion, until the worst violation is a tenth of what it was; then cold multipliers at the
                           *    restored point.  Entered after a failed line search at an iterate whose violation exceeds
                           *    constr_viol_tol, and before the first iteration of a start that resto_first describes.  A restoration
                           *    that does not reach its goal ends the solve with status 5 (IPOPT: "converged to a point of local
                           *    infeasibility").  0 = none: a failed line search is status 2 */
  int32_t shift_stagnation; /* 10: once the scaled optimality error has not halved for this many iterations at a feasible iterate
                           *    (violation <= constr_viol_tol) the late curvature shift may start at iteration 40 instead of waiting for
                           *    shift_after; ends the sawtooth of the scaled model 15-20 iterations sooner; 0 = off */
  int32_t err_stall_iters; /* 150: a solve whose scaled optimality error has not halved for this many iterations ends with status 5
                           *    instead of running to max_iter (limit cycles below constr_viol_tol escape stall_iters' test); 0 = off */
  int32_t carry_shift;    /* 1: a converged solve in which some stage's row curvature had to be shifted tells the next solve of the same
                           *    carry slot (cfz_mpc_set_carry / the closed loop) to shift from its first iteration instead of waiting for
                           *    shift_after / shift_stagnation: a cornered vehicle otherwise repeats the 40+ iterations of the scaled
                           *    model at every MPC iteration.  Solves without carried multipliers are unaffected.  0 = off */
  double tol;             /* :362 1e-2 */
  double constr_viol_tol; /* :363 1e-2 */
  double dual_inf_tol;    /* IPOPT default 1 */
  double compl_inf_tol;   /* IPOPT default 1e-4 */
  double mu_init /* 1e-3 (IPOPT: 0.1) */, kappa_eps, kappa_mu, theta_mu, tau_min, bound_push, bound_frac, s_max, kappa_sigma;
  double eta_phi, gamma_theta, gamma_phi, delta_sw, s_theta, s_phi, reg_primal;
  double stall_kappa;     /* 0.9: progress = violation below stall_kappa x its last checkpoint */
  double warm_push;       /* 1e-6: distance from a bound kept by a start that carries multipliers */
  double reg_dual_rows;   /* 1e-8: IPOPT's dual regularisation delta_c (paper sec. 3.1), permanently on the separation rows: two rows of
                           *    a block, or rows of different blocks of a stage, become dependent at a contact and their multipliers
                           *    run away along the null space; 0 = off */
  double resto_first;     /* 0.3 (metres): a start whose separation rows of stages >= 1 are violated by more than this -- the warm
                           *    start of a vehicle whose neighbour's prediction has moved into its path -- goes through the restoration
                           *    phase before the first iteration; 0 = never */
} cfz_options;

typedef struct cfz_handle cfz_handle;

void cfz_default_spec(cfz_spec *spec);       /* reference constants, no obstacles */
void cfz_default_options(cfz_options *opt);  /* reference s_opts + IPOPT defaults */

/* Builds the solver for one NLP structure on `device` for up to `max_batch` instances.
 * Replaces the graph construction half of setup_controller (:165-368). */
int cfz_create(const cfz_spec *spec, const cfz_options *opt, int device, int max_batch, cfz_handle **out);
int cfz_destroy(cfz_handle *h);
int cfz_max_batch(const cfz_handle *h);
/* LDS bytes one instance (= one wavefront) occupies and how many instances the runtime keeps resident per CU. */
int cfz_kernel_info(const cfz_handle *h, int32_t *lds_bytes_per_instance, int32_t *instances_per_cu);

/* opti.set_value(current_x..current_delta, current_ref_*, p_other_pred[*]) (:432-456).
 * x0[B][5]; ref[B][3][N] rows x,y,psi; nbr[B][n_nbr][3][N] (already advanced by the caller
 * as `_adv_onestep` does, :445-455). */
int cfz_mpc_set_params(cfz_handle *h, int B, const double *x0, const double *ref, const double *nbr);

/* opti.set_initial(x..w) (:466-473).  zu[B][7][N] rows x,y,psi,v,delta,a,w.  The dual
 * initial guesses of :458-464,:475-476 are not taken: the engine eliminates the OBCA duals
 * and rebuilds them from the poses (DESIGN.md "Certificate elimination"). */
int cfz_mpc_set_warm(cfz_handle *h, int B, const double *zu);

/* Multipliers from the previous MPC iteration (IPOPT: warm_start_init_point; the reference hands the previous
 * duals to opti.set_initial at :458-464, :475-476).  carry[b] != 0 declares that the next cfz_mpc_solve of slot b
 * is the MPC iteration following the one last solved in slot b (horizon moved on by one stage): if that solve
 * converged, the interior-point iteration starts from its slack and bound multipliers, costates and barrier
 * parameter, shifted by one stage, instead of z = 1, nu = 0, mu = mu_init.  The flags hold for one solve; NULL or
 * no call = cold.  The closed loop (cfz_loop_*) always carries.  Typically 1.8 instead of 4.2 iterations. */
int cfz_mpc_set_carry(cfz_handle *h, int B, const int32_t *carry);

/* The same flags as a HIP device array int32[B] (e.g. `status == 0` of the previous iteration, computed on the device):
 * nothing is copied or synchronised; the array is read by the next solve's kernel and must stay valid until it ends. */
int cfz_mpc_set_carry_device(cfz_handle *h, int B, const int32_t *d_carry);

/* Which carry record each instance of the next solve reads and refreshes: slots[b] in [0, max_batch).  Default (no
 * call, or NULL): instance b uses record b.  Lets several callers share one handle without mixing their multipliers:
 * the reference's `for v in vehicles: v.step()` loop (:642-647) and the ROS nodes (vehicle_node.py:150-152) step ONE
 * vehicle at a time, so each vehicle solves a batch of one in its own slot.  Holds for one solve, like the flags.
 * The slots of one call must be pairwise distinct (two instances on one record would race on it): duplicates are an API error. */
int cfz_mpc_set_slots(cfz_handle *h, int B, const int32_t *slots);

/* sol = opti.solve() (:479): runs the batched solver and blocks until done. */
int cfz_mpc_solve(cfz_handle *h, int B);

/* sol.value(...) (:484-500).  Any output pointer may be NULL.
 * zu[B][7][N]; l,m [B][N][4*n_obs]; lam_ij,lam_ji [B][n_nbr][N][4]; s [B][n_nbr][N][2]. */
int cfz_mpc_get(cfz_handle *h, int B, double *zu, double *l, double *m, double *lam_ij, double *lam_ji, double *s);

/* sol.stats() (:481): per-instance outcome.  Any pointer may be NULL.
 * status,iters int32[B]; cost, kkt_err (scaled optimality error E_0), min_sep fp64[B].
 * status: 0 converged (IPOPT Solve_Succeeded); 1 iteration limit; 2 line search failed; 3 non-finite iterate;
 *         4 measured state infeasible: it violates a collision row, or a box on x, y, v, delta, by more than constr_viol_tol
 *           (stage 0 is pinned to the measurement: no iterations; the rows of stage 0 take no part in the iteration otherwise);
 *         5 locally infeasible: the constraint violation stalled above constr_viol_tol, the scaled optimality error stalled
 *           (err_stall_iters), or a restoration phase did not reach its goal (IPOPT: "converged to a point of local infeasibility").
 *         Every status != 0 is what
 *         the reference sees as an exception from opti.solve() and answers with the shift fallback (:501-524). */
int cfz_mpc_stats(cfz_handle *h, int B, int32_t *status, int32_t *iters, double *cost, double *kkt_err,
                  double *min_sep);

/* Milliseconds the last cfz_mpc_solve / cfz_loop_step spent in its solver kernel (HIP events
 * on the handle's stream); after a sequential cfz_loop_step (cfz_loop_set_order) the sum of its V solve launches. */
double cfz_last_solve_ms(const cfz_handle *h);

/* ---- device-resident path ------------------------------------------------------------- */
/* Same as set_params + set_warm + solve + get(zu) on HIP device pointers, asynchronous on
 * `stream` (a hipStream_t; NULL = the handle's own stream).  d_status/d_iters int32[B],
 * d_stats fp64[B][3] = cost, kkt_err, min_sep.  d_zu is read as the warm start and overwritten
 * with the solution. */
int cfz_mpc_solve_device(cfz_handle *h, int B, const double *d_x0, const double *d_ref, const double *d_nbr,
                         double *d_zu, int32_t *d_status, int32_t *d_iters, double *d_stats, void *stream);

/* ---- vehicle-sharded closed loop (SURVEY.md 8e partitioning B; the reference's ROS deployment runs one process per vehicle
 * and exchanges predictions as messages, ros2_ws/src/confrez_ros/src/vehicle_node.py:111-189) --------------------------------
 * One MPC iteration of the n_own vehicles this rank owns in S scenarios, entirely on `stream` (NULL = the handle's), no host
 * synchronisation: parameters + shifted warm start from the gathered predictions (:432-476), solve started from the carried
 * multipliers, read-back or shift fallback (:484-524), plant (:528-543).  Instances are ordered [s][o].  All pointers are HIP
 * device pointers:
 *   d_own[n_own]            global indices of the owned vehicles, ascending
 *   d_table[n_own][T][7]    their plans sampled every dt; d_k0[S] start sample of every scenario; t = iteration number
 *   d_allpred[S][V][3][N]   x, y, psi of every vehicle's last prediction, vehicle order (the caller's all-gather)
 *   d_pred[S][n_own][7][N], d_state[S][n_own][5]   in/out;  d_status, d_iters int32[S n_own], d_stats fp64[S n_own][3] out
 *   d_carry int32[S n_own]  in/out: written with status == 0, read by the next call (t > 0) as cfz_mpc_set_carry_device */
int cfz_vsl_step(cfz_handle *h, int S, int V, int n_own, const int32_t *d_own, int T, const double *d_table, const int32_t *d_k0,
                 int t, const double *d_allpred, double *d_pred, double *d_state, int32_t *d_status, int32_t *d_iters,
                 double *d_stats, int32_t *d_carry, void *stream);

/* ---- dual warm start ----------------------------------------------------------------------
 * Vehicle.dual_ws (confrez/control/vehicle.py:233-296): for n fixed poses[n][3] = (x, y, psi) the duals
 * l, m [n][4*n_obs] that certify the separation d[n][n_obs] (may be NULL) of the vehicle body from every
 * static obstacle of the handle's spec.  The reference maximises that separation with IPOPT
 * (tol 1e-8); here it is the optimum in closed form: d = the Euclidean distance of the two polygons, the duals
 * encode the unit direction between their closest points (face-vertex and vertex-vertex cases alike) and satisfy
 * the rows (:276-280) exactly.  Polygons that touch or overlap get their best face normal (d <= 0). */
int cfz_dual_ws(cfz_handle *h, int n, const double *poses, double *l, double *m, double *d);

/* MultiVehiclePlanner.joint_dual_ws (confrez/control/multi_vehicle_planner.py:208-341): for n pairs of fixed poses
 * poses_this[n][3], poses_other[n][3] of two vehicles the duals lam[n][4] (faces of the first), mu[n][4] (faces of the
 * second), s[n][2] of the rows -b_this'lam - b_other'mu = d, A_this'lam + s = 0, A_other'mu - s = 0, |s| <= 1,
 * lam, mu >= 0 (:292-295) and the separation d[n] they certify (may be NULL).  The reference maximises d with IPOPT;
 * here: the optimum in closed form, d = the Euclidean distance of the two bodies, s = minus the unit direction between
 * their closest points (vertex-vertex closest features included). */
int cfz_joint_dual_ws(cfz_handle *h, int n, const double *poses_this, const double *poses_other, double *lam, double *mu,
                      double *s, double *d);

/* ---- Vehicle.state_ws (confrez/control/vehicle.py:99-231): warm-start plan through the strategy's tube -----------
 * One NLP per vehicle, B of them in one call (no handle: nothing is kept).  Instance b has n_sets[b] strategy steps,
 * T_b = N (n_sets[b] - 1) Euler steps and T_b + 1 trajectory points.
 *   init_pose[B][3]       x, y, psi of the first point (:131-138; v, delta, a0, w0 start at zero)
 *   final_heading[B]      psi of the last point (:194-195), NaN = free; the pointer may be NULL
 *   tube                  for every instance, for strategy steps 1..n_sets-1: back cell then front cell, each as
 *                         A[4][2] row-major followed by b[4] (24 doubles per step), instances back to back (:178-192)
 *   guess                 x, y, psi of every point, instances back to back (spline_ws, :199-205); NULL (spline_ws = False, what the
 *                         reference's scripts configure for vehicle_0: IPOPT then starts from zeros) = cfz_state_ws_default_guess
 *   traj (out)            x, y, psi, v, delta, a, w of every point, instances back to back; the last input is repeated
 *   status, iters, cost   per instance (may be NULL); status as in cfz_mpc_stats, the reference raises on status != 0
 * The solver is the interior point of the MPC path with the exact Hessian of the Lagrangian and IPOPT's delta_w ladder
 * driven by a curvature test; the Newton system is solved as a stage recursion (a Riccati sweep over the T stages with
 * the terminal-heading row, the only one that can lose rank, bordered and regularised: delta_c = 1e-9;
 * csrc/cfz_plan.inl).  With a terminal heading and a guess that stands still (guess = NULL) the first linearisation
 * is rank deficient -- the headings cannot move -- and the solve ends with status 2 after a few iterations: hence
 * the default guess through the tube when the caller has none (the speed along any guess is seeded here). */
#define CFZ_KERNEL_AUTO 0
#define CFZ_KERNEL_WIDE 1
#define CFZ_KERNEL_NARROW 2

typedef struct cfz_plan_options {
  int32_t N;              /* :100 steps per strategy step, 30 */
  int32_t max_iter;       /* :210 500 */
  int32_t bounded_input;  /* :104, :155-167 */
  int32_t stall_iters;    /* 0 (as the reference: an infeasible plan runs to max_iter); n > 0: status 5 after n iterations without
                           *   progress of the constraint violation, as in the MPC step -- a batch then does not wait for such a plan */
  int32_t kernel;         /* where the Riccati sweep keeps its per-stage data: 0 = by batch size (up to one plan per CU: CFZ_KERNEL_WIDE,
                           *   else CFZ_KERNEL_NARROW), CFZ_KERNEL_WIDE = 1 (in LDS, one plan per CU at a time: the fastest single plan),
                           *   CFZ_KERNEL_NARROW = 2 (in the workspace, several plans per CU: the highest throughput; also what a plan
                           *   too long for the LDS, T > 498, gets).  Same arithmetic in the same order: the two agree bit for bit. */
  int32_t reserved0;
  double dt;              /* :101 0.1 */
  double wb;              /* wheelbase */
  double shrink_tube;     /* :106 0.5 in the callers */
  double bounds[12];      /* lo,hi of x, y, v, delta, a, w */
  double tol;             /* :208 1e-2 */
  double constr_viol_tol; /* :209 1e-2 */
  double mu_init;         /* 0.1 (IPOPT's default, what the reference's state_ws runs with; 1e-3 until round 3) */
  double curv_kappa;      /* 1e-8 */
} cfz_plan_options;

void cfz_default_plan_options(cfz_plan_options *opt);

/* Workspace of the planning entry points: one HIP stream and the device buffers of the last call, kept and reused (a
 * planning call used to hipMalloc / hipFree seven to nine buffers and end in hipDeviceSynchronize, stalling every other
 * stream of the process).  The `_w` forms run on the workspace's stream and wait for that stream only; the plain forms
 * (cfz_state_ws, cfz_colloc, cfz_joint_colloc) use a workspace of their own per calling thread and device.  A workspace
 * is not thread-safe (one call at a time), like a handle. */
typedef struct cfz_plan_ws cfz_plan_ws;
int cfz_plan_ws_create(int device, cfz_plan_ws **out);
int cfz_plan_ws_destroy(cfz_plan_ws *ws);
/* Gives the device memory a workspace holds back to the runtime now (it is allocated again by the next call).  ws = NULL: the
 * calling thread's own workspaces behind the plain entry points, which otherwise live as long as the thread.  A workspace also
 * shrinks by itself: a call that used less than a quarter of a block above 256 MB releases that block at the start of the next. */
int cfz_plan_ws_trim(cfz_plan_ws *ws);
int cfz_state_ws_w(cfz_plan_ws *ws, int B, const cfz_plan_options *opt, const int32_t *n_sets, const double *init_pose,
                   const double *final_heading, const double *tube, const double *guess, double *traj, int32_t *status,
                   int32_t *iters, double *cost);
int cfz_state_ws(int device, int B, const cfz_plan_options *opt, const int32_t *n_sets, const double *init_pose,
                 const double *final_heading, const double *tube, const double *guess, double *traj, int32_t *status,
                 int32_t *iters, double *cost);
/* The guess cfz_state_ws takes for an instance when the caller passes none (host arithmetic, no GPU): x, y, psi of the
 * N (n_sets - 1) + 1 points of the piecewise-linear path from the initial pose through the centres of the back cells of strategy steps
 * 1 .. n_sets - 1 (centre = mean of the cell's vertices), heading at a step = direction from the back cell's centre to the front
 * cell's on the branch nearest the previous heading, the terminal heading (NaN = free) at the last step.
 * tube: (n_sets - 1) x 24 doubles as for cfz_state_ws; guess (out): (N (n_sets - 1) + 1) x 3.  0 = ok, -1 = bad argument. */
int cfz_state_ws_default_guess(int32_t n_sets, int32_t N, const double init_pose[3], double final_heading, const double *tube,
                               double *guess);

/* ---- Vehicle.setup_single_final_problem + solve_single_final_problem (confrez/control/vehicle.py:360-661) -------------
 * The single-vehicle collocation plan: N = N_per_set (n_sets - 1) intervals of free length dt, K = 5 Radau points each,
 * 6 N points per instance; B instances in one call (no handle: nothing is kept).
 *   spec                  wb, dmin (:369), g, bounds (:439-478) and the static obstacles (:523-541); N, dt, n_nbr, weights unused
 *   init_pose, final_heading, tube   as in cfz_state_ws (:426-436, :619-620, :570-617)
 *   guess                 x, y, psi, v, delta, a, w at every point, instances back to back (interp_ws_for_collocation's
 *                         output, :629-636); dt0[B] the initial interval length (:388-389)
 *   traj (out)            x, y, psi, v, delta, a, w at every point; dt (out) [B]
 *   status, iters, cost   per instance (may be NULL); the reference raises on status != 0
 * The OBCA duals l, m (:411-416) are eliminated as in the MPC step and rebuilt from the poses by cfz_dual_ws.  Same
 * interior point as cfz_state_ws; dt is bordered out of the banded system (csrc/cfz_colloc.inl). */
#define CFZ_COLLOC_K 5
typedef struct cfz_colloc_options {
  int32_t N_per_set;      /* :368 5 */
  int32_t max_iter;       /* IPOPT default 3000 (:652 leaves it unset) */
  int32_t exact_rows;     /* 0: dual regularisation of proximal type, delta_c = 1e-7 (rows met to delta_c x multiplier, robust where
                           *    the reference's rows lose rank); 1: IPOPT's form, delta_c = 1e-9 (exact optimum at tight tolerances) */
  int32_t one_pivot;      /* 0: the band is eliminated a panel of 16 pivots at a time (single plans: for batches up to two per CU);
                           *    1: one pivot at a time -- joint plan: same pivots, same arithmetic per entry, same factor; single
                           *    plans: the one-wavefront kernel with its LDS window.  Kept as the check of the panel version, ~2x slower */
  int32_t vv_rows;        /* 1 (default): a (point, obstacle) or (point, pair of vehicles) block whose closest features are two
                           *    vertices is constrained by their Euclidean distance -- the reference's OBCA rows admit any unit
                           *    direction (vehicle.py:523-541, multi_vehicle_planner.py:419-451); 0: face-normal certificates only
                           *    (a restriction at corner-to-corner contacts, kept to show the gap) */
  int32_t kernel;         /* must be 0: the field named the one-wavefront collocation kernel that round 4 retired (slower at every batch size,
                           *    and not deterministic: docs/notebook.md); any other value is an error since round 5 (the slot keeps the layout) */
  double shrink_tube;     /* :370; 0.5 in plan_single_path */
  double tol;             /* :650 1e-2 */
  double constr_viol_tol; /* :651 1e-2 */
  double mu_init;         /* 0.1 (IPOPT's default) */
  double curv_kappa;      /* 1e-8 */
  int32_t structured;     /* 0 or 1 (any other value is an error since round 6).  1 (default): the Newton system is eliminated interval by interval,
                           *    csrc/cfz_jstruct.inl -- vehicle-major ordering (a band of half-bandwidth 51 per vehicle, the condensed pair blocks of a
                           *    joint plan beside it), tube rows condensed, every vehicle's interiors (64 unknowns) by themselves on the matrix cores,
                           *    the pair-coupled poses of an interval index through a 64 x 64 capacitance system, a block recursion over separators of
                           *    at most 15 unknowns per vehicle that keeps every hand-off in registers; single plans (cfz_colloc) run the same scheme
                           *    with 16-row blocks.  0 (also what one_pivot = 1 takes, and what a plan of more than 255 intervals per vehicle is routed
                           *    to): pivot by pivot along the band, for a joint plan the band across the vehicles (half-bandwidth ~300, 88 MB per
                           *    four-vehicle plan) a panel at a time: same matrix, same solution to rounding, 3-6x slower.  (Round 4's scheme for single
                           *    plans, 2 until round 5, is gone: its separator recursion handed blocks from wavefront to wavefront through global
                           *    memory.) */
  int32_t reserved1;
} cfz_colloc_options;

void cfz_default_colloc_options(cfz_colloc_options *opt);
int cfz_colloc_w(cfz_plan_ws *ws, int B, const cfz_spec *spec, const cfz_colloc_options *opt, const int32_t *n_sets,
                 const double *init_pose, const double *final_heading, const double *tube, const double *guess,
                 const double *dt0, double *traj, double *dt, int32_t *status, int32_t *iters, double *cost);
int cfz_colloc(int device, int B, const cfz_spec *spec, const cfz_colloc_options *opt, const int32_t *n_sets,
               const double *init_pose, const double *final_heading, const double *tube, const double *guess,
               const double *dt0, double *traj, double *dt, int32_t *status, int32_t *iters, double *cost);

/* ---- MultiVehiclePlanner.solve_final_problem_obca (confrez/control/multi_vehicle_planner.py:343-480) -----------------------
 * The joint plan: the collocation problems of V vehicles (each as in cfz_colloc, from its own single-vehicle result) with ONE
 * shared interval length dt (:365-366), cost sum_a J_a (:387), and for every pair of vehicles and every collocation point
 * of the shorter plan the two bodies at least spec->dmin apart (:389-456).  B independent instances (scenarios) of V vehicles
 * each in one launch, one workgroup per instance (BASELINE.json configs[3]); the reference solves one.
 *   n_sets[B*V], init_pose[B*V][3], final_heading[B*V], tube, guess   per vehicle, instance-major, as in cfz_colloc
 *   dt0[B]                initial shared interval length (:361 the mean of the single results')
 *   pairs[n_pairs][2]     vehicle index pairs a < b with a separation row, the same for every instance; NULL = all pairs (:56-58)
 *   traj (out)            x, y, psi, v, delta, a, w at every point, vehicles back to back; dt (out) [B]
 *   status, iters, cost   per instance (may be NULL)
 * The vehicle-vehicle OBCA duals (:404-431) are eliminated like the obstacle duals (two smooth rows per pair and point over a
 * working set) and rebuilt from the poses by cfz_joint_dual_ws.  The vehicles' interval blocks are interleaved in time, which
 * widens the band to ~100 V; the elimination then runs from global memory (csrc/cfz_colloc.inl). */
int cfz_joint_colloc_w(cfz_plan_ws *ws, int B, int V, const cfz_spec *spec, const cfz_colloc_options *opt, const int32_t *n_sets,
                       const double *init_pose, const double *final_heading, const double *tube, const double *guess, const double *dt0,
                       int n_pairs, const int32_t *pairs, double *traj, double *dt, int32_t *status, int32_t *iters, double *cost);
int cfz_joint_colloc(int device, int B, int V, const cfz_spec *spec, const cfz_colloc_options *opt, const int32_t *n_sets,
                     const double *init_pose, const double *final_heading, const double *tube, const double *guess, const double *dt0,
                     int n_pairs, const int32_t *pairs, double *traj, double *dt, int32_t *status, int32_t *iters, double *cost);

/* Size of the banded primal-dual system one (joint) collocation plan is eliminated on (host arithmetic, no device): unknowns nk,
 * half-bandwidth kb of the ordering, bytes of the band as stored (LAPACK general-band layout, nk x (3 kb + 1) doubles).  V vehicles
 * with n_sets[V] strategy steps each, has_final[V] (NULL = all have a terminal heading), pairs as in cfz_joint_colloc (NULL = all
 * pairs; V = 1: none).  bench.py prices the planning kernels' HBM traffic with it.  Any output pointer may be NULL. */
int cfz_colloc_band_info(int V, const int32_t *n_sets, const int32_t *has_final, int N_per_set, int n_obs, int n_pairs,
                         const int32_t *pairs, int32_t *nk, int32_t *kb, int64_t *band_bytes);

/* The same for the elimination a plan actually goes through (`structured` as in cfz_colloc_options: 1 = interval by interval,
 * cfz_jstruct.inl -- vehicle-major ordering, half-bandwidth 51, tube rows condensed; 0 = along the band):
 * alg_bytes = the bytes one Newton system's elimination moves between its phases (every array written once and read where another phase
 * consumes it: csrc/cfz_jstruct.inl jstruct_alg_doubles; the band path: 3 x the band), what bench.py
 * prices the planning kernels' HBM traffic with; workspace_bytes = the plan's slab in HBM.  Any output pointer may be NULL. */
int cfz_colloc_elimination_info(int V, const int32_t *n_sets, const int32_t *has_final, int N_per_set, int n_obs, int n_pairs, const int32_t *pairs,
                                int structured, int32_t *nk, int32_t *kb, int64_t *band_bytes, int64_t *alg_bytes, int64_t *workspace_bytes);

/* Layout version of the structs of this header (cfz_spec, cfz_options, cfz_colloc_options, cfz_plan_options): a binding compares it with the
 * CFZ_ABI_VERSION it was written against before it passes a struct (conflict_rez_amd/engine.py does).  Round 5: 5; round 6: 6
 * (cfz_colloc_options.structured lost its value 2: a caller that still passes it is refused instead of silently taking another path). */
#define CFZ_ABI_VERSION 6
int cfz_abi_version(void);

/* ---- batched closed loop of MultiDistributedFollower.solve (:630-663) ---------------------
 * S scenarios x V vehicles (V = n_nbr + 1), B = S*V instances ordered [s][v].
 * ref_table[V][T][7]: each vehicle's planned trajectory (x,y,psi,v,delta,a,w) sampled every dt
 * (what get_current_ref :370-404 interpolates); scenario s starts at sample k0[s].
 * cfz_loop_init sets state = ref_table[v][k0][0:5] + noise[s][v][5] and the first prediction =
 * the plan at the horizon times (:397-400).
 * cfz_loop_step does one iteration for all scenarios, entirely on the device:
 *   neighbours' predictions copied first (get_others_pred :636-637), every vehicle's
 *   step(): parameters + shifted warm start (:432-476), solve (:479), read-back or shift
 *   fallback (:484-524), clock += dt (:526), plant integration over dt with (a0,w0) (:528-543).
 * Exchange rule (cfz_loop_set_order): with no order set (the default), Jacobi: every vehicle plans against the others'
 * predictions of the previous iteration, advanced one step.  With an order, the V solves of scenario s run one after
 * another in the order order[s]: the vehicle of rank r plans against the predictions of the vehicles ranked before it
 * from this same iteration (after their solve or their shift fallback; they already start at this iteration's time, so
 * they are not advanced) and the previous iteration's predictions of the others, advanced.  Measured state, reference,
 * warm start (its own previous prediction, advanced), carried multipliers, read-back, fallback, plant and record are the
 * same in both rules.  A converged solve then keeps dmin - constr_viol_tol from the prediction of every vehicle ranked
 * before it at stages 1..N-1; the realised states after the plant are not bounded so (the stage-0 dynamics defect and the
 * plant's finer integration separate them from the predictions): cfz_loop_audit measures them. */
int cfz_loop_init(cfz_handle *h, int S, int T, const double *ref_table, const int32_t *k0, const double *noise);
int cfz_loop_step(cfz_handle *h);
/* K iterations for all scenarios in one persistent launch: the V solves of a scenario exchange predictions by the rule
 * above (Jacobi, or in the order of cfz_loop_set_order), but scenarios no longer wait for each other between iterations.
 * Same results, bit for bit, as K calls of cfz_loop_step under the same rule.  cfz_loop_last_iterations: IPM iterations
 * summed over all solves of that call. */
int cfz_loop_run(cfz_handle *h, int K);
long cfz_loop_last_iterations(const cfz_handle *h);
/* solves of that call that converged (status 0); the others took the reference's shift fallback (:501-524) */
long cfz_loop_last_converged(const cfz_handle *h);
/* how the solves of that call ended: counts[s] = solves with status s (0 converged, 1 iteration limit, 2 line search, 3 non-finite,
 * 4 measured state infeasible (in collision or outside the boxes: no iteration), 5 stalled / locally infeasible) */
int cfz_loop_last_status_counts(const cfz_handle *h, long counts[6]);
/* state[S][V][5], pred[S][V][7][N], status int32[S][V] of the last step; NULL to skip. */
int cfz_loop_get(cfz_handle *h, double *state, double *pred, int32_t *status, int32_t *iters);
/* Exchange order of the closed loop (cfz_loop_step, cfz_loop_run).  order[S][V]: row s is the order in which the V vehicles
 * of scenario s solve within one MPC iteration; a vehicle sees the predictions of those before it from the same iteration and
 * those of the others from the previous one, advanced one step.  NULL: Jacobi, every vehicle sees the previous iteration's
 * predictions (the reference, vehicle_follower.py:636-641).  cfz_loop_init / cfz_loop_init_tables reset it to NULL.
 * The order holds for every later step and run until it is changed; it may change between calls (at a step boundary all
 * predictions start at the same time).  Refused: a call before cfz_loop_init, a row that is not a permutation of 0..V-1
 * (the order in force stays). */
int cfz_loop_set_order(cfz_handle *h, const int32_t *order);

/* ---- disturbances of the closed loop ------------------------------------------------------------------------------------------
 * The reference's follower measures its state exactly (opti.set_value of the current state, to which stage 0 is pinned,
 * vehicle_follower.py:194-199) and its plant applies the solver's input exactly (:528-543).  With a disturbance set, step t of
 * scenario s, vehicle v (cfz_loop_step and cfz_loop_run alike, under either exchange rule) becomes:
 *   1. the solver's x0 is the measurement, state + d[0:5] (:194-199); the true state is kept;
 *   2. parameters, warm start, solve, read-back or shift fallback as without (a measurement inside a clearance or outside the boxes
 *      ends in status 4 and takes the fallback);
 *   3. the applied input is (a0 + d[5], w0 + d[6]) clipped to the spec's input box, (a0, w0) being what the step would apply;
 *   4. the new state is the plant (:528-543) from the TRUE state with the applied input, plus d[7:12];
 *   5. the record (cfz_loop_record) keeps that true state and the applied input.  Predictions are the solver's own.
 * d[i] = level[s] * sigma[i] * z[i], sigma = sigma_meas (x, y, psi, v, delta) | sigma_act (a, w) | sigma_proc (x, y, psi, v, delta) and
 * z the twelve standard normals of (seed, stream[s], v, t): Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 * (stream[s], v, t, j), j = 0..5, each call's four words giving z[2j], z[2j+1] by Box-Muller (csrc/cfz_disturb.inl states the
 * bits).  t counts the MPC iterations done since cfz_loop_init / cfz_loop_init_tables.  A stream depends on (seed, stream id,
 * vehicle, step) alone: not on S, on the workgroup that serves the item, on the exchange rule or on stepping against running.
 * cfz_loop_set_disturbance: a NULL sigma group is zeros; all three NULL switch the disturbance off (the undisturbed kernels run
 * again).  level[S] NULL: 1; stream[S] NULL: s.  The setting holds until it is changed and may change between calls, the step count
 * keeps running; cfz_loop_init / cfz_loop_init_tables switch it off and reset the count.  Refused, the setting in force staying: a
 * call before cfz_loop_init, a negative or non-finite sigma or level.
 * cfz_loop_disturbance: d[K][S][V][12] that the loop adds at steps [t0, t0 + K) under the setting in force, past or future (a pure
 * function of the setting); each d is a rounded double that the loop adds in one rounded addition, so a host replay that
 * downloads d has the loop's exact inputs.  Refused when no disturbance is set, t0 < 0, K < 1. */
int cfz_loop_set_disturbance(cfz_handle *h, uint64_t seed, const double sigma_meas[5], const double sigma_act[2],
                             const double sigma_proc[5], const double *level /* [S] or NULL: 1 */,
                             const uint32_t *stream /* [S] or NULL: s */);
int cfz_loop_disturbance(cfz_handle *h, int t0, int K, double *d /* [K][S][V][12] */);

/* ---- lossy prediction exchange of the closed loop ---------------------------------------------------------------------------------
 * Above, every vehicle receives every neighbour's newest prediction, complete and on time.  The reference's deployment does not: a
 * callback overwrites others_pred[other] with whichever VehiclePredictionMsg arrived last (ros2_ws/src/confrez_ros/src/vehicle_node.py:
 * 154-163), timer_callback steps on a timer with whatever is there (:171-189), and step() advances that message by one stage whatever
 * its age (_adv_onestep, vehicle_follower.py:413-426): a late or lost message means a stale prediction, read time-shifted.  With a
 * comm setting, cfz_loop_step and cfz_loop_run alike, under either exchange rule (csrc/cfz_comm.inl states the model once):
 *   Messages.  In MPC iteration tau (counted since cfz_loop_init / cfz_loop_init_tables) vehicle u of scenario s publishes its
 *     prediction after that iteration, the solution or the shift fallback: message tau, which starts at time tau.
 *   Delivery.  delivered(s, v <- u, tau) = u1 > p_drop[s], u1 in (0, 1] the first uniform of the Philox4x32-10 call with key
 *     (seed & 0xffffffff, seed >> 32) and counter (stream[s], v, tau + 1, 8 + u), v the receiver; u1 = (((w0 >> 5) << 26) + (w1 >> 6)
 *     + 1) * 2^-53.  Word 3 is 8..15: never a noise pair 0..5 of cfz_loop_set_disturbance, even under an equal seed.  p_drop = 0
 *     delivers everything, p_drop = 1 nothing.  A bit depends on (seed, stream id, receiver, sender, tau) alone: not on S, on the
 *     workgroup, on the exchange rule or on stepping against running.
 *   Want.  In iteration t vehicle v wants message tau* = t - 1 of a neighbour (Jacobi), tau* = t of one ranked before it (sequential).
 *   Age.  v reads message tau* - a, a the smallest a >= 0 with delivered(tau* - a), or a = min(max_age, tau* - tau_on): tau_on is the
 *     message standing in the predictions when cfz_loop_set_comm was called; it counts as delivered and history starts there.  A message
 *     of age max_age always gets through: the staleness is bounded.
 *   Row.  Stage k of the neighbour's block reads row min(k + fresh + (compensate ? a : 0), N - 1) of that message, fresh = 1 under
 *     Jacobi and 0 for a vehicle ranked before (what is read without loss).  compensate = 0 is the reference node, the last message
 *     advanced as if it were new; compensate = 1 advances it by its age.
 * The vehicle's own warm start, reference window, carried multipliers, read-back, fallback, plant, record, audit and disturbances are
 * unaffected: a vehicle never loses its own prediction.  cfz_loop_get, the record and the audit see the newest messages.
 * cfz_loop_set_comm: p_drop NULL switches the exchange back to lossless (the kernels that ran before run again).  stream[S] NULL: s.
 * Every call that switches it on restarts history at the current predictions.  cfz_loop_init / cfz_loop_init_tables switch it off.
 * Refused, the loop's state and the setting in force staying: a call before cfz_loop_init, a p_drop outside [0, 1] or not finite,
 * max_age outside 1..CFZ_MAX_AGE, compensate other than 0 or 1.
 * cfz_loop_comm: the delivery bits of messages [tau0, tau0 + K) under the setting in force, past or future (a pure function of the
 * setting), delivered[k][s][v][u] for receiver v and sender u, the diagonal 1.  The bits, not the ages: a host replay states the age
 * rule itself.  Refused when no comm setting is on, tau0 < 0, K < 1.
 * cfz_vsl_step is untouched: its caller gathers the predictions and owns their delivery. */
#define CFZ_MAX_AGE 6
int cfz_loop_set_comm(cfz_handle *h, uint64_t seed, const double *p_drop /* [S], NULL: off */, int max_age /* 1..CFZ_MAX_AGE */,
                      int compensate /* 0 | 1 */, const uint32_t *stream /* [S] or NULL: s */);
int cfz_loop_comm(cfz_handle *h, int tau0, int K, int32_t *delivered /* [K][S][V][V], diagonal 1 */);

/* ---- per-scenario problem constants of the closed loop ------------------------------------------------------------------------------
 * The constants of the NLP are what `setup_controller(dt, N, dmin)` bakes into the graph once per follower (vehicle_follower.py:146-368);
 * above they are the handle's, one set for every scenario.  A *problem* is a pair (cfz_spec, cfz_options).  With a pool of P problems
 * and problem_of[S], every solve of scenario s (cfz_loop_step and cfz_loop_run alike, under either exchange rule, with or without
 * disturbances and lossy exchange) uses problem problem_of[s]: its dmin, bounds and weights, every field of cfz_options, the constants
 * derived from them, and the stage-0 feasibility test that yields status 4.  The clip of the disturbed input (cfz_loop_set_disturbance,
 * step 3) uses that problem's input box, and happens only while a disturbance is set: with none set the applied input is clipped to
 * no box, under cfz_loop_step and cfz_loop_run alike.  (Without a pool, cfz_loop_run under cfz_loop_set_comm alone does clip to the
 * handle's box.  A pool of the handle's own problem therefore equals no pool under comm as long as every applied input lies inside
 * that box: a converged solve's always does, a shift fallback's does when the inputs of the plan that seeded the predictions do.)
 * The handle's, whatever the pool says: geometry and time base (N, n_obs, n_nbr, rk_substeps, dt, wb, g, A_obs, b_obs: the plant, the
 * audit, the workspace layout and the carry records are built from them) and cfz_options.carry_duals (the carry records are sized by
 * cfz_create).  A pool entry that differs from the handle in any of these is refused, and cfz_last_error names the field.
 * Everything else about a step is unchanged and per scenario as before: reference window, warm start, carried multipliers (slot b),
 * exchange rule, disturbances, lossy exchange, read-back or fallback, plant, record, audit (which measures signed distance, not dmin).
 * The setting holds until it is changed and may change between calls, at a step boundary; carried multipliers stay (a warm start, not
 * a promise).  cfz_loop_init / cfz_loop_init_tables switch it off.  Off is the default, and with it off the kernels that ran before
 * run again.  cfz_vsl_step and the host-buffer path cfz_mpc_solve* always use the handle's constants.
 * cfz_problem_check: host arithmetic, no device.  0 if (spec, opt) may stand in a pool of a handle created with (base, base_opt), else -1
 * and cfz_last_error names the first field that differs or is invalid.  The value checks are cfz_create's own (sizes, filter_cap,
 * restoration, reg_dual_rows, resto_first, obstacles that are bounded quadrilaterals), and every box of `bounds` must have lo <= hi, both
 * finite.  base_opt NULL: the default options; opt NULL: base_opt.
 * cfz_loop_set_problems: specs[P], opts[P] (NULL: the handle's options for every entry), problem_of[S]; P = 0 or specs NULL: off.
 * Refused, the loop's state and the setting in force staying: a call before cfz_loop_init, P < 0, a problem_of[s] outside [0, P), any
 * entry that cfz_problem_check refuses (the text is then prefixed with "problem p: "). */
int cfz_problem_check(const cfz_spec *base, const cfz_options *base_opt, const cfz_spec *spec, const cfz_options *opt);
int cfz_loop_set_problems(cfz_handle *h, int P, const cfz_spec *specs, const cfz_options *opts, const int32_t *problem_of);

/* ---- per-scenario obstacle maps of the closed loop -----------------------------------------------------------------------------------
 * Above, every scenario of a launch stands on the handle's obstacles.  A *map* is n_obs obstacles, A_obs[n_obs][4][2] and
 * b_obs[n_obs][4] as in cfz_spec; n_obs is the handle's (the workspace layout, the LDS size and the carry records are built from it).
 * With a pool of M maps and map_of[S], every solve of scenario s (cfz_loop_step and cfz_loop_run alike, under either exchange rule,
 * with or without disturbances and lossy exchange) uses the obstacles of map map_of[s]: for its separation rows, its working set, the
 * stage-0 feasibility test that yields status 4, and its restoration.  Nothing else about a step changes.
 * The setting composes with cfz_loop_set_problems, in either call order: scenario s then solves problem problem_of[s] on map
 * map_of[s].  A pool problem still carries the handle's obstacles (cfz_problem_check is unchanged); the map comes from here.  The
 * same kernels run as under a problem pool; with maps alone every scenario solves the handle's problem, and the applied input is
 * clipped only while a disturbance is set, as under a problem pool.
 * The audit follows the map: cfz_loop_audit measures the vehicle-obstacle signed distance of scenario s against map map_of[s] under
 * the mapping in force WHEN IT IS CALLED (not the one a recorded step was solved under), and where[s][5] is the obstacle's index
 * within that map.  cfz_audit_maps is cfz_audit with the maps given by the caller (M = 0 or A_obs NULL: the handle's map, which is
 * cfz_audit); it does not read the loop's setting.  The vehicle-vehicle column does not depend on the map.
 * The setting holds until it is changed and may change between calls, at a step boundary; carried multipliers and working-set codes
 * stay (a warm start, not a promise).  cfz_loop_init / cfz_loop_init_tables switch it off.  Off is the default, and with it off the
 * kernels that ran before run again.  cfz_mpc_solve*, cfz_vsl_step, cfz_dual_ws and the planning entry points keep the handle's map.
 * cfz_map_check: host arithmetic, no device.  0 if the base->n_obs obstacles may stand in a map pool of a handle created with `base`:
 * every entry finite and every obstacle a bounded quadrilateral (the check cfz_create makes); else -1 and cfz_last_error names the
 * obstacle ("obstacle j ...").
 * cfz_loop_set_maps: A_obs[M][n_obs][4][2], b_obs[M][n_obs][4], map_of[S]; M = 0 or A_obs NULL: off.  Refused, the loop's state and the
 * setting in force staying: a call before cfz_loop_init, M < 0, a map_of[s] outside [0, M), any map that cfz_map_check refuses (the
 * text is then prefixed with "map m: "). */
int cfz_map_check(const cfz_spec *base, const double *A_obs /* [n_obs][4][2] */, const double *b_obs /* [n_obs][4] */);
int cfz_loop_set_maps(cfz_handle *h, int M, const double *A_obs /* [M][n_obs][4][2] */, const double *b_obs /* [M][n_obs][4] */,
                      const int32_t *map_of /* [S] */);

/* ---- closed loop over per-scenario plans -------------------------------------------------------
 * tables[P][V][T][7]: a pool of P plan sets (each what cfz_loop_init takes as ref_table); scenario s follows set table_of[s]
 * (NULL: set s, which needs P == S).  Otherwise exactly cfz_loop_init, which is this call with P = 1 and every scenario on set 0.
 * Refused: P < 1, table_of[s] outside [0, P), S * V > max_batch, NULL tables or k0. */
int cfz_loop_init_tables(cfz_handle *h, int S, int P, int T, const double *tables, const int32_t *table_of, const int32_t *k0,
                         const double *noise);

/* ---- record of the realised trajectory (the reference's `final_traj`, vehicle_follower.py:74-82, :526-563) ----------------
 * cfz_loop_record(h, K): the next K steps (of cfz_loop_step and cfz_loop_run alike) each write, per scenario and vehicle, the
 * state after the plant (x, y, psi, v, delta) and the applied input (a, w) (:556-563), and the status and iterations of that
 * step's solve.  K = 0 stops recording and frees the record; cfz_loop_init / cfz_loop_init_tables do the same.  A step or run
 * that would go past K recorded steps is refused before anything is launched (the loop's state stays as it was).
 * cfz_loop_history: recorded steps [t0, t0 + K) as traj[K][S][V][7], status[K][S][V], iters[K][S][V]; any output may be NULL. */
int cfz_loop_record(cfz_handle *h, int K);
int cfz_loop_history(cfz_handle *h, int t0, int K, double *traj, int32_t *status, int32_t *iters);

/* ---- audit of a realised trajectory --------------------------------------------------------------------------------------
 * Signed distance of two convex polygons: their Euclidean distance if they are disjoint, else minus the penetration depth (the
 * smallest overlap of their projections over the face normals of both, 0 when they only touch).  Bodies: the spec's rectangle g
 * at (x, y, psi); obstacles: the spec's n_obs polygons.  Per scenario s over the steps [t0, t0 + K) (step numbers relative to t0):
 *   clear[s][0] the smallest vehicle-vehicle signed distance, where[s][0:3] its (step, u, w) with u < w;
 *   clear[s][1] the smallest vehicle-obstacle signed distance, where[s][3:6] its (step, v, j)   (+inf and -1: nothing to measure);
 *   first_contact[s] the first step with a negative signed distance, -1 if none;
 *   arrive[s][v] the first step at which vehicle v is within pos_tol of its goal in (x, y), within psi_tol of its heading
 *   (wrapped) and |v| <= v_tol, -1 if never.
 * Ties go to the lowest step, then the lowest index.  One wavefront per scenario, deterministic.  Any output may be NULL.
 * cfz_loop_audit: the handle's record; goals = the last sample of the table each scenario follows.
 * cfz_audit: a host trajectory traj[K][S][V][7] (x, y, psi, v, ...: what cfz_loop_history returns, or a `_follower_final.pkl`
 * of the reference laid out so) with goal[S][V][3]; V in 1..CFZ_MAX_NBR+1 need not be the handle's.
 * cfz_loop_audit follows cfz_loop_set_maps (the mapping in force when it is called); cfz_audit_maps takes M maps and map_of[S] from
 * the caller, see "per-scenario obstacle maps" above.  Refused there: M < 0, a map_of[s] outside [0, M), a map cfz_map_check refuses. */
int cfz_loop_audit(cfz_handle *h, int t0, int K, double pos_tol, double psi_tol, double v_tol, double *clear, int32_t *where,
                   int32_t *first_contact, int32_t *arrive);
int cfz_audit(cfz_handle *h, int K, int S, int V, const double *traj, const double *goal, double pos_tol, double psi_tol, double v_tol,
              double *clear, int32_t *where, int32_t *first_contact, int32_t *arrive);
int cfz_audit_maps(cfz_handle *h, int K, int S, int V, const double *traj, const double *goal, int M, const double *A_obs /* [M][n_obs][4][2] */,
                   const double *b_obs /* [M][n_obs][4] */, const int32_t *map_of /* [S] */, double pos_tol, double psi_tol, double v_tol,
                   double *clear, int32_t *where, int32_t *first_contact, int32_t *arrive);

/* ---- score of a realised trajectory --------------------------------------------------------------------------------------
 * What the closed loop cost, per scenario s and vehicle v over the recorded steps [t0, t0 + K) (step numbers relative to t0).  The audit
 * above says whether the loop was safe; this measures the reference's own objective along the trajectory actually driven
 * (vehicle_follower.py:263-272: tracking error, a^2, v^2 w^2, delta^2; the six sums below in the order of cfz_spec.weights), the price
 * of yielding and how long a vehicle ran on the shift fallback (:501-524; back_up_steps counts the same consecutive failures).
 * Record row z_t = (x, y, psi, v, delta, a, w) with status_t, iters_t as cfz_loop_history returns them; its plan row is
 * r_t = plan[min(k0[s] + t + 1, T - 1)], plan[T][7] the vehicle's plan in the set table_of[s] and k0[s] the clock index of the state
 * before the window's first step (the loop seeds the state at plan[k0] and step t integrates the plant from clock k0 + t to
 * k0 + t + 1, so a vehicle that follows its plan exactly has z_t = r_t; the clamp is that of the loop's reference window).
 * arrive is cfz_loop_audit's arrival against the plan's last sample; upto = arrive + 1 if the vehicle arrived, else K.  Every quantity
 * runs over t < upto: a vehicle that parks early is not charged for standing at its goal.
 *   val[s][v][0:3]  dx2, dy2, psi2: sum (x - x_r)^2, (y - y_r)^2, wrap(psi - psi_r)^2, wrap(e) = e - 2 pi rint(e (1 / 2 pi))
 *   val[s][v][3:6]  a2, vw2, delta2: sum a^2, (v w)^2, delta^2
 *   val[s][v][6:8]  da2, dw2: sum over 1 <= t < upto of (a_t - a_{t-1})^2, (w_t - w_{t-1})^2
 *   val[s][v][8]    absv: sum |v_t| (dt absv is the distance travelled)
 *   val[s][v][9]    dev2_max: max_t (x - x_r)^2 + (y - y_r)^2, ties to the lowest step
 *   cnt[s][v][0:2]  steps = upto, arrive (-1: never)
 *   cnt[s][v][2:4]  failed: steps with status != 0; fail_run: the longest run of consecutive such steps
 *   cnt[s][v][4]    reversals: changes of sign in the sequence of sign(v_t) over the steps with |v_t| > v_tol
 *   cnt[s][v][5]    waiting: steps with |v_t| <= v_tol and (t < arrive or never arrived)
 *   cnt[s][v][6:8]  near_steps: steps at which the signed distance of this body to any other body of the scenario is < near [m] (bodies
 *                   that touch count at every near); first_near: the first such step, -1 none
 *   cnt[s][v][8:10] iters_sum, iters_max of iters_t
 *   cnt[s][v][10]   dev_max_step: the step of dev2_max
 * Raw sums: means, roots, dt and the weights are the caller's (conflict_rez_amd/engine.py, score_summary).  One wavefront per scenario;
 * a vehicle's steps are summed in one fixed tree, so the same record gives the same bits on every run (conflict_rez_amd/csrc/cfz_score.inl).
 * cfz_loop_score: the handle's record, plan pool, table_of and clock (k0[s] = the clock now minus the steps recorded after t0).
 * cfz_score: host arrays traj[K][S][V][7], status[K][S][V] and iters[K][S][V] (either NULL: all 0), tables[P][V][T][7], table_of[S],
 * k0[S]; V in 1..CFZ_MAX_NBR+1 need not be the handle's; the body is the handle's.
 * Refused: a window outside the record, non-positive sizes, a table_of[s] outside [0, P), a negative k0[s], a negative or non-finite
 * near, a NULL pointer other than status and iters. */
#define CFZ_SCORE_NVAL 10
#define CFZ_SCORE_NCNT 11
int cfz_loop_score(cfz_handle *h, int t0, int K, double pos_tol, double psi_tol, double v_tol, double near, double *val, int32_t *cnt);
int cfz_score(cfz_handle *h, int K, int S, int V, const double *traj, const int32_t *status, const int32_t *iters, int P, int T,
              const double *tables /* [P][V][T][7] */, const int32_t *table_of /* [S] */, const int32_t *k0 /* [S] */, double pos_tol,
              double psi_tol, double v_tol, double near, double *val, int32_t *cnt);

/* ---- conflict map of a set of plans ---------------------------------------------------------------------------------------
 * Body clearance of every pair of plans against their relative delay, before any closed loop is run.  The audit and the score above
 * inspect a loop that was driven, in which all vehicles of a scenario share one clock; this inspects the plans themselves and shifts the
 * clock of one vehicle of a pair against the other's.
 * Inputs: tables[P][V][T][7], a pool of plan sets as cfz_loop_init_tables takes it (rows x, y, psi, ...; only those three are read); a
 * window D >= 0 in samples; margin >= 0 in metres.
 * Pairs q = (u, w), u < w, in the audit's order (0,1), (0,2), ..., (1,2), ...; npair = V (V - 1) / 2.  Lag tau in [-D, D] is stored at
 * index tau + D.  tau > 0: w runs tau samples late; tau < 0: u runs |tau| samples late.  A late vehicle waits at its first sample; a
 * vehicle past its plan stays at its last sample.  For step i in [0, T + |tau|):
 *   iu  = clamp(i - max(-tau, 0), 0, T - 1)
 *   iw  = clamp(i - max( tau, 0), 0, T - 1)
 *   d_i = signed distance of the handle's body rectangle at tables[p][u][iu][0:3] and at tables[p][w][iw][0:3]: the Euclidean distance
 *         if the bodies are disjoint, else minus the penetration depth (0 when they only touch), as the audit's clear.
 *   clear[p][q][tau + D]    min_i d_i (+inf if every d_i is NaN)
 *   info[p][q][tau + D][0]  when: the lowest i that attains it (-1 if every d_i is NaN)
 *   info[p][q][tau + D][1]  first: the lowest i with d_i < margin, -1 if there is none
 *   info[p][q][tau + D][2]  count: the number of such i
 * The comparison with margin is made without a root, on the key that the kernel minimises (the squared distance of disjoint bodies, minus
 * the depth otherwise): disjoint bodies count when key < margin^2, touching or overlapping bodies when key < margin, so bodies that only
 * touch count at every margin > 0 and at margin = 0 exactly the overlapping ones do.  A d_i within rounding of margin may fall on
 * either side.
 * One workgroup per (set, pair); minima are taken under the total order (d, i), counts are integers: the same tables give the same bits on
 * every run (conflict_rez_amd/csrc/cfz_conflict.inl).
 * cfz_plan_conflicts: host tables; V in 1..CFZ_MAX_NBR+1 need not be the handle's, the body is the handle's; V = 1 has no pairs: it
 * returns 0, launches nothing and writes nothing.  cfz_loop_plan_conflicts: the pool that cfz_loop_init* left on the device, P, V, T
 * its own; nothing is uploaded and the loop's state, clock and record are left untouched.  Either output may be NULL.
 * Refused: non-positive P, V or T, V above CFZ_MAX_NBR+1, D < 0, a negative or non-finite margin, NULL tables, sizes whose outputs
 * would pass 2^31 entries, the loop form before cfz_loop_init*.  What needs no handle is checked before the handle is looked at. */
#define CFZ_CONFLICT_NINFO 3 /* when, first, count */
int cfz_plan_conflicts(cfz_handle *h, int P, int V, int T, const double *tables /* [P][V][T][7] */, int D, double margin,
                       double *clear /* [P][npair][2D+1] */, int32_t *info /* [P][npair][2D+1][3] */);
int cfz_loop_plan_conflicts(cfz_handle *h, int D, double margin, double *clear, int32_t *info);

/* ---- start delays that resolve a plan set's conflicts ----------------------------------------------------------------------
 * How late which vehicle of a plan set must leave so that no pair of plans comes within the margin, searched over the conflict map above.
 * If the vehicles of a set start d[0..V-1] samples late, each waiting at its first sample, pair (u, w) visits exactly the body
 * configurations of the map's lag tau = d[w] - d[u]: while both wait they stand as at step 0 of that lag, after that the steps are the
 * same steps, beyond T + |tau| both rest at their last samples.  So the pair stays clear under d exactly when count[p][q][tau + D] == 0,
 * and its smallest clearance under d is clear[p][q][tau + D], bit for bit.
 * Inputs per plan set p: the map count[p][npair][2D+1], optionally clear of the same shape; a slack r >= 0 in samples; caps cap[p][v] in
 * [0, D] (NULL: D for every vehicle), the most vehicle v may be delayed; 0: it must leave on time.
 * A lag index j is free for pair q when count[p][q][j] == 0 and, where clear is given, clear[p][q][j] is finite (a pair whose distances
 * are all NaN, from a plan that did not converge, is not free).
 * A delay vector d, 0 <= d[v] <= cap[p][v], is feasible with slack r when for every pair q = (u, w) in the audit's order every lag tau' in
 * [d[w] - d[u] - r, d[w] - d[u] + r] lies inside [-D, D] and is free; lags outside the window are unknown and count as not free, so
 * |d[w] - d[u]| + r <= D is required.  With r > 0 the answer tolerates either vehicle of any pair slipping up to r further samples.
 * The answer is the feasible d that is smallest under the total order (span, total, tuple): span = max_v d[v]; total = sum_v d[v]; the
 * tuple compared lexicographically with vehicle 0 most significant, that is the integer idx = sum_v d[v] (D+1)^(V-1-v).  It always
 * has a zero: subtracting min_v d[v] keeps the differences and the caps and lowers the span.
 *   delays[p][V]  the answer, all -1 if nothing is feasible
 *   info[p][0]    found: 1 or 0
 *   info[p][1]    span, -1 if not found
 *   info[p][2]    total, -1 if not found
 *   rclear[p]     min over pairs of clear[p][q][d[w] - d[u] + D] at the answer; +inf for V = 1, -inf if not found; not written when
 *                 clear is NULL
 * V = 1: found, delay 0, nothing is launched.  D = 0: the only candidate is all zeros.  r > D: nothing is found (a result, not an error).
 * One workgroup per plan set; the spans are searched in ascending order, so a set answered at span m costs (m+1)^V candidates and only a
 * set without a solution costs the whole box (D+1)^V; minima of integers under a total order and one min of doubles: the same bits on
 * every run (conflict_rez_amd/csrc/cfz_delay.inl).
 * cfz_delay_search: a map the caller holds (as cfz_plan_conflicts returned it, or edited: the union of two margins, say).
 * cfz_plan_delays: host tables as cfz_plan_conflicts takes them; the map is computed on the device and searched there, it never comes
 * back to the host, and clear is always given.  cfz_loop_plan_delays: the same on the pool that cfz_loop_init* left on the device (P,
 * V, T its own, cap[P][V] with that P); the loop's state, clock and record are left untouched.  info and rclear may be NULL.
 * Refused before anything is launched: non-positive P or V (T, for cfz_plan_delays), V above CFZ_MAX_NBR+1, D < 0, slack < 0, a cap
 * outside [0, D], NULL count (tables) or delays, (D+1)^V > 2^31 ("search space too large": idx must fit an int, and the bound also limits
 * the time of a set without a solution), what cfz_plan_conflicts / cfz_loop_plan_conflicts refuse.  What needs no handle is checked
 * before the handle is looked at. */
#define CFZ_DELAY_NINFO 3 /* found, span, total */
int cfz_delay_search(cfz_handle *h, int P, int V, int D, const int32_t *count /* [P][npair][2D+1] */, const double *clear /* or NULL */,
                     int slack, const int32_t *cap /* [P][V] or NULL */, int32_t *delays /* [P][V] */, int32_t *info /* [P][3] or NULL */,
                     double *rclear /* [P] or NULL */);
int cfz_plan_delays(cfz_handle *h, int P, int V, int T, const double *tables /* [P][V][T][7] */, int D, double margin, int slack,
                    const int32_t *cap, int32_t *delays, int32_t *info, double *rclear);
int cfz_loop_plan_delays(cfz_handle *h, int D, double margin, int slack, const int32_t *cap, int32_t *delays, int32_t *info, double *rclear);

/* ---- coordination diagrams and hold-point schedules of a plan set ----------------------------------------------------------
 * A start delay lets a vehicle wait at its first sample only.  A plan offers more places to wait: wherever it is at rest (a parking
 * manoeuvre rests at every change of direction) the vehicle can stay as it can at the start.  These calls search, per plan set, for
 * schedules with such waits under which no pair of plans comes within the margin.  Sample-wise only, as the conflict map is.
 * Inputs: tables[P][V][T][7] as above; length[P][V] in [1, T] (NULL: T): vehicle v's plan is its samples 0 .. length-1, its goal sample
 * g_v = length-1, what lies beyond is padding and is never read; hold[P][V][T], bytes, non-zero: the vehicle may stay at that sample
 * for any number of steps.  g_v always counts as holdable; sample 0 only if the caller says so.
 * Blocked.  For pair q = (u, w), u < w, in the audit's order, i < length_u, j < length_w: B_q[i][j] = 1 when the signed distance of the
 * body of u at its sample i and the body of w at its sample j is below the margin (the conflict map's predicate, u's body the first
 * argument everywhere); 0 outside the lengths.  The conflict map's count[p][q][tau] is the sum of B_q along the samples of lag tau.
 * Schedule.  s_v(t), t in [0, H): s_v(0) = 0; s_v(t+1) - s_v(t) in {0, 1}; a step of 0 only where hold[s_v(t)] is set (or at g_v);
 * s_v(H-1) = g_v.  Its arrival a_v is the first t with s_v(t) = g_v, its waits the number of steps of 0 before a_v (a_v - g_v).
 * Conflict-free with slack r >= 0: for every pair, every t in [0, H) and every t' = clamp(t + d, 0, H-1), |d| <= r,
 * B_q[s_u(t)][s_w(t')] = 0 and B_q[s_u(t')][s_w(t)] = 0: the conflict map of the scheduled tables has count 0 at every lag in [-r, r].
 * Prioritised schedule of an order pi (a permutation of the vehicles): for k = 0 .. V-1 vehicle pi_k takes a schedule that is
 * conflict-free with slack r against those of pi_0 .. pi_{k-1}; among those the smallest arrival; among those the pointwise largest one
 * (every sample as early as possible, waits as late as possible; the pointwise maximum of two feasible schedules is feasible).  The
 * order is infeasible if some vehicle has no such schedule within H.
 * Answer per set: over orders[O][V], shared by all sets, the feasible order smallest under (makespan = max a_v, total = sum a_v, index).
 *   schedule[p][V][H]  s_v(t) of the answer, all -1 if no order is feasible ("nothing feasible within the horizon" is a result)
 *   arrival[p][V], waits[p][V]  -1 if not found
 *   info[p][5]    found (1 or 0), order index, makespan, total (-1 if not found), number of feasible orders
 * V = 1: found, arrival g_0, no waits, nothing is launched.
 * cfz_plan_coordination returns the diagrams themselves: blocked[P][npair][T][words], words = (T + 31) / 32 of 32 bits, bit (j & 31) of
 * word j >> 5 of row i is B_q[i][j] (V = 1: nothing is written).  cfz_plan_schedule computes them on the device and searches them there;
 * cfz_loop_plan_schedule does so on the pool that cfz_loop_init* left on the device (P, V, T its own; only length, hold and orders are
 * uploaded); the loop's state, clock and record are left untouched.  arrival, waits and info may be NULL.
 * One workgroup of four wavefronts per set, a wavefront per order; the reachable samples of a vehicle are a row of T bits over the 64
 * lanes, hence T <= CFZ_SCHEDULE_MAX_T; the rows of all H steps are kept for the walk back, in LDS up to 144 KB per workgroup and in
 * global memory beyond.  Integers only: the same outputs on every run (conflict_rez_amd/csrc/cfz_coord.inl, cfz_schedule.inl).
 * Refused before anything is launched: a margin that is negative or not finite, non-positive P, T, H or O, V outside 1..CFZ_MAX_NBR+1,
 * a length outside [1, T], T > CFZ_SCHEDULE_MAX_T, H > CFZ_SCHEDULE_MAX_H, H < T (no room even for a plan without waits), slack < 0,
 * an order that is not a permutation of 0..V-1, NULL tables, hold, orders, schedule or blocked, sizes beyond 2^31 elements (the pool,
 * the diagrams, the schedule) or a workspace beyond 2 GiB.  What needs no handle is checked before the handle is looked at. */
#define CFZ_SCHEDULE_NINFO 5 /* found, order, makespan, total, feasible orders */
#define CFZ_SCHEDULE_MAX_T 2048
#define CFZ_SCHEDULE_MAX_H 32768
int cfz_plan_coordination(cfz_handle *h, int P, int V, int T, const double *tables /* [P][V][T][7] */, const int32_t *length /* [P][V] or NULL */,
                          double margin, uint32_t *blocked /* [P][npair][T][words] */);
int cfz_plan_schedule(cfz_handle *h, int P, int V, int T, const double *tables, const int32_t *length, const uint8_t *hold /* [P][V][T] */,
                      int H, double margin, int slack, int O, const int32_t *orders /* [O][V] */, int32_t *schedule /* [P][V][H] */,
                      int32_t *arrival /* [P][V] or NULL */, int32_t *waits /* [P][V] or NULL */, int32_t *info /* [P][5] or NULL */);
int cfz_loop_plan_schedule(cfz_handle *h, const int32_t *length, const uint8_t *hold, int H, double margin, int slack, int O,
                           const int32_t *orders, int32_t *schedule, int32_t *arrival, int32_t *waits, int32_t *info);

const char *cfz_last_error(void);
/* First 16 hex digits of the SHA-256 over the kernel sources this library was built from (__graft_entry__.source_hash; "unknown" for
 * a build made by hand).  bench.py quotes profiler counters from profiles/ only if they were taken on a library with the same hash. */
const char *cfz_source_hash(void);

#ifdef __cplusplus
}
#endif
#endif /* CONFREZ_HIP_H */
