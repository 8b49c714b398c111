// cfz_loop_body.inl -- the body of the persistent closed-loop kernels loop_kernel, loop_kernel_seq, their disturbed variants
// loop_kernel_dist, loop_kernel_seq_dist, the lossy-exchange variants loop_kernel_comm, loop_kernel_seq_comm and the problem-pool variants
// loop_kernel_pool, loop_kernel_seq_pool, loop_kernel_pool_comm, loop_kernel_seq_pool_comm (cfz_engine.hip), included inside all ten.  The including kernel defines `constexpr bool kSeq` and the exchange order arrays `xperm`, `xrank`
// (nullptr for the Jacobi kernels), `constexpr bool kDist` and the disturbance setting `dz` with the step count `step0` (unused
// constants in the undisturbed kernels), `constexpr bool kComm` and the comm setting `cm` (an unused constant in the kernels
// without it), `constexpr bool kPool`, the pool of problems `pool`, `problem_of` of cfz_loop_set_problems (nullptr constants in the
// kernels without it) and `dz_clip`, whether a disturbance is set and the applied input is therefore clipped to the problem's input box
// (the pool kernels' argument; true in the others, which run only under a setting that clips); everything else is the kernel's arguments.
  extern __shared__ double smem[];
  const cfz::KSpec &sp = ka->sp; const cfz::KDer &dv = ka->dv; const cfz::Lay &L = ka->L;
  const int N = sp.N, nn = sp.n_nbr, B = S * V, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  double *my = scratch + (size_t)blockIdx.x * (5 + 3 * N + nn * 3 * N + 7 * N);
  double *ref = my + 5;  // (the record keeps the layout x0 | ref | nbr | zu of the stepwise path; only ref is used here)
  double *dn = ref + 3 * N;  // kDist: d[5:12] of the item in hand, kept from the parameter phase to the plant in the idle nbr | zu slots
  int32_t *head = qbuf, *tail = qbuf + K, *slots = qbuf + 2 * K;
  // what wavefront 0 popped, for wavefront 1: {iteration t (-1: leave), instance b, whether the item runs at raised issue priority}.
  // Lives in the reduction exchange area of the workspace, which is idle between two solves.
  volatile int32_t *cmd = reinterpret_cast<volatile int32_t *>(smem + L.xw);
#define CFZ_LD(p) __builtin_amdgcn_readfirstlane(__hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
  int idle = 0;
  while (true) {
    if (wave == 0) {
      // ---- pop (wavefront 0 only): lowest iteration first -----------------------------------------------
      int t = -1, b = -1, idx = 0;
      while (true) {
        int t0 = CFZ_LD(&ctrl[0]);
        const int hint = t0;
        while (t0 < K && CFZ_LD(&head[t0]) >= B) ++t0;
        if (t0 > hint && lane == 0) atomicMax(&ctrl[0], t0);
        if (t0 >= K) break;  // every item of every iteration has been handed out
        for (int tt = t0; tt < K; ++tt) {
          const int hd = CFZ_LD(&head[tt]), tl = CFZ_LD(&tail[tt]);
          if (tl == 0) break;  // no scenario has reached iteration tt yet, hence none is further either
          if (hd >= tl) continue;
          idx = __builtin_amdgcn_readfirstlane(atomicAdd(&head[tt], lane == 0 ? 1 : 0));
          if (idx < B) { t = tt; break; }
        }
        if (t < 0) {  // nothing to hand out right now
          __builtin_amdgcn_s_sleep(32);
          if (++idle > (1 << 22) || CFZ_LD(&ctrl[2])) { if (lane == 0) atomicExch(&ctrl[2], 1); break; }
          continue;
        }
        idle = 0;
        for (int spins = 0; (b = CFZ_LD(&slots[(size_t)t * B + idx])) < 0; ++spins) {
          __builtin_amdgcn_s_sleep(8);
          if (spins > (1 << 23) || CFZ_LD(&ctrl[2])) break;
        }
        if (b < 0) { if (lane == 0) atomicExch(&ctrl[2], 1); t = -1; }
        break;
      }
      CFZ_MARK(1);
      // acquire: predictions / states written by other workgroups.  One agent-scope acquire by the polling wavefront
      // (invalidates this CU's L1), completed before the barrier that releases the other wavefront's loads.
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      // The launch ends with its slowest scenario (a chain of K dependent iterations).  An item of the oldest open iteration
      // (prio_lag >= 0: t <= ctrl[0] + prio_lag) that also sits among the last prio_tail positions of its iteration's queue
      // (prio_tail > 0, t >= 1) belongs to a scenario that is behind: items are published in the order in which their scenarios
      // finished the iteration before, under either exchange rule.  Iteration 0 was queued by the host in index order, which says
      // nothing, so there the iteration decides alone; B < prio_tail: every position qualifies.  Decided here, by the wavefront that
      // holds the position, from scalars only.
      int pr = 0;
      if (prio_lag >= 0 && t >= 0) pr = (t <= CFZ_LD(&ctrl[0]) + prio_lag && (prio_tail <= 0 || t == 0 || idx >= B - prio_tail)) ? 1 : 0;
      if (lane == 0) { cmd[0] = t; cmd[1] = b; cmd[2] = pr; }
    }
    __syncthreads();
    // the item through readfirstlane: the same in every lane, and known to the compiler as such.  s_setprio ignores EXEC; under a
    // condition read from (volatile) LDS the raise sat in an EXEC-masked region and ran in every wavefront, followed by the lowering.
    const int t = __builtin_amdgcn_readfirstlane(cmd[0]), b = __builtin_amdgcn_readfirstlane(cmd[1]);
    if (t < 0) break;
    const int pr = __builtin_amdgcn_readfirstlane(cmd[2]);
    CFZ_MARK(2);
    CFZ_ITEM_STAMP(0, pr);
    // Both wavefronts of a prioritised item take issue priority over the wavefronts they share their SIMDs with (VALU issue is
    // arbitrated by priority, then age), the others give way.  Lowered again below, after the hand-off.
    if (pr) __builtin_amdgcn_s_setprio(3);
    const int s = b / V, v = b - s * V;
    // kPool: the constants of the scenario's problem, pool[problem_of[s]], in place of the handle's block; the index is the same in
    // every lane of both wavefronts, so the block is still read through scalar loads.  N, n_nbr and the layout L stay the handle's.
    const KArgs *const kp = kPool ? pool + __builtin_amdgcn_readfirstlane(problem_of[s]) : ka;
    const cfz::KSpec &spi = kPool ? kp->sp : sp;
    const cfz::KDer &dvi = kPool ? kp->dv : dv;
    // kComm: the ring of messages indexed by the absolute iteration instead of the parity pair (cfz_comm.inl)
    const double *pin = kComm ? cm.ring + (size_t)cfz::comm_slot(step0 + t - 1, cm.max_age) * cm.slot_stride
                              : pred + (size_t)(t & 1) * B * 7 * N;   // predictions after iteration t-1
    double *pout = kComm ? cm.ring + (size_t)cfz::comm_slot(step0 + t, cm.max_age) * cm.slot_stride : pred + (size_t)((t + 1) & 1) * B * 7 * N;
    const double *tab = ref_table + (size_t)table_of[s] * V * T * 7;
    const int rv = kSeq ? xrank[b] : 0;  // v's rank in its scenario's exchange order
    // kComm: the age of what v reads of each neighbour, three bits each in neighbour order.  Every thread makes the at most
    // (V - 1) * max_age draws itself (they depend on the item alone), so the ages need no LDS; the value is wavefront-uniform.
    uint32_t ages = 0;
    if (kComm) {
      int o = 0;
      for (int u = 0; u < V; ++u) {
        if (u == v) continue;
        const bool cur = kSeq && xrank[s * V + u] < rv;
        ages |= (uint32_t)cfz::comm_age(cm, s, v, u, cfz::comm_want(step0 + t, cur)) << (3 * o);
        ++o;
      }
      ages = __builtin_amdgcn_readfirstlane(ages);
    }
    // ---- parameters and shifted warm start (vehicle_follower.py:432-476), straight into the solver's workspace: measured
    // state, neighbours' poses with cos / sin, warm start (solve_instance's `preloaded` form); only the reference goes through
    // a global record (the solver reads it from there in every iteration)
    if (!kDist) {
      if (tid < 5) smem[L.x0 + tid] = state[b * 5 + tid];
    } else if (tid < cfz::kDisturbN) {
      // twelve lanes, one Philox call each: the measurement state + d[0:5] is what the solver is pinned to; d[5:12] wait for the plant
      const double d = cfz::disturb_value(dz, s, v, step0 + t, tid);
      if (tid < 5) smem[L.x0 + tid] = cfz::disturb_add(state[b * 5 + tid], d);
      else dn[tid - 5] = d;
    }
    for (int k = tid; k < N; k += cfz::kNL) {
      const int ka = (k + 1 < N) ? k + 1 : N - 1;
      int kr = kidx0[s] + t_base + t + k; if (kr > T - 1) kr = T - 1;
      for (int c = 0; c < 3; ++c) ref[c * N + k] = tab[((size_t)v * T + kr) * 7 + c];
      for (int c = 0; c < 7; ++c) smem[L.p + k * cfz::kNP + c] = pin[((size_t)b * 7 + c) * N + ka];
      int o = 0;
      for (int u = 0; u < V; ++u) {
        if (u == v) continue;
        const size_t bo = (size_t)s * V + u;
        double *q = smem + L.nb4 + (k * nn + o) * 4;
        const bool cur = kSeq && xrank[bo] < rv;  // ranked before v: its prediction of this iteration, not advanced
        const double *pu = cur ? pout : pin;
        int ku = cur ? k : ka;
        if (kComm) {  // the message the age rule gives, at the row of cfz_comm.inl (age 0: the slot and the row above)
          const int a = (ages >> (3 * o)) & 7;
          pu = cm.ring + (size_t)cfz::comm_slot(cfz::comm_want(step0 + t, cur) - a, cm.max_age) * cm.slot_stride;
          ku = cfz::comm_row(k, cur ? 0 : 1, cm.compensate, a, N);
        }
        const double po = pu[(bo * 7 + 2) * N + ku];
        q[0] = pu[(bo * 7 + 0) * N + ku]; q[1] = pu[(bo * 7 + 1) * N + ku]; q[2] = cos(po); q[3] = sin(po);
        ++o;
      }
    }
    __syncthreads();
    CFZ_MARK(3);
    CFZ_ITEM_STAMP(1, 0);
    int oi[2]; double od[3];
    cfz::DualOut duo = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    cfz::solve_instance<true>(spi, dvi, nullptr, ref, nullptr, nullptr, smem, L, oi, od, duo, wst ? wst + (size_t)b * wst_stride : nullptr, 1, 2);
    __syncthreads();
    CFZ_MARK(4);
    CFZ_ITEM_STAMP(2, 0);
    // ---- read-back (the solution is still in the workspace) or shift fallback (:484-524), plant (:528-543) ------------
    for (int i = tid; i < 7 * N; i += cfz::kNL) {
      const int c = i / N, k = i - c * N;
      const int ka = (k + 1 < N) ? k + 1 : N - 1;
      cfz::store_shared(pout + (size_t)b * 7 * N + i, (oi[1] == 0) ? smem[L.p + k * cfz::kNP + c] : pin[((size_t)b * 7 + c) * N + ka]);
    }
    CFZ_MARK(5);
    if (tid == 0) {
      double a0 = (oi[1] == 0) ? smem[L.p + 5] : pin[((size_t)b * 7 + 5) * N + 1];
      double w0 = (oi[1] == 0) ? smem[L.p + 6] : pin[((size_t)b * 7 + 6) * N + 1];
      double z[5], out[5];
      if (!kDist) {
        for (int i = 0; i < 5; ++i) z[i] = smem[L.x0 + i];
      } else {  // the plant starts from the true state (x0 holds the measurement) with the disturbed, clipped input
        for (int i = 0; i < 5; ++i) z[i] = state[b * 5 + i];
        if (!kPool || dz_clip) {
          a0 = cfz::disturb_clip(cfz::disturb_add(a0, dn[0]), spi.bounds[8], spi.bounds[9]);
          w0 = cfz::disturb_clip(cfz::disturb_add(w0, dn[1]), spi.bounds[10], spi.bounds[11]);
        } else {  // a pool kernel standing in for the undisturbed one: no disturbance is set, so nothing is clipped either
          a0 = cfz::disturb_add(a0, dn[0]); w0 = cfz::disturb_add(w0, dn[1]);
        }
      }
      cfz::rk4_step<false>(z, a0, w0, sp.dt, sp.wb, kPlantSubsteps, out, nullptr);
      if (kDist)
        for (int i = 0; i < 5; ++i) out[i] = cfz::disturb_add(out[i], dn[2 + i]);
      for (int i = 0; i < 5; ++i) cfz::store_shared(state + b * 5 + i, out[i]);
      // status, iters and stats are read after the launch only, but every iteration of the launch rewrites them, from another XCD as a
      // rule: written through as well, or an older iteration's dirty line, written back later, would overwrite the newer value
      cfz::store_shared(status + b, (int32_t)oi[1]); cfz::store_shared(iters + b, (int32_t)oi[0]);
      if (rec) {
        double *r = rec + ((size_t)t * B + b) * 7;
        for (int i = 0; i < 5; ++i) r[i] = out[i];
        r[5] = a0; r[6] = w0;
        rec_si[(size_t)t * 2 * B + b] = oi[1]; rec_si[(size_t)(t * 2 + 1) * B + b] = oi[0];
      }
      for (int i = 0; i < 3; ++i) cfz::store_shared(stats + b * 3 + i, od[i]);
      atomicAdd(iter_sum, oi[0]);
      if (oi[1] == 0) atomicAdd(iter_sum + 1, 1);  // converged solves of this launch
      atomicAdd(iter_sum + 2 + (oi[1] < 0 ? 0 : (oi[1] > 5 ? 5 : oi[1])), 1);  // ... and how every solve of it ended (status 0..5)
    }
    // release: prediction, state and carry record of (s, v, t), the three things another workgroup reads in this launch, were stored
    // write-through (cfz::store_shared), so no write-back of the XCD's L2 is needed -- it would sweep out every resident workgroup's
    // spill frames with them.  Every storing wavefront waits for its stores (the asm wait: the compiler does not count on it and
    // cannot drop it), the workgroup meets, and only then one lane signals, by atomics.  rec and rec_si are written once per item and
    // read after the launch: plain stores.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    CFZ_MARK(6);
    if (tid == 0) {
      const int c = atomicAdd(&done[s], 1);
      if (kSeq) {  // completions of a scenario are serialised: c % V is this item's rank; publish exactly one item
        const int r = c % V;
        const int tn = r < V - 1 ? t : t + 1;
        if (tn < K) {
          const int pos = atomicAdd(&tail[tn], 1);
          __hip_atomic_store(&slots[(size_t)tn * B + pos], s * V + xperm[s * V + (r < V - 1 ? r + 1 : 0)], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
        }
      } else if ((c % V) == V - 1 && t + 1 < K) {  // last vehicle of the scenario: publish iteration t+1
        const int pos = atomicAdd(&tail[t + 1], V);
        for (int u = 0; u < V; ++u)
          __hip_atomic_store(&slots[(size_t)(t + 1) * B + pos + u], s * V + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      atomicAdd(&ctrl[1], 1);
    }
    // the priority ends with the item: neither the pop loop of wavefront 0 nor wavefront 1's wait at the barrier holds it
    if (pr) __builtin_amdgcn_s_setprio(0);
    CFZ_ITEM_STAMP(3, 0);
    CFZ_MARK(8);
  }
  CFZ_MARK(9);
#undef CFZ_LD
