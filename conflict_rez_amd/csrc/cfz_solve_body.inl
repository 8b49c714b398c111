// cfz_solve_body.inl -- the body of solve_kernel and solve_kernel_pool (cfz_engine.hip), included inside both.  The including kernel
// defines `constexpr bool kPool` and, for the kernel without a pool, the constants `pool`, `problem_of` (nullptr) and `V`.
  extern __shared__ double smem[];
  if ((int)blockIdx.x >= B) return;
  // workgroups are dispatched in index order: `order` puts the instances expected to run longest first
  const int b = order ? order[blockIdx.x] : (int)blockIdx.x;
  // kPool: the spec and the derived constants of the scenario's problem; N, n_obs, n_nbr and the layout stay the handle's
  const KArgs *const kp = kPool ? pool + __builtin_amdgcn_readfirstlane(problem_of[b / V]) : ka;
  const cfz::KSpec &sp = kp->sp; const cfz::KDer &dv = kp->dv; const cfz::Lay &L = ka->L;
  const int N = ka->sp.N, no = ka->sp.n_obs, nn = ka->sp.n_nbr;
  int oi[2]; double od[3];
  cfz::DualOut duo = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
#ifdef CFZ_STAMPS
  duo.stamps = reinterpret_cast<unsigned long long *>(stats) + (size_t)B * 3 + (size_t)b * 24;  // diagnostic build: stats has room
#endif
  if (du.l) {
    duo.l = du.l + (size_t)b * N * 4 * no; duo.mm = du.m + (size_t)b * N * 4 * no;
    duo.lam_ij = du.lam_ij + (size_t)b * nn * N * 4; duo.lam_ji = du.lam_ji + (size_t)b * nn * N * 4;
    duo.s = du.s + (size_t)b * nn * N * 2;
  }
  // carry record of the instance's slot (default: slot b): used when the caller says that this solve is the successor of
  // the previous one in that slot
  const int slot = slots ? slots[b] : b;
  cfz::solve_instance(sp, dv, x0 + (size_t)b * 5, ref + (size_t)b * 3 * N, nbr + (size_t)b * nn * 3 * N,
                      zu + (size_t)b * 7 * N, smem, L, oi, od, duo, wst ? wst + (size_t)slot * wst_stride : nullptr,
                      carry_all || (carry && carry[b]));
  if (threadIdx.x == 0) {
    iters[b] = oi[0]; status[b] = oi[1];
    stats[b * 3 + 0] = od[0]; stats[b * 3 + 1] = od[1]; stats[b * 3 + 2] = od[2];
  }
