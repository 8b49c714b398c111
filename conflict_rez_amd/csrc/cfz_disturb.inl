// cfz_disturb.inl -- the disturbance streams of the closed loop (cfz_loop_set_disturbance / cfz_loop_disturbance): measurement,
// actuator and process noise drawn from a counter-based generator inside the kernels that own the state, so that no noise is
// stored or uploaded and the stepwise loop, the persistent loop and a host replay see the same variates word for word.
// Plain CFZ_CALL functions, so that the CPU test build (tests/emu/cfz_disturb_emu.cpp) compiles the same source as loop_prep,
// loop_post, disturb_fill and the disturbed persistent kernels in cfz_engine.hip.  The reference has no such model: it runs the
// follower against its integrator with the exact state (vehicle_follower.py:194-199, :528-543) and on vehicles.
//
// Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123), integer arithmetic only.
//   key      (seed & 0xffffffff, seed >> 32) of the user's 64-bit seed
//   counter  (stream_s, v, step, j): the scenario's stream id, the vehicle, the MPC iteration since cfz_loop_init* and the pair 0..5
// The four output words w0..w3 of one call give two standard normals by Box-Muller in double:
//   u1 = (((w0 >> 5) << 26) + (w1 >> 6) + 1) * 2^-53  in (0, 1]      u2 = (((w2 >> 5) << 26) + (w3 >> 6)) * 2^-53  in [0, 1)
//   r = sqrt(-2 log u1),  z[2j] = r cos(2 pi u2),  z[2j+1] = r sin(2 pi u2)
// The twelve variates of one (scenario, vehicle, step): z[0:5] measurement noise on x, y, psi, v, delta; z[5:7] actuator noise on
// a, w; z[7:12] process noise on x, y, psi, v, delta.  The disturbance d[i] = level_s * sigma[i] * z[i] is a rounded value of its own
// and is added by one plain rounded addition (disturb_add): neither is contracted into a fused multiply-add, whatever the
// translation unit's -ffp-contract says, so a host that downloads d (cfz_loop_disturbance) replays the loop with exact inputs.
#ifndef CFZ_DISTURB_INL
#define CFZ_DISTURB_INL

#include <math.h>
#include <stdint.h>

#ifndef CFZ_CALL
#if defined(__HIPCC__)
#define CFZ_CALL __host__ __device__ __forceinline__
#else
#define CFZ_CALL static inline
#endif
#endif

#if defined(__clang__)
#define CFZ_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CFZ_NO_CONTRACT  // g++: the test build passes -ffp-contract=off
#endif

namespace cfz {

constexpr int kDisturbN = 12;  // variates of one (scenario, vehicle, step): 5 measurement, 2 actuator, 5 process

// What the kernels need of a disturbance setting: device arrays sigma[12], level[S], stream[S].  sigma == nullptr: off.
struct DisturbArgs {
  uint64_t seed;
  const double *sigma, *level;
  const uint32_t *stream;
};

CFZ_CALL DisturbArgs disturb_none() { return {0, nullptr, nullptr, nullptr}; }

CFZ_CALL uint32_t disturb_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

CFZ_CALL void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = disturb_mulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = disturb_mulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the two uniforms of four words: 53 bits each, u1 never 0
CFZ_CALL void disturb_uniforms(const uint32_t w[4], double &u1, double &u2) {
  const double p53 = 1.0 / 9007199254740992.0;  // 2^-53
  u1 = (double)((((uint64_t)(w[0] >> 5)) << 26) + (uint64_t)(w[1] >> 6) + 1u) * p53;
  u2 = (double)((((uint64_t)(w[2] >> 5)) << 26) + (uint64_t)(w[3] >> 6)) * p53;
}

// Box-Muller: two standard normals of four words (products only: nothing here can be contracted)
CFZ_CALL void disturb_box_muller(const uint32_t w[4], double z[2]) {
  double u1, u2;
  disturb_uniforms(w, u1, u2);
  const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586476925286766559 * u2;
  z[0] = r * cos(a); z[1] = r * sin(a);
}

// pair j of (seed, stream, v, step): the normals z[2j], z[2j+1]
CFZ_CALL void disturb_pair(uint64_t seed, uint32_t stream, uint32_t v, uint32_t step, uint32_t j, double z[2]) {
  const uint32_t ctr[4] = {stream, v, step, j}, key[2] = {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)};
  uint32_t w[4];
  philox4x32_10(ctr, key, w);
  disturb_box_muller(w, z);
}

// d = level * sigma * z, rounded after each product
CFZ_CALL double disturb_scale(double level, double sigma, double z) {
  CFZ_NO_CONTRACT
  const double ls = level * sigma;
  return ls * z;
}

// x + d in one rounded addition of its own
CFZ_CALL double disturb_add(double x, double d) {
  CFZ_NO_CONTRACT
  return x + d;
}

CFZ_CALL double disturb_clip(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }

// d[i] of scenario s, vehicle v at `step`, i in 0..11: every kernel forms every disturbance through this one function
CFZ_CALL double disturb_value(const DisturbArgs &dz, int s, int v, int step, int i) {
  double z[2];
  disturb_pair(dz.seed, dz.stream[s], (uint32_t)v, (uint32_t)step, (uint32_t)(i >> 1), z);
  return disturb_scale(dz.level[s], dz.sigma[i], (i & 1) ? z[1] : z[0]);
}

}  // namespace cfz
#endif  // CFZ_DISTURB_INL
