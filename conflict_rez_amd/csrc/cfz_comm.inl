// cfz_comm.inl -- the lossy prediction exchange of the closed loop (cfz_loop_set_comm / cfz_loop_comm): which of a neighbour's
// predictions a vehicle plans against when messages are lost.  The reference's node keeps whichever VehiclePredictionMsg arrived
// last (ros2_ws/src/confrez_ros/src/vehicle_node.py:154-163), steps on a timer with whatever is there (:171-189), and step()
// advances that message by one stage whatever its age (_adv_onestep, vehicle_follower.py:413-426).  Plain CFZ_CALL functions, as
// cfz_disturb.inl, so that the CPU test build (tests/emu/cfz_comm_emu.cpp) compiles the same source as loop_prep, comm_fill and the
// persistent comm kernels in cfz_engine.hip.
//
// Messages.  In MPC iteration tau (counted since cfz_loop_init*) vehicle u of scenario s publishes its prediction after that
//   iteration, the solution or the shift fallback: message tau, which starts at time tau.
// Delivery.  delivered(s, v <- u, tau) = u1 > p_drop[s], u1 in (0, 1] the first uniform (disturb_uniforms) of the Philox4x32-10 call
//   with key (seed & 0xffffffff, seed >> 32) of the comm seed and counter (stream[s], v, tau + 1, 8 + u); v is the receiver.  Word 3
//   is 8..15 and never meets the noise pairs 0..5 of cfz_disturb.inl, even under an equal seed.  p_drop = 0 delivers everything
//   (u1 > 0), p_drop = 1 nothing (u1 <= 1).
// Want.  In iteration t vehicle v wants message tau* = t - 1 of a neighbour (Jacobi), or tau* = t of a neighbour ranked before it
//   under the sequential exchange, whose prediction of this iteration already exists.
// Age.  v reads message tau* - a, a the smallest a >= 0 with delivered(tau* - a), or a = A_eff = min(max_age, tau* - tau_on): tau_on is
//   the message that stood in `pred` when the setting was made; it counts as delivered, and a message of age max_age always gets
//   through.
// Row.  Stage k of the neighbour's block reads row min(k + fresh + (compensate ? a : 0), N - 1) of that message; fresh = 1 under
//   Jacobi, 0 for a vehicle ranked before: what the lossless loop reads.  compensate = 0 is the reference node (the last message
//   advanced as if it were new), compensate = 1 advances it by its age.
// Ring.  Message tau lives in slot (tau + 1) mod D of ring[D][S * V][7][N], D = max_age + 2: iteration t reads tau in
//   [t - 1 - max_age, t] and writes tau = t, whose slot last held tau = t - D.
#ifndef CFZ_COMM_INL
#define CFZ_COMM_INL

#include "cfz_disturb.inl"

#ifndef CFZ_MAX_AGE
#define CFZ_MAX_AGE 6
#endif

#if defined(__HIPCC__)
#define CFZ_MEMBER __host__ __device__ __forceinline__
#else
#define CFZ_MEMBER inline
#endif

namespace cfz {

constexpr int kCommWord = 8;  // word 3 of a delivery draw's counter is kCommWord + sender

// What the kernels need of a comm setting: device arrays p_drop[S], stream[S] and the ring.  p_drop == nullptr: off.
struct CommArgs {
  uint64_t seed;
  const double *p_drop;
  const uint32_t *stream;
  double *ring;  // [D][S * V][7][N], D = max_age + 2
  int max_age, compensate, tau_on;
  size_t slot_stride;  // S * V * 7 * N, the doubles of one slot
};

CFZ_CALL CommArgs comm_none() { return {0, nullptr, nullptr, nullptr, 0, 0, 0, 0}; }

// the delivery bit of message tau from vehicle u to vehicle v under stream id `stream` and drop rate p
CFZ_CALL bool comm_delivered(uint64_t seed, uint32_t stream, int v, int u, int tau, double p) {
  const uint32_t ctr[4] = {stream, (uint32_t)v, (uint32_t)(tau + 1), (uint32_t)(kCommWord + u)};
  const uint32_t key[2] = {(uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32)};
  uint32_t w[4];
  philox4x32_10(ctr, key, w);
  double u1, u2;
  disturb_uniforms(w, u1, u2);
  return u1 > p;
}

// the message vehicle v wants of a neighbour in iteration t; `earlier`: the neighbour is ranked before v (sequential exchange)
CFZ_CALL int comm_want(int t, bool earlier) { return earlier ? t : t - 1; }

// the age rule over any delivery predicate bit(tau)
template <class Bit> CFZ_CALL int comm_age_of(const Bit &bit, int tau_star, int max_age, int tau_on) {
  const int room = tau_star - tau_on, a_eff = room < max_age ? room : max_age;
  int a = 0;
  while (a < a_eff && !bit(tau_star - a)) ++a;
  return a;
}

struct CommDraw {  // the predicate of the loop: the draws of (scenario, receiver, sender)
  uint64_t seed; uint32_t stream; int v, u; double p;
  CFZ_MEMBER bool operator()(int tau) const { return comm_delivered(seed, stream, v, u, tau, p); }
};

// the age of what vehicle v of scenario s reads of vehicle u when it wants message tau_star
CFZ_CALL int comm_age(const CommArgs &cm, int s, int v, int u, int tau_star) {
  const CommDraw draw = {cm.seed, cm.stream[s], v, u, cm.p_drop[s]};
  return comm_age_of(draw, tau_star, cm.max_age, cm.tau_on);
}

CFZ_CALL int comm_slot(int tau, int max_age) { return (tau + 1) % (max_age + 2); }

// the row of the message that stage k reads
CFZ_CALL int comm_row(int k, int fresh, int compensate, int a, int N) {
  const int r = k + fresh + (compensate ? a : 0);
  return r < N - 1 ? r : N - 1;
}

}  // namespace cfz
#endif  // CFZ_COMM_INL
