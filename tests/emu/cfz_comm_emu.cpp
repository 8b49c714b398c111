// Test-only CPU build of the closed loop's lossy exchange: conflict_rez_amd/csrc/cfz_comm.inl compiled with g++.  Never shipped,
// never loaded by the package.
#include "../../conflict_rez_amd/csrc/cfz_comm.inl"

namespace {
struct ArrayBit {  // bits[0 .. n) of messages base .. base + n - 1
  const int32_t *bits; int base;
  bool operator()(int tau) const { return bits[tau - base] != 0; }
};
}  // namespace

extern "C" {

int cfz_emu_max_age(void) { return CFZ_MAX_AGE; }

// n delivery bits: seed[n], stream[n], v[n] (receiver), u[n] (sender), tau[n], p[n] -> bit[n], ctr[n][4] (the Philox counter drawn from)
void cfz_emu_delivered(long n, const uint64_t *seed, const uint32_t *stream, const int32_t *v, const int32_t *u, const int32_t *tau,
                       const double *p, int32_t *bit, uint32_t *ctr) {
  for (long i = 0; i < n; ++i) {
    bit[i] = cfz::comm_delivered(seed[i], stream[i], v[i], u[i], tau[i], p[i]) ? 1 : 0;
    ctr[i * 4] = stream[i]; ctr[i * 4 + 1] = (uint32_t)v[i]; ctr[i * 4 + 2] = (uint32_t)(tau[i] + 1); ctr[i * 4 + 3] = (uint32_t)(cfz::kCommWord + u[i]);
  }
}

// delivered[K][S][V][V] of messages [tau0, tau0 + K) as the device's comm_fill forms it
void cfz_emu_comm(uint64_t seed, const double *p_drop, const uint32_t *stream, int S, int V, int tau0, int K, int32_t *delivered) {
  for (int k = 0; k < K; ++k)
    for (int s = 0; s < S; ++s)
      for (int v = 0; v < V; ++v)
        for (int u = 0; u < V; ++u)
          delivered[(((long)k * S + s) * V + v) * V + u] = u == v ? 1 : (cfz::comm_delivered(seed, stream[s], v, u, tau0 + k, p_drop[s]) ? 1 : 0);
}

// the age rule over given bits: bits[i] is the delivery bit of message base + i
int cfz_emu_age(const int32_t *bits, int base, int tau_star, int max_age, int tau_on) {
  const ArrayBit b = {bits, base};
  return cfz::comm_age_of(b, tau_star, max_age, tau_on);
}

// the age rule over the loop's own draws
int cfz_emu_age_drawn(uint64_t seed, const double *p_drop, const uint32_t *stream, int max_age, int tau_on, int s, int v, int u, int tau_star) {
  const cfz::CommArgs cm = {seed, p_drop, stream, nullptr, max_age, 0, tau_on, 0};
  return cfz::comm_age(cm, s, v, u, tau_star);
}

int cfz_emu_want(int t, int earlier) { return cfz::comm_want(t, earlier != 0); }
int cfz_emu_slot(int tau, int max_age) { return cfz::comm_slot(tau, max_age); }
int cfz_emu_row(int k, int fresh, int compensate, int a, int N) { return cfz::comm_row(k, fresh, compensate, a, N); }
}
