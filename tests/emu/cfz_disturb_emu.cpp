// Test-only CPU build of the closed loop's disturbance streams: conflict_rez_amd/csrc/cfz_disturb.inl compiled with g++
// (-ffp-contract=off).  Never shipped, never loaded by the package.
#include "../../conflict_rez_amd/csrc/cfz_disturb.inl"

extern "C" {

void cfz_emu_philox(const uint32_t *ctr, const uint32_t *key, uint32_t *out) { cfz::philox4x32_10(ctr, key, out); }

// the two normals of four given words
void cfz_emu_box_muller(const uint32_t *w, double *z) { cfz::disturb_box_muller(w, z); }

// n draws: seed[n], stream[n], v[n], step[n] -> words[n][6][4], z[n][12]
void cfz_emu_normals(long n, const uint64_t *seed, const uint32_t *stream, const uint32_t *v, const uint32_t *step, uint32_t *words,
                     double *z) {
  for (long i = 0; i < n; ++i)
    for (uint32_t j = 0; j < 6; ++j) {
      const uint32_t ctr[4] = {stream[i], v[i], step[i], j}, key[2] = {(uint32_t)(seed[i] & 0xffffffffu), (uint32_t)(seed[i] >> 32)};
      cfz::philox4x32_10(ctr, key, words + (i * 6 + j) * 4);
      cfz::disturb_pair(seed[i], stream[i], v[i], step[i], j, z + i * 12 + 2 * j);
    }
}

// d[K][S][V][12] of steps [t0, t0 + K) as the device's disturb_fill forms it (sigma[12], level[S], stream[S])
void cfz_emu_disturbance(uint64_t seed, const double *sigma, const double *level, const uint32_t *stream, int S, int V, int t0, int K,
                         double *d) {
  const cfz::DisturbArgs dz = {seed, sigma, level, stream};
  for (int k = 0; k < K; ++k)
    for (int s = 0; s < S; ++s)
      for (int v = 0; v < V; ++v)
        for (int i = 0; i < cfz::kDisturbN; ++i) d[(((long)k * S + s) * V + v) * cfz::kDisturbN + i] = cfz::disturb_value(dz, s, v, t0 + k, i);
}

double cfz_emu_disturb_add(double x, double d) { return cfz::disturb_add(x, d); }
}
