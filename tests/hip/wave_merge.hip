// tests/test_wave_merge_gpu.py: the device forms of conflict_rez_amd/csrc/cfz_wave.inl alone, one workgroup of one wavefront.
//   wave_merge <in> <out>
// in:  WaveCase[64], WaveSpan[64], the value of every lane (raw structs of tests/hip/wave_merge_case.h).
// out: WaveCase[6][64]  wave_xor at off = 1, 2, 4, 8, 16, 32;  WaveCase[64]  the commutative butterfly (case_min) at width 64;
//      WaveSpan[7][64]  the ordered butterfly (span_concat) at group widths 1, 2, 4, 8, 16, 32, 64; every lane's result.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../conflict_rez_amd/csrc/cfz_wave.inl"
#include "wave_merge_case.h"

static void die(const char *what) { fprintf(stderr, "wave_merge: %s\n", what); exit(1); }
#define CHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) die(hipGetErrorString(e_)); } while (0)

constexpr int kLanes = 64, kXor = 6, kWidths = 7;

__global__ __launch_bounds__(kLanes) void wave_kernel(const WaveCase *c, const WaveSpan *s, WaveCase *xo, WaveCase *mo, WaveSpan *oo) {
  const int lane = threadIdx.x;
  const WaveCase mine = c[lane];
  for (int k = 0; k < kXor; ++k) xo[k * kLanes + lane] = cfz::wave_xor(mine, 1 << k);
  WaveCase m = mine;
  cfz::wave_merge<WaveCase, case_min>(m, kLanes);
  mo[lane] = m;
  for (int k = 0; k < kWidths; ++k) {
    WaveSpan a = s[lane];
    cfz::wave_merge_ordered<WaveSpan, span_concat>(a, lane, 1 << k);
    oo[k * kLanes + lane] = a;
  }
}

int main(int argc, char **argv) {
  if (argc != 3) die("usage: wave_merge <in> <out>");
  std::vector<WaveCase> c(kLanes), xo(kXor * kLanes), mo(kLanes);
  std::vector<WaveSpan> s(kLanes), oo(kWidths * kLanes);
  FILE *fi = fopen(argv[1], "rb");
  if (!fi || fread(c.data(), sizeof(WaveCase), kLanes, fi) != kLanes || fread(s.data(), sizeof(WaveSpan), kLanes, fi) != kLanes) die("short input");
  fclose(fi);
  WaveCase *dc, *dxo, *dmo;
  WaveSpan *ds, *doo;
  CHECK(hipMalloc((void **)&dc, c.size() * sizeof(WaveCase))); CHECK(hipMalloc((void **)&dxo, xo.size() * sizeof(WaveCase)));
  CHECK(hipMalloc((void **)&dmo, mo.size() * sizeof(WaveCase)));
  CHECK(hipMalloc((void **)&ds, s.size() * sizeof(WaveSpan))); CHECK(hipMalloc((void **)&doo, oo.size() * sizeof(WaveSpan)));
  CHECK(hipMemcpy(dc, c.data(), c.size() * sizeof(WaveCase), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(ds, s.data(), s.size() * sizeof(WaveSpan), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(wave_kernel, dim3(1), dim3(kLanes), 0, 0, dc, ds, dxo, dmo, doo);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(xo.data(), dxo, xo.size() * sizeof(WaveCase), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(mo.data(), dmo, mo.size() * sizeof(WaveCase), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(oo.data(), doo, oo.size() * sizeof(WaveSpan), hipMemcpyDeviceToHost));
  FILE *fo = fopen(argv[2], "wb");
  if (!fo || fwrite(xo.data(), sizeof(WaveCase), xo.size(), fo) != xo.size() || fwrite(mo.data(), sizeof(WaveCase), mo.size(), fo) != mo.size() ||
      fwrite(oo.data(), sizeof(WaveSpan), oo.size(), fo) != oo.size() || fclose(fo) != 0)
    die("cannot write the output");
  return 0;
}
