// probe_gfx950.hip — TEST INFRASTRUCTURE: the probes of probe_body.hpp on the device backend (wave_gfx950.hpp).
// One kernel per probe, one workgroup = one wavefront = one case, the power table in 2 KiB-aligned dynamic LDS as in
// k_step.  Builds tests/libsf_wave_probe.so with the product's flags (tests/wave_probe_lib.py); never part of the product.
//
// Every launcher takes the HOST's arrays (PArgs with host pointers and the byte sizes in PSizes), copies them to the
// device, launches, waits and copies every array back: the tests see inputs, results and sentinels alike.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../strikeforce_amd/csrc/wave_gfx950.hpp"
// clang-format off
#include "../../strikeforce_amd/csrc/sf_core.hpp"
#include "../../strikeforce_amd/csrc/sf_host.hpp"
#include "probe_body.hpp"
// clang-format on

namespace sfp {

struct DevIO {
  static constexpr bool DEVICE = true;
  static __device__ __forceinline__ uint32_t ld(const uint32_t *r) { return r[threadIdx.x]; }
  static __device__ __forceinline__ void st(uint32_t *r, uint32_t v) { r[threadIdx.x] = v; }
  static __device__ __forceinline__ void stp(uint32_t *r, bool p) { r[threadIdx.x] = p ? 1u : 0u; }
  static __device__ __forceinline__ void stu(uint32_t *p, uint32_t v) {
    if (threadIdx.x == 0) *p = v;
  }
};
using PD = Probes<sf::WaveGfx950, DevIO>;

// the case's LDS: [power table][its region, from the image in HBM and back to it]
static __device__ __forceinline__ void lds_in(const PArgs &a, uint8_t *lds) {
  uint32_t *w = (uint32_t *)lds;
  for (uint32_t i = threadIdx.x; i < XT_BYTES / 4u; i += 64u) w[i] = a.exptab[i];
  const uint32_t *img = (const uint32_t *)(a.limg + (size_t)blockIdx.x * a.l_stride);
  for (uint32_t i = threadIdx.x; i < a.l_stride / 4u; i += 64u) w[XT_BYTES / 4u + i] = img[i];
  __syncthreads();
}
static __device__ __forceinline__ void lds_out(const PArgs &a, const uint8_t *lds) {
  __syncthreads();
  const uint32_t *w = (const uint32_t *)lds;
  uint32_t *img = (uint32_t *)(a.limg + (size_t)blockIdx.x * a.l_stride);
  for (uint32_t i = threadIdx.x; i < a.l_stride / 4u; i += 64u) img[i] = w[XT_BYTES / 4u + i];
}

#define X(name)                                                           \
  __global__ __launch_bounds__(64) void k_probe_##name(PArgs a) {         \
    extern __shared__ __attribute__((aligned(2048))) uint8_t lds[];       \
    lds_in(a, lds);                                                       \
    PD::name(a, blockIdx.x, lds);                                         \
    lds_out(a, lds);                                                      \
  }
SFP_PROBES(X)
#undef X

// byte sizes of the arrays of a PArgs, in the order of `slots` below (0 = not used, the pointer is passed on as null)
struct PSizes {
  uint64_t in[4], s[4], out[3], so, g, limg, rng, rng2, scal;
};

struct Tables {
  uint16_t *logt = nullptr;
  uint32_t *exptab = nullptr;
};
static int tables(Tables &t) {
  static Tables d;
  if (!d.logt) {
    std::vector<uint16_t> logt(sf::LOGT_ENTRIES, 0);
    std::vector<uint32_t> exptab(512);
    sf::build_rng_tables(logt.data(), exptab.data());
    if (hipMalloc(&d.logt, logt.size() * 2) != hipSuccess || hipMalloc(&d.exptab, 512 * 4) != hipSuccess) return 1;
    if (hipMemcpy(d.logt, logt.data(), logt.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return 1;
    if (hipMemcpy(d.exptab, exptab.data(), 512 * 4, hipMemcpyHostToDevice) != hipSuccess) return 1;
  }
  t = d;
  return 0;
}

typedef void (*Kernel)(PArgs);
static int run(Kernel k, const PArgs &h, const PSizes &z) {
  if (h.cases == 0 || h.cases > 8192u || (h.l_stride & 3u) || XT_BYTES + h.l_stride > 48u * 1024u) return 2;
  PArgs d = h;
  Tables t;
  if (tables(t)) return 1;
  d.logt = t.logt, d.exptab = t.exptab;
  const void *hp[] = {h.in0, h.in1, h.in2, h.in3, h.s0, h.s1, h.s2, h.s3, h.out0, h.out1, h.out2, h.so, h.g, h.limg, h.rng, h.rng2, h.scal};
  const void **dp[] = {(const void **)&d.in0, (const void **)&d.in1, (const void **)&d.in2, (const void **)&d.in3,
                       (const void **)&d.s0, (const void **)&d.s1, (const void **)&d.s2, (const void **)&d.s3,
                       (const void **)&d.out0, (const void **)&d.out1, (const void **)&d.out2, (const void **)&d.so,
                       (const void **)&d.g, (const void **)&d.limg, (const void **)&d.rng, (const void **)&d.rng2, (const void **)&d.scal};
  const uint64_t *sz = &z.in[0];
  constexpr int N = 17;
  static_assert(sizeof(PSizes) == N * sizeof(uint64_t), "one size per array");
  void *dev[N] = {};
  int rc = 0;
  for (int i = 0; i < N && !rc; ++i) {
    *dp[i] = nullptr;
    if (!sz[i] || !hp[i]) continue;
    if (hipMalloc(&dev[i], sz[i]) != hipSuccess || hipMemcpy(dev[i], hp[i], sz[i], hipMemcpyHostToDevice) != hipSuccess) rc = 1;
    *dp[i] = dev[i];
  }
  if (!rc) {
    hipLaunchKernelGGL(k, dim3(h.cases), dim3(64), XT_BYTES + h.l_stride, 0, d);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = 3;
  }
  for (int i = 0; i < N; ++i) {
    if (!dev[i]) continue;
    if (!rc && hipMemcpy(const_cast<void *>(hp[i]), dev[i], sz[i], hipMemcpyDeviceToHost) != hipSuccess) rc = 1;
    if (rc != 3) (void)hipFree(dev[i]);  // after a failed launch nothing more is asked of the device
  }
  return rc;
}

}  // namespace sfp

extern "C" {
// the tables the launchers upload, as the product's host code builds them: logt[LOGT_ENTRIES], exptab[512]
void sfp_tables(uint16_t *logt, uint32_t *exptab) {
  memset(logt, 0, sizeof(uint16_t) * sf::LOGT_ENTRIES);
  sf::build_rng_tables(logt, exptab);
}
int sfp_fused_round() { return sf::WaveGfx950::FUSED_ROUND ? 1 : 0; }  // which branch of Core::draw() this backend takes
#define X(name) \
  int sfp_##name(const sfp::PArgs *a, const sfp::PSizes *z) { return sfp::run(sfp::k_probe_##name, *a, *z); }
SFP_PROBES(X)
#undef X
}
