// probe_emu.cpp — TEST INFRASTRUCTURE: the probes of probe_body.hpp on the CPU wave emulator (tests/emu/wave_emu.hpp).
// Builds libsf_wave_probe_emu.so, loaded only by tests/wave_probe_lib.py.  Every export takes the host's own arrays.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../emu/wave_emu.hpp"
// clang-format off
#include "../../strikeforce_amd/csrc/sf_core.hpp"
#include "../../strikeforce_amd/csrc/sf_host.hpp"
#include "probe_body.hpp"
// clang-format on

namespace sfp {

struct EmuIO {
  static constexpr bool DEVICE = false;
  static sf::EmuV ld(const uint32_t *r) {
    sf::EmuV v;
    memcpy(v.v, r, sizeof v.v);
    return v;
  }
  static void st(uint32_t *r, const sf::EmuV &v) { memcpy(r, v.v, sizeof v.v); }
  static void stp(uint32_t *r, sf::EmuP p) {
    for (int i = 0; i < 64; ++i) r[i] = (uint32_t)((p.m >> i) & 1ull);
  }
  static void stu(uint32_t *p, uint32_t v) { *p = v; }
};
using PE = Probes<sf::WaveEmu, EmuIO>;

template <class F>
static int run(const PArgs &a, F fn) {
  std::vector<uint32_t> lds((XT_BYTES + a.l_stride + 3u) / 4u);
  uint8_t *l = (uint8_t *)lds.data();
  for (uint32_t c = 0; c < a.cases; ++c) {
    memcpy(l, a.exptab, XT_BYTES);
    if (a.l_stride) memcpy(l + XT_BYTES, a.limg + (size_t)c * a.l_stride, a.l_stride);
    fn(a, c, l);
    if (a.l_stride) memcpy(a.limg + (size_t)c * a.l_stride, l + XT_BYTES, a.l_stride);
  }
  return 0;
}

}  // namespace sfp

extern "C" {
// the generator's tables as the product's host code builds them: logt[LOGT_ENTRIES], exptab[512]
void sfpe_tables(uint16_t *logt, uint32_t *exptab) {
  memset(logt, 0, sizeof(uint16_t) * sf::LOGT_ENTRIES);
  sf::build_rng_tables(logt, exptab);
}
int32_t sfpe_logt_off() { return sf::LOGT_OFF; }
int sfpe_fused_round() { return sf::WaveEmu::FUSED_ROUND ? 1 : 0; }
uint32_t sfpe_sum_bias_lane() { return sfp::PE::C::SUM_BIAS_LANE; }
#define X(name) \
  int sfpe_##name(const sfp::PArgs *a) { return sfp::run(*a, sfp::PE::name); }
SFP_PROBES(X)
#undef X
}
