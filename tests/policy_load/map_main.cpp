// map_main.cpp — builds every weight image through the index maps of strikeforce_amd/csrc/sf_policy_stage_map.hpp (what
// sf_policy_load_weights' kernel evaluates with one thread per destination element) and compares it BIT FOR BIT with the
// image sf_policy_stage.hpp's functions build (what sf_policy_create uploads), for tests/test_policy_load_maps.py, which
// builds this with -fsanitize=address,undefined.
//
//   map_main            every case; prints one line "ok <case> <elements>" per case, or "MISMATCH <case> at <index>" and
//                       exits 1
// Every source lies in a heap block of exactly its size, so a map that points outside it is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../strikeforce_amd/csrc/sf_policy_stage.hpp"
#include "../../strikeforce_amd/csrc/sf_policy_stage_map.hpp"

namespace smap = sfp::smap;

static int failures = 0;

template <class T>
static void same(const std::string &name, const std::vector<T> &got, const std::vector<T> &want) {
  if (got.size() != want.size()) {
    std::printf("MISMATCH %s size %zu != %zu\n", name.c_str(), got.size(), want.size());
    ++failures;
    return;
  }
  for (size_t i = 0; i < got.size(); ++i)
    if (std::memcmp(&got[i], &want[i], sizeof(T)) != 0) {
      std::printf("MISMATCH %s at %zu\n", name.c_str(), i);
      ++failures;
      return;
    }
  std::printf("ok %s %zu\n", name.c_str(), got.size());
}

// `n` floats in a block of exactly that size; every element distinct and none zero (a swapped index cannot cancel)
static std::unique_ptr<float[]> distinct(size_t n, float base = 1.0f) {
  std::unique_ptr<float[]> p(new float[n]);
  for (size_t i = 0; i < n; ++i) p[i] = base + (float)i;
  return p;
}

static float from_bits(uint32_t u) {
  float x;
  std::memcpy(&x, &u, 4);
  return x;
}

// one matrix through a map: element d of the image is src[map(d)] or +0
template <class Map>
static std::vector<float> gather(const float *src, size_t n, Map map) {
  std::vector<float> out(n);
  for (size_t d = 0; d < n; ++d) {
    const uint32_t s = map((uint32_t)d);
    out[d] = s == smap::ZERO ? 0.f : src[s];
  }
  return out;
}

static void tiles_case(const std::string &name, int rows, int cols, int prows, int pcols) {
  const auto src = distinct((size_t)rows * cols);
  const std::vector<float> pad = sfp::pad_zero(src.get(), rows, cols, prows, pcols);
  std::vector<float> want;
  want.assign(7, -1.f);  // (stage_tiles appends: the image starts behind what the block holds)
  const size_t off = sfp::stage_tiles(want, pad.data(), prows, pcols);
  want.erase(want.begin(), want.begin() + (long)off);
  same(name, gather(src.get(), (size_t)prows * pcols, [&](uint32_t d) { return smap::tiles_of_pad(d, rows, cols, pcols); }), want);
  if (rows == prows && cols == pcols)
    same(name + "/plain", gather(src.get(), (size_t)rows * cols, [&](uint32_t d) { return smap::tiles(d, cols); }), want);
}

static void pad_case(const std::string &name, int rows, int cols, int prows, int pcols) {
  const auto src = distinct((size_t)rows * cols);
  same(name, gather(src.get(), (size_t)prows * pcols, [&](uint32_t d) { return smap::pad(d, rows, cols, pcols); }),
       sfp::pad_zero(src.get(), rows, cols, prows, pcols));
}

// the values a split has to get right: ties, round-ups into the next exponent (and into infinity), zeros, denormals, +-inf
static std::vector<float> split_specials() {
  const uint32_t bits[] = {
      0x00000000u, 0x80000000u,                            // +-0
      0x3f808000u, 0x3f818000u, 0xbf808000u, 0xbf818000u,  // ties: to even down, to even up
      0x3f808001u, 0x3f807fffu,                            // just above / below a tie
      0x3f7fffffu, 0x3fffffffu, 0xbfffffffu, 0x407fc000u,  // round up into the next exponent
      0x7f7fffffu, 0xff7fffffu, 0x7f7f8000u,               // round up into infinity
      0x7f800000u, 0xff800000u,                            // +-inf
      0x00000001u, 0x80000001u, 0x00008000u, 0x00018000u, 0x007fffffu, 0x807fffffu, 0x00800000u, 0x00ffffffu,  // denormals and the edge
      0x3f800001u, 0x3f80ffffu, 0x4b7fffffu, 0x33800000u, 0x0c000001u,
  };
  std::vector<float> v;
  for (uint32_t b : bits) v.push_back(from_bits(b));
  return v;
}

static std::unique_ptr<float[]> split_values(size_t n) {
  std::unique_ptr<float[]> p(new float[n]);
  const std::vector<float> sp = split_specials();
  uint64_t s = 0x2545f4914f6cdd1dull;
  for (size_t i = 0; i < n; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    uint32_t u = (uint32_t)(s >> 32);
    const uint32_t e = 87u + (u >> 23) % 80u;  // exponents 2^-40 .. 2^39: finite, normal
    u = (u & 0x807fffffu) | (e << 23);
    p[i] = from_bits(u);
  }
  for (size_t i = 0; i < sp.size() && i * 7 + 3 < n; ++i) p[i * 7 + 3] = sp[i];  // spread over rows and K tiles
  return p;
}

static std::vector<uint16_t> split_image(const float *src, size_t halves, bool permuted, int K_or_Cin) {
  std::vector<uint16_t> out(halves);
  for (size_t d = 0; d < halves; ++d) {
    uint32_t part = 0, p[3];
    const uint32_t s = permuted ? smap::split_of_permute((uint32_t)d, (uint32_t)K_or_Cin, &part) : smap::split((uint32_t)d, (uint32_t)K_or_Cin, &part);
    smap::split3(src[s], p);
    out[d] = (uint16_t)p[part];
  }
  return out;
}

int main() {
  const int HID = 160, ACT = 9, OBS_C = 32, G3 = 480, COMB = 329, COMB_PAD = 352;
  // k_tail's stream order: the network's matrices, then the small shapes of tests/test_policy_stage.py
  tiles_case("tiles/gru", G3, HID, G3, HID);
  tiles_case("tiles/res", HID, HID, HID, HID);
  tiles_case("tiles/comb-padded", HID, COMB, HID, COMB_PAD);
  tiles_case("tiles/policy-head-padded", ACT, HID, 16, HID);
  tiles_case("tiles/value-head-padded", 1, HID, 16, HID);
  tiles_case("tiles/32x32", 32, 32, 32, 32);
  tiles_case("tiles/16x352", 16, COMB_PAD, 16, COMB_PAD);
  tiles_case("tiles/odd-corner", 13, 21, 32, 48);
  // paddings
  pad_case("pad/comb", HID, COMB, HID, COMB_PAD);
  pad_case("pad/policy-head", ACT, HID, 16, HID);
  pad_case("pad/value-head", 1, HID, 16, HID);
  pad_case("pad/policy-bias", ACT, 1, 16, 1);
  pad_case("pad/value-bias", 1, 1, 16, 1);
  pad_case("pad/odd", 3, 5, 7, 11);
  // conv0's transpose and conv1..3's permutation
  const int conv0_shapes[3][2] = {{HID, OBS_C * 9}, {5, 7}, {1, 9}}, perm_shapes[3][2] = {{HID, HID}, {3, 5}, {7, 1}};
  for (const auto &nc : conv0_shapes) {
    const auto src = distinct((size_t)nc[0] * nc[1]);
    same("conv0/" + std::to_string(nc[0]) + "x" + std::to_string(nc[1]),
         gather(src.get(), (size_t)nc[0] * nc[1], [&](uint32_t d) { return smap::conv0_transpose(d, nc[0], nc[1]); }),
         sfp::conv0_transpose(src.get(), nc[0], nc[1]));
  }
  for (const auto &nc : perm_shapes) {
    const size_t n = (size_t)nc[0] * nc[1] * 9;
    const auto src = distinct(n);
    same("perm/" + std::to_string(nc[0]) + "x" + std::to_string(nc[1]),
         gather(src.get(), n, [&](uint32_t d) { return smap::conv_permute(d, nc[1]); }), sfp::conv_permute(src.get(), nc[0], nc[1]));
  }
  // the bf16 split: conv1 / conv2 as create() builds them (split of the permuted tensor), the image alone at two strips x
  // two K tiles, and each special value's three parts against sf_policy_stage.hpp's own arithmetic
  {
    const size_t n = (size_t)HID * HID * 9;
    const auto src = split_values(n);
    const std::vector<float> perm = sfp::conv_permute(src.get(), HID, HID);
    same("split/conv-permuted", split_image(src.get(), n * 3, true, HID), sfp::split_weights(perm.data(), HID, HID * 9));
  }
  {
    const auto src = split_values((size_t)320 * 32);
    same("split/320x32", split_image(src.get(), (size_t)320 * 32 * 3, false, 32), sfp::split_weights(src.get(), 320, 32));
  }
  {
    std::vector<uint16_t> got, want;
    for (float x : split_specials()) {
      uint32_t p[3];
      smap::split3(x, p);
      const uint16_t hi = sfp::bf16_rn(x);
      const float r1 = x - sfp::bf16_f32(hi);
      const uint16_t mid = sfp::bf16_rn(r1);
      const uint16_t lo = sfp::bf16_rn(r1 - sfp::bf16_f32(mid));
      for (int k = 0; k < 3; ++k) got.push_back((uint16_t)p[k]);
      want.push_back(hi), want.push_back(mid), want.push_back(lo);
      if (p[0] > 0xffffu || p[1] > 0xffffu || p[2] > 0xffffu) ++failures, std::printf("MISMATCH split/specials: a part above 16 bits\n");
    }
    same("split/specials", got, want);
    // the ties went to even and the round-up crossed the exponent: 1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6, 1.99999988 -> 2
    uint32_t p[3];
    smap::split3(from_bits(0x3f808000u), p);
    if (p[0] != 0x3f80u) ++failures, std::printf("MISMATCH tie down\n");
    smap::split3(from_bits(0x3f818000u), p);
    if (p[0] != 0x3f82u) ++failures, std::printf("MISMATCH tie up\n");
    smap::split3(from_bits(0x3fffffffu), p);
    if (p[0] != 0x4000u) ++failures, std::printf("MISMATCH round-up into the next exponent\n");
    smap::split3(from_bits(0x7f800000u), p);
    if (p[0] != 0x7f80u) ++failures, std::printf("MISMATCH +inf\n");
    smap::split3(from_bits(0x80000000u), p);
    if (p[0] != 0x8000u) ++failures, std::printf("MISMATCH -0\n");
  }
  return failures ? 1 : 0;
}
