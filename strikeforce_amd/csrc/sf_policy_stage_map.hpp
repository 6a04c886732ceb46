// sf_policy_stage_map.hpp — every weight layout of the policy kernels as ONE function each: destination index -> source
// index (or "zero"), plus the f32 -> 3 x bf16 split.  Nothing of HIP and no allocation: sf_policy_load.hpp's kernels call
// these with one thread per destination element (sf_policy_load_weights), and tests/policy_load/map_main.cpp builds every
// image through them on the CPU and compares it bit for bit with sf_policy_stage.hpp's functions, which sf_policy_create
// uses.  Indices are 32 bit: the largest image (a split convolution, 691 200 halves) is far below 2^32.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SFP_MAP_HD __host__ __device__
#else
#define SFP_MAP_HD
#endif

namespace sfp {
namespace smap {

constexpr uint32_t ZERO = 0xffffffffu;    // "no source: the destination holds +0"
constexpr uint32_t BN = 160, BK = 16;     // k_gemm_b3's strip of output columns and its K tile (SPLIT_BN, SPLIT_BK)

// stage_tiles: Wt[tile][k-step][lane][j] = W[16 tile + (lane & 15)][16 k-step + 4 (lane >> 4) + j], W [N][K]
SFP_MAP_HD inline uint32_t tiles(uint32_t d, uint32_t K) {
  const uint32_t j = d & 3u, l = (d >> 2) & 63u, r = d >> 8, steps = K / 16u;
  const uint32_t st = r % steps, tile = r / steps;
  return (16u * tile + (l & 15u)) * K + 16u * st + 4u * (l >> 4) + j;
}

// conv0_transpose: [n][ck] -> [ck][n]
SFP_MAP_HD inline uint32_t conv0_transpose(uint32_t d, uint32_t N, uint32_t CK) {
  const uint32_t ck = d / N, n = d % N;
  return n * CK + ck;
}

// conv_permute: [n][cin][tap] -> [n][tap][cin]
SFP_MAP_HD inline uint32_t conv_permute(uint32_t d, uint32_t Cin) {
  const uint32_t c = d % Cin, r = d / Cin;
  const uint32_t tap = r % 9u, n = r / 9u;
  return (n * Cin + c) * 9u + tap;
}

// pad_zero: src [rows][cols] in the top-left corner of [prows][pcols]
SFP_MAP_HD inline uint32_t pad(uint32_t d, uint32_t rows, uint32_t cols, uint32_t pcols) {
  const uint32_t r = d / pcols, c = d % pcols;
  return r < rows && c < cols ? r * cols + c : ZERO;
}

// stage_tiles of pad_zero(src): the padded matrix [prows][pcols] in k_tail's stream order (rows == prows, cols == pcols:
// stage_tiles alone)
SFP_MAP_HD inline uint32_t tiles_of_pad(uint32_t d, uint32_t rows, uint32_t cols, uint32_t pcols) {
  return pad(tiles(d, pcols), rows, cols, pcols);
}

// split_weights' image [N / 160][K / 16][160][3 parts][16] bf16 of W [N][K]: half d holds part *part of W[returned index]
SFP_MAP_HD inline uint32_t split(uint32_t d, uint32_t K, uint32_t *part) {
  const uint32_t kk = d % BK;
  uint32_t r = d / BK;
  *part = r % 3u;
  r /= 3u;
  const uint32_t nn = r % BN;
  r /= BN;
  const uint32_t KT = K / BK, kt = r % KT, strip = r / KT;
  return (strip * BN + nn) * K + kt * BK + kk;
}

// the same of conv_permute(W): what sf_policy_create splits for conv1 and conv2 (K = 9 Cin)
SFP_MAP_HD inline uint32_t split_of_permute(uint32_t d, uint32_t Cin, uint32_t *part) {
  return conv_permute(split(d, 9u * Cin, part), Cin);
}

SFP_MAP_HD inline uint32_t f32_bits(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  return u;
}
SFP_MAP_HD inline float bits_f32(uint32_t u) {
  float x;
  __builtin_memcpy(&x, &u, 4);
  return x;
}
// f32 -> bf16, round to nearest even, in integer arithmetic (sf_policy_stage.hpp's bf16_rn; inf stays inf, a NaN stays one)
SFP_MAP_HD inline uint32_t bf16_rn(float x) {
  uint32_t u = f32_bits(x);
  if ((u & 0x7f800000u) == 0x7f800000u) return (u >> 16) | ((u & 0xffffu) ? 0x40u : 0u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return u >> 16;
}
// x = hi + mid + lo up to 2^-24 |x|: each part the nearest-even bf16 of what the parts before left.  Both subtractions are
// exact in f32 (a part and its remainder do not overlap), so contraction could not change them; it is off all the same.
SFP_MAP_HD inline void split3(float x, uint32_t part[3]) {
#pragma clang fp contract(off)
  part[0] = bf16_rn(x);
  const float r1 = x - bits_f32(part[0] << 16);
  part[1] = bf16_rn(r1);
  const float r2 = r1 - bits_f32(part[1] << 16);
  part[2] = bf16_rn(r2);
}

}  // namespace smap
}  // namespace sfp
