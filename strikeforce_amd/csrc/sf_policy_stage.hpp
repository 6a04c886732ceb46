// sf_policy_stage.hpp — the host arithmetic that lays the network's weights out the way the policy kernels read them.
// Plain C++, nothing of HIP: sf_policy.hip's create() calls these, and tests/policy_stage/stage_main.cpp runs them on the
// CPU under the sanitizers (tests/test_policy_stage.py compares every image bit for bit with a restatement of the layouts).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace sfp {

constexpr int SPLIT_BN = 160, SPLIT_BK = 16;  // k_gemm_b3's strip of output columns and its K tile (BN, B3_BK)

// f32 -> bf16, round to nearest even (finite inputs: weights)
inline uint16_t bf16_rn(float x) {
  uint32_t u;
  std::memcpy(&u, &x, 4);
  if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)((u >> 16) | ((u & 0xffffu) ? 0x40u : 0u));
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf16_f32(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float x;
  std::memcpy(&x, &u, 4);
  return x;
}
// W [N][K] (N % 160 == 0, K % 16 == 0) -> k_gemm_b3's image: [N / 160][K / 16][160][3 parts][16] bf16
inline std::vector<uint16_t> split_weights(const float *W, int N, int K) {
  std::vector<uint16_t> img((size_t)N * K * 3);
  const int KT = K / SPLIT_BK;
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) {
      const float x = W[(size_t)n * K + k];
      const uint16_t hi = bf16_rn(x);
      const float r1 = x - bf16_f32(hi);
      const uint16_t mid = bf16_rn(r1);
      const float r2 = r1 - bf16_f32(mid);
      const uint16_t lo = bf16_rn(r2);
      const size_t rec = (((size_t)(n / SPLIT_BN) * KT + k / SPLIT_BK) * SPLIT_BN + n % SPLIT_BN) * 48 + k % SPLIT_BK;
      img[rec] = hi, img[rec + 16] = mid, img[rec + 32] = lo;
    }
  return img;
}

// W [N][K] (N, K % 16 == 0) appended to `stage` in k_tail's weight stream order (ts_wp / ts_issue); returns where it starts:
// Wt[tile][k-step][lane][j] = W[16 tile + (lane & 15)][16 k-step + 4 (lane >> 4) + j]
inline size_t stage_tiles(std::vector<float> &stage, const float *src, int N, int K) {
  const size_t off = stage.size();
  stage.resize(off + (size_t)N * K);
  float *t = stage.data() + off;
  for (int tile = 0; tile < N / 16; ++tile)
    for (int st = 0; st < K / 16; ++st)
      for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 4; ++j)
          t[(((size_t)tile * (K / 16) + st) * 64 + l) * 4 + j] = src[(size_t)(16 * tile + (l & 15)) * K + 16 * st + 4 * (l >> 4) + j];
  return off;
}

// conv0's weights [n][c][ky][kx] -> [c][ky][kx][n] for k_conv0_sparse (CK = channels * 9)
inline std::vector<float> conv0_transpose(const float *w, int N, int CK) {
  std::vector<float> tr((size_t)CK * N);
  for (int n = 0; n < N; ++n)
    for (int ck = 0; ck < CK; ++ck) tr[(size_t)ck * N + n] = w[(size_t)n * CK + ck];
  return tr;
}

// conv1..3's weights [n][cin][ky][kx] -> [n][ky][kx][cin]: the K-order of an NHWC im2col row
inline std::vector<float> conv_permute(const float *w, int N, int Cin) {
  std::vector<float> perm((size_t)N * Cin * 9);
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < Cin; ++c)
      for (int tap = 0; tap < 9; ++tap) perm[((size_t)n * 9 + tap) * Cin + c] = w[((size_t)n * Cin + c) * 9 + tap];
  return perm;
}

// src [rows][cols] as the top-left corner of a zero matrix [prows][pcols]: combined_processor's 329 inputs padded to
// COMB_PAD, a head's 9 rows or 1 row (and its bias) padded to the 16 columns of one MFMA tile
inline std::vector<float> pad_zero(const float *src, int rows, int cols, int prows, int pcols) {
  std::vector<float> pad((size_t)prows * pcols, 0.f);
  for (int r = 0; r < rows; ++r) std::memcpy(&pad[(size_t)r * pcols], src + (size_t)r * cols, (size_t)cols * sizeof(float));
  return pad;
}

}  // namespace sfp
