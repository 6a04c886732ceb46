// sf_rollout_dense.hpp — a stored observation list back to the dense row a torch module reads (include/strikeforce_policy.h,
// sf_rollout_dense): states[i] of the reference's epochs, `model->forward(states[i])` (bots/bot-1/Agent.hpp:392,
// RewardNet.hpp:265-274).  Included behind sf_rollout_gae.hpp.
//   k_rollout_dense<E>   one workgroup per row: the row's zeros as 16-byte stores with the list's loads between them, then
//                        the scatter
// A position's zero and its value come from different lanes and waves of one workgroup.  They are ordered: every wave
// waits until its zero stores are acknowledged (s_waitcnt vmcnt(0)), the workgroup meets at a barrier, and only then is
// a value stored.  Nothing reads the destination, so a 16-bit value is a 2-byte store.
#pragma once
#include "sf_rollout_gae.hpp"

namespace sfp {

constexpr int DENSE_ROW = 32 * 31 * 31;  // 30 752 elements
constexpr int DENSE_WG = 256;            // lanes per row: one 16-byte load of keys and of vals each covers 1024 entries
constexpr int DENSE_A = 8, DENSE_B = 7;  // rounds of zero stores in front of the count's load and of the entries' loads
static_assert(DENSE_WG * (DENSE_A + DENSE_B) * 16 <= DENSE_ROW * 2, "the unconditional rounds stay inside a 16-bit row");

struct DenseArgs {
  const uint32_t *keys, *vals;  // [T][stride][list_cap], the values as their bits
  const uint32_t *counts;       // [T][stride]
  const int32_t *cells;         // [rows] or null: row b is cell0 + b
  int32_t cell0;
  uint32_t n_cells;  // T * stride
  int list_cap;
  int nhwc;        // channel fastest
  void *dense;     // [rows][DENSE_ROW] of E
  uint8_t *valid;  // [rows] or null
};

// round-to-nearest-even; a NaN stays a NaN (quiet bit set)
__device__ inline uint16_t dense_bf16(uint32_t x) {
  const uint32_t r = (x + 0x7fffu + ((x >> 16) & 1u)) >> 16;
  return (uint16_t)((x & 0x7fffffffu) > 0x7f800000u ? (x >> 16) | 0x40u : r);
}
__device__ inline uint16_t dense_f16(uint32_t x) {
  const _Float16 h = (_Float16)__builtin_bit_cast(float, x);  // v_cvt_f16_f32: nearest even, overflow to inf, subnormals kept
  return __builtin_bit_cast(uint16_t, h);
}

// E: 0 = f32 (the value's bits), 1 = bf16, 2 = f16.  An entry whose key names no position of the row (channel above 31,
// row or column above 30) is skipped: nothing is written outside the row.
template <int E>
__device__ inline void dense_put(void *row, uint32_t k, uint32_t v, bool nhwc) {
  const uint32_t ch = (k & 511u) / 9u, y = (k >> 9) & 31u, x = (k >> 14) & 31u;
  if (ch >= 32u || y >= 31u || x >= 31u) return;
  const uint32_t pos = nhwc ? (y * 31u + x) * 32u + ch : (ch * 31u + y) * 31u + x;
  if (E == 0)
    static_cast<uint32_t *>(row)[pos] = v;
  else
    static_cast<uint16_t *>(row)[pos] = E == 1 ? dense_bf16(v) : dense_f16(v);
}

template <int E>
__global__ __launch_bounds__(DENSE_WG) void k_rollout_dense(DenseArgs g) {
  constexpr int UNITS = DENSE_ROW * (E == 0 ? 4 : 2) / 16;  // 7 688 or 3 844 16-byte units: the row is a whole number of them
  const int b = blockIdx.x, l = threadIdx.x;
  const bool nhwc = g.nhwc != 0;
  char *row = static_cast<char *>(g.dense) + (size_t)b * (size_t)(UNITS * 16);
  u32x4 *z = reinterpret_cast<u32x4 *>(row);
  const u32x4 zero = {0, 0, 0, 0};
  // The way to the list is three loads deep (cell, count, entries).  The zeros wait for none of them, so they are issued
  // in between: each load's latency runs under stores.  DENSE_A + DENSE_B full rounds of the workgroup fit either row.
  // the cell, checked before anything is read through it
  int32_t cell = g.cells ? g.cells[b] : g.cell0 + b;
#pragma unroll
  for (int u = 0; u < DENSE_A; ++u) z[l + DENSE_WG * u] = zero;
  cell = __builtin_amdgcn_readfirstlane(cell);
  bool good = (uint32_t)cell < g.n_cells;  // (a negative cell is above every n_cells <= 2^31 as unsigned)
  uint32_t count = 0;
  if (good) count = g.counts[(size_t)cell];
#pragma unroll
  for (int u = DENSE_A; u < DENSE_A + DENSE_B; ++u) z[l + DENSE_WG * u] = zero;
  count = (uint32_t)__builtin_amdgcn_readfirstlane((int)count);
  good = good && count <= (uint32_t)g.list_cap;  // the 0xffffffff marker is above every list_cap
  const uint32_t n = good ? count : 0u;
  const size_t src = good ? (size_t)cell * (size_t)g.list_cap : (size_t)0;
  const u32x4 *k4 = reinterpret_cast<const u32x4 *>(g.keys + src), *v4 = reinterpret_cast<const u32x4 *>(g.vals + src);
  // the first 1024 entries: loaded in front of the scatter, under the rest of the zeros (inside the stored row:
  // list_cap % 4 == 0; what lies behind the count is loaded and not used)
  u32x4 kr = {0, 0, 0, 0}, vr = {0, 0, 0, 0};
  if ((uint32_t)(4 * l) < n) kr = k4[l], vr = v4[l];
#pragma unroll 8
  for (int i = l + DENSE_WG * (DENSE_A + DENSE_B); i < UNITS; i += DENSE_WG) z[i] = zero;
  if (n == 0) {  // (uniform over the workgroup) nothing follows the zeros
    if (l == 0 && g.valid) g.valid[b] = good ? 1 : 0;
    return;
  }
  // zeros before values: each wave's zero stores are acknowledged, then the workgroup meets
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if ((uint32_t)(4 * l + j) < n) dense_put<E>(row, kr[j], vr[j], nhwc);
  for (uint32_t base = 4u * DENSE_WG; base < n; base += 4u * DENSE_WG) {  // lists above 1024 entries
    const uint32_t e = base + 4u * (uint32_t)l;
    if (e < n) {
      kr = k4[e >> 2], vr = v4[e >> 2];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e + (uint32_t)j < n) dense_put<E>(row, kr[j], vr[j], nhwc);
    }
  }
  if (l == 0 && g.valid) g.valid[b] = 1;
}

}  // namespace sfp
