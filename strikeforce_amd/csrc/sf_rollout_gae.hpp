// sf_rollout_gae.hpp — the rollout buffer for a learner that does not train per game (include/strikeforce_policy.h,
// sf_rollout_continue, sf_rollout_gae).  Included behind sf_rollout.hpp.
//   k_rollout_record_cont   one tick of every agent into its next slot, game ends marked in first[slot], cursor never rewound
//   k_rollout_gae_v         V[T][agents] of the ready agents: the stored value or its f32 log, fully parallel
//   k_rollout_gae           the recursion G_t = gamma * boot_t + x_t over a ready agent's column, game ends cutting it
// The logarithm is in the parallel pass: the serial chain of k_rollout_gae holds four f32 operations per slot.
#pragma once
#include "sf_rollout.hpp"

namespace sfp {

// One wavefront per agent, the continuing rule: k_rollout_record's loads and stores (sf_rollout.hpp: keep the two in step)
// with the cursor never rewound and one byte more, first[slot] = the restart flag.  The body is restated here and not
// shared through a __device__ helper: with a helper, inlined, k_rollout_record came out of the compiler as 743 instructions
// in place of its 746, and that kernel has to stay the code it was.
__global__ __launch_bounds__(256) void k_rollout_record_cont(RolloutDst d, RolloutSrc s, uint8_t *first) {
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), l = threadIdx.x & 63;
  const int a = blockIdx.x * 4 + w;
  if (a >= s.agents) return;
  // the cursor, the flags and the count: unconditional loads from addresses that are valid whatever the options
  const uint8_t *fmp = s.reset_mask ? s.reset_mask + a : reinterpret_cast<const uint8_t *>(d.fill);
  const int32_t *fwp = s.reset_words ? s.reset_words + (size_t)(a / s.reset_group) * (size_t)s.reset_stride : d.fill;
  const uint32_t *cp = d.keys ? s.counts + a : reinterpret_cast<const uint32_t *>(d.fill);
  const uint8_t fm = *fmp;
  const int32_t fw = *fwp;
  int f = d.fill[a];
  uint32_t count = *cp;
  f = __builtin_amdgcn_readfirstlane(f);
  count = (uint32_t)__builtin_amdgcn_readfirstlane((int)count);
  const bool fresh = __builtin_amdgcn_readfirstlane((int)((s.reset_mask && fm != 0) || (s.reset_words && fw != 0))) != 0;
  if (f >= d.T) {
    if (l == 0) atomicAdd(&d.counters[0], 1ull);
    return;
  }
  const size_t slot = (size_t)f * (size_t)d.stride + (size_t)a;
  // this lane's share of the small rows, loaded in front of every store
  float p = 1.f, val = 0.f, rew = 0.f, dsc = 0.f;
  int32_t act = 0;
  uint8_t imi = 0;
  if (l < ACT) p = s.probs[(size_t)a * ACT + l];
  if (l == 0) {
    act = s.action[a], val = s.value[a], rew = s.reward[a];
    if (d.disc) dsc = s.disc[a];
    if (d.imitate) imi = s.imitate[a];
  }
  if (d.keys) {
    // min(count, list_cap) entries, never past either row; a count that does not fit is stored as it came
    uint32_t n = count < (uint32_t)d.list_cap ? count : (uint32_t)d.list_cap;
    n = n < (uint32_t)s.cap ? n : (uint32_t)s.cap;
    const uint32_t *sk = s.keys + (size_t)a * s.cap;
    const float *sv = s.vals + (size_t)a * s.cap;
    uint32_t *dk = d.keys + slot * d.list_cap;
    float *dv = d.vals + slot * d.list_cap;
    if (s.vec) {
      const int n4 = (int)(n >> 2), rest = (int)(n & 3u);
      uint32_t kt = 0;
      float vt = 0.f;
      if (l < rest) kt = sk[4 * n4 + l], vt = sv[4 * n4 + l];  // (entries behind the count are not written)
      rollout_copy2<u32x4, 4>(sk, sv, dk, dv, n4, l);
      if (l < rest) dk[4 * n4 + l] = kt, dv[4 * n4 + l] = vt;
    } else {
      rollout_copy2<uint32_t, 8>(sk, sv, dk, dv, (int)n, l);
    }
    const float *sp = s.pov + (size_t)a * HID;
    float *dp = d.pov + slot * HID;
    if (s.pov_vec) {
      if (l < HID / 4) reinterpret_cast<u32x4 *>(dp)[l] = reinterpret_cast<const u32x4 *>(sp)[l];
    } else {
      const Row3 r = row_load(sp, l);
      row_store(dp, l, r);
    }
    if (l == 0) {
      d.counts[slot] = count;
      if (count > (uint32_t)d.list_cap) atomicAdd(&d.counters[1], 1ull);
    }
  }
  if (l < ACT) d.logp[slot * ACT + l] = log_f32(p);
  if (l == 0) {
    d.action[slot] = act, d.value[slot] = val, d.reward[slot] = rew;
    if (d.disc) d.disc[slot] = dsc;
    if (d.imitate) d.imitate[slot] = imi;
    first[slot] = fresh ? 1 : 0;
    d.fill[a] = f + 1;
  }
}

// One lane per (agent, GV_ROWS slots): a slot's row is read and written with agents across the lanes, the rows' loads in
// front of the logarithms.  Agents that are not ready are skipped.
constexpr int GV_ROWS = 4;
__global__ __launch_bounds__(256) void k_rollout_gae_v(const int32_t *fill, const float *value, float *v, int T, int stride, int log_values,
                                                       int agents) {
#pragma clang fp contract(off)
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= agents) return;
  if (fill[a] != T) return;
  const int t0 = blockIdx.y * GV_ROWS;
  float x[GV_ROWS];
#pragma unroll
  for (int u = 0; u < GV_ROWS; ++u)
    if (t0 + u < T) x[u] = value[(size_t)(t0 + u) * (size_t)stride + a];
#pragma unroll
  for (int u = 0; u < GV_ROWS; ++u)
    if (t0 + u < T) v[(size_t)(t0 + u) * (size_t)stride + a] = log_values ? log_f32(x[u]) : x[u];
}

struct GaeArgs {
  float gamma, lambda, scale;
  int log_values;
  const float *next_value;    // [agents] or null: no bootstrap behind slot T - 1
  const uint8_t *next_mask;   // the restart flags of the tick behind slot T - 1, as RolloutSrc has this tick's; both null:
  const int32_t *next_words;  //   that tick continues the game
  int next_stride, next_group;
  const uint8_t *first;  // [T][stride] or null (the per-game rule: no game ends inside a buffer)
  const float *v;        // [T][stride]: k_rollout_gae_v's output, or the stored values themselves
  float *returns, *adv;  // [T][stride], each may be null
  int agents;
};

// One lane per ready agent, slots from T - 1 down, GAE_RB rows loaded ahead of the chain that depends on them.  f32, every
// product rounded before its add.  A game end behind slot t (first[t + 1], or the next tick's flag for t = T - 1) or a
// missing bootstrap leaves G_t = x_t: the term is selected away, not multiplied by 0, so an infinity or NaN of the next
// game never crosses.  One wavefront per workgroup: 4096 agents are 64 wavefronts, spread over 64 CUs.
constexpr int GAE_RB = 16;
__global__ __launch_bounds__(64) void k_rollout_gae(RolloutDst d, GaeArgs g) {
#pragma clang fp contract(off)
  const int a = blockIdx.x * 64 + threadIdx.x;
  if (a >= g.agents) return;
  if (d.fill[a] != d.T) return;
  const size_t st = (size_t)d.stride;
  const int T = d.T;
  bool cut = g.next_value == nullptr;  // does slot i's game end behind it (or is there nothing to bootstrap from)
  if (g.next_mask) cut = cut || g.next_mask[a] != 0;
  if (g.next_words) cut = cut || g.next_words[(size_t)(a / g.next_group) * (size_t)g.next_stride] != 0;
  float vn = 0.f;  // V_{i+1}
  if (g.next_value) {
    vn = g.next_value[a];
    if (g.log_values) vn = log_f32(vn);
  }
  const float lambda = g.lambda, oml = 1.f - lambda;
  const bool all_g = lambda == 1.f, all_v = lambda == 0.f;
  float G = 0.f;  // G_{i+1}
  for (int hi = T - 1; hi >= 0; hi -= GAE_RB) {
    float r[GAE_RB], v[GAE_RB];
    uint8_t e[GAE_RB];
#pragma unroll
    for (int u = 0; u < GAE_RB; ++u) {
      const int i = hi - u;
      if (i >= 0) {
        r[u] = d.reward[(size_t)i * st + a], v[u] = g.v[(size_t)i * st + a];
        e[u] = g.first ? g.first[(size_t)i * st + a] : (uint8_t)0;  // first[i]: the game of slot i - 1 ended behind it
      }
    }
#pragma unroll
    for (int u = 0; u < GAE_RB; ++u) {
      const int i = hi - u;
      if (i >= 0) {
        const float x = g.scale * r[u];
        const float pv = oml * vn, pg = lambda * G;
        const float mixed = pv + pg;  // (1 - lambda) * V_{i+1} + lambda * G_{i+1}
        const float boot = (i == T - 1 || all_v) ? vn : all_g ? G : mixed;
        const float y = g.gamma * boot;
        const float sum = y + x;
        G = cut ? x : sum;
        const size_t o = (size_t)i * st + a;
        if (g.returns) g.returns[o] = G;
        if (g.adv) g.adv[o] = G - v[u];
        vn = v[u];
        cut = e[u] != 0;
      }
    }
  }
}

}  // namespace sfp
