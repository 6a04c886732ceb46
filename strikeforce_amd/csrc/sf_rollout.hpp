// sf_rollout.hpp — the kernels of the device rollout buffer (include/strikeforce_policy.h, sf_rollout_*): what one bot-1
// `Agent` keeps per game in `states, log_probs, values, rewards, actions` (StrikeForce-client/bots/bot-1/Agent.hpp:200-204,
// 227,233-234,301-302), for every agent of a batch, and the gradient-free arithmetic computeReturns() / train_log() run
// over it (:333-351).  Included behind sf_policy_tail.hpp (log_f32).
//   k_rollout_record    one tick of every agent into its next slot (or nothing: the agent is ready)
//   k_rollout_returns   returns, log V, advantages and the two half-buffer statistics of the ready agents
//   k_rollout_release, k_rollout_ready, k_update_actions   the cursor and the policy's action slot
// Storage is the caller's, slot-major ([T][agents]...): a tick's stores of neighbouring agents are neighbours, and a ready
// agent's column is read with agents across the lanes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sfp {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // 16 bytes of a row, whatever they hold

// The caller's buffers and the library's cursor.  `stride` = the agent count the buffers were made for.
struct RolloutDst {
  uint32_t *keys;    // [T][stride][list_cap] or null: states are not kept
  float *vals;       // [T][stride][list_cap]
  uint32_t *counts;  // [T][stride]
  float *pov;        // [T][stride][160]
  int32_t *action;   // [T][stride]
  float *logp;       // [T][stride][9]
  float *value, *reward;  // [T][stride]
  float *disc;            // [T][stride] or null
  uint8_t *imitate;       // [T][stride] or null
  int32_t *fill;          // [stride]: slots written, T = ready
  unsigned long long *counters;  // [0] ticks dropped on a ready agent, [1] states stored with a list that did not fit, [2] scratch of sf_rollout_status
  int stride, T, list_cap;
};
// One tick's buffers, as the two networks left them.
struct RolloutSrc {
  const uint32_t *keys;
  const float *vals;
  const uint32_t *counts;
  const float *pov;
  int cap;
  int vec;  // the list rows are 16-byte aligned (cap % 4 == 0 and aligned bases): 16-byte loads
  int pov_vec;
  const float *probs, *value;
  const int32_t *action;
  const float *reward, *disc;
  const uint8_t *imitate;
  const uint8_t *reset_mask;   // [agents] or null
  const int32_t *reset_words;  // word (a / reset_group) * reset_stride, or null
  int reset_stride, reset_group;
  int agents;
};

// n units (V = 16 bytes or a dword) of a key row and of a value row, a batch's loads in front of its stores
template <class V, int UN>
__device__ inline void rollout_copy2(const void *sk, const void *sv, void *dk, void *dv, int n, int l) {
  const V *k = static_cast<const V *>(sk), *v = static_cast<const V *>(sv);
  V *ko = static_cast<V *>(dk), *vo = static_cast<V *>(dv);
  for (int base = 0; base < n; base += 64 * UN) {  // (n is uniform over the wave)
    V kr[UN], vr[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int i = base + 64 * u + l;
      if (i < n) kr[u] = k[i], vr[u] = v[i];
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int i = base + 64 * u + l;
      if (i < n) ko[i] = kr[u], vo[i] = vr[u];
    }
  }
}

// One wavefront per agent.  In order: a ready agent (fill == T) drops the tick, restart flag or not (`if (is_training ...)
// return;`, Agent.hpp:219); a restarted game's agent starts at slot 0 again (a new Agent per game; ~Agent trains nothing
// from a partial buffer); the tick is appended at slot `fill`.
__global__ __launch_bounds__(256) void k_rollout_record(RolloutDst d, RolloutSrc s) {
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
  if (fresh) f = 0;
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
    // min(count, list_cap) entries — never past the caller's row; a count that does not fit (the 0xffffffff marker too)
    // is stored as it came: sf_policy_forward_sparse on the stored row sees "did not fit" as the live call did
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
  if (l < ACT) d.logp[slot * ACT + l] = log_f32(p);  // torch::log(output[0])   Agent.hpp:204
  if (l == 0) {
    d.action[slot] = act, d.value[slot] = val, d.reward[slot] = rew;
    if (d.disc) d.disc[slot] = dsc;
    if (d.imitate) d.imitate[slot] = imi;
    d.fill[a] = f + 1;
  }
}

// computeReturns() (Agent.hpp:333-339), the log V and the advantage of the PPO epochs (:401,407) and train_log()'s four
// numbers (:342-350) for the ready agents, one lane per agent: a slot's row is read with agents across the lanes.  f32 in
// the reference's operation order, every product rounded before the add (no contraction); the statistics are sequential
// f32 sums in slot order.  RB rows are loaded ahead of the chain that depends on them.
constexpr int RR_RB = 8;
__global__ __launch_bounds__(256) void k_rollout_returns(RolloutDst d, float gamma, float *returns, float *logv, float *adv, float *stats, int agents) {
#pragma clang fp contract(off)
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= agents) return;
  if (d.fill[a] != d.T) return;
  const size_t st = (size_t)d.stride;
  const int T = d.T;
  const float om = 1.f - gamma;
  float ret = 0.f;
  for (int hi = T - 1; hi >= 0; hi -= RR_RB) {
    float r[RR_RB], v[RR_RB];
#pragma unroll
    for (int u = 0; u < RR_RB; ++u) {
      const int i = hi - u;
      if (i >= 0) r[u] = d.reward[(size_t)i * st + a], v[u] = d.value[(size_t)i * st + a];
    }
#pragma unroll
    for (int u = 0; u < RR_RB; ++u) {
      const int i = hi - u;
      if (i >= 0) {
        const float x = om * r[u];
        if (i == T - 1) {
          ret = x;  // returns[T - 1] = (1 - gamma) * rewards[T - 1]
        } else {
          const float y = gamma * ret;
          ret = y + x;  // gamma * returns[i + 1] + (1 - gamma) * rewards[i]
        }
        const float lv = log_f32(v[u]);
        const size_t o = (size_t)i * st + a;
        if (returns) returns[o] = ret;
        if (logv) logv[o] = lv;
        if (adv) adv[o] = ret - lv;
      }
    }
  }
  if (!stats) return;
  const int half = T / 2;
  float sum[2] = {0.f, 0.f}, nothing[2] = {0.f, 0.f};
#pragma unroll
  for (int h = 0; h < 2; ++h)
    for (int lo = h * half; lo < (h + 1) * half; lo += RR_RB) {
      float r[RR_RB];
      int32_t ac[RR_RB];
#pragma unroll
      for (int u = 0; u < RR_RB; ++u) {
        const int i = lo + u;
        if (i < (h + 1) * half) r[u] = d.reward[(size_t)i * st + a], ac[u] = d.action[(size_t)i * st + a];
      }
#pragma unroll
      for (int u = 0; u < RR_RB; ++u) {
        const int i = lo + u;
        if (i < (h + 1) * half) {
          sum[h] = sum[h] + r[u];
          nothing[h] = nothing[h] + (ac[u] == 0 ? 1.f : 0.f);
        }
      }
    }
  // r_avg: the half sums over T, as :347-348 divide them; n_avg over T / 2 (:349-350)
  const f32x4 o = {sum[0] / (float)T, sum[1] / (float)T, nothing[0] / (float)half, nothing[1] / (float)half};
  reinterpret_cast<f32x4 *>(stats)[a] = o;
}

// clear() of the five vectors (Agent.hpp:430-431): with a mask, the agents whose byte is set, ready or not; without,
// every ready agent
__global__ void k_rollout_release(int32_t *fill, int T, const uint8_t *mask, int agents) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  if (a >= agents) return;
  if (mask ? mask[a] != 0 : fill[a] == T) fill[a] = 0;
}

// mask[a] = the agent is ready (either output may be null); count: how many are
__global__ void k_rollout_ready(const int32_t *fill, int T, uint8_t *mask, unsigned long long *count, int agents) {
  const int a = blockIdx.x * 256 + threadIdx.x;
  const bool ready = a < agents && fill[a] == T;
  if (a < agents && mask) mask[a] = ready ? 1 : 0;
  if (count) {
    const unsigned long long b = __ballot(ready);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
  }
}

// AgentModel::update_actions(one_hot(action)) (Agent.hpp:396, RewardNet.hpp:271-272); an index outside [0, 9) means 0
__global__ void k_update_actions(float *action_input, const int32_t *action, int agents) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= agents * ACT) return;
  const int a = e / ACT, j = e - a * ACT;
  int given = action[a];
  given = (uint32_t)given < (uint32_t)ACT ? given : 0;
  action_input[e] = (j == given) ? 1.f : 0.f;
}

}  // namespace sfp
