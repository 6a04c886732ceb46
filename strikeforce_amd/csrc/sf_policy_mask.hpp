// sf_policy_mask.hpp — sf_policy_act_masked (strikeforce_policy.h): sf_policy_act's draw under an action mask
// (sf_action_mask_io.d_actions, strikeforce.h).  Included by sf_policy.hip behind sf_policy_tail.hpp, whose act_pick, ActStr
// and mix64 it uses or restates; act_pick, k_act and k_tail are not touched, and the fused sf_policy_predict_sparse keeps
// drawing unmasked.
//
// act_pick_masked is act_pick with one line more: behind the scaling (v[0] = 0.5, the rest scaled to 0.5 in all) every v[k]
// whose bit is clear becomes 0; bit 0 counts as set whatever the word says, so the word 0 of a dead seat yields action 0.
// The sum, the hashed draw, the search and the arg-max are act_pick's own operations in act_pick's order: with every bit set
// the two agree bit for bit.  A masked entry has width 0 in the search (`u < c` with c unchanged) and u < tot always holds
// (u = x * tot with x <= 1 - 2^-24, and the float below a power of two is exactly 2^-24 of it away), so the search ends at
// the last unmasked entry at the latest: a masked action is never drawn.  `tot` is returned for d_probs_out.
#pragma once

namespace sfp {

__device__ inline int act_pick_masked(float (&v)[ACT], uint32_t mask, uint64_t seed, uint64_t draw, int greedy, int a, float &tot) {
#pragma clang fp contract(off)  // separate multiplies and adds, as act_pick's come out: the sum is restated in the tests
  const float sc = 0.5f / (1.f - v[0] + 1e-5f);
#pragma unroll
  for (int k = 1; k < ACT; ++k) v[k] *= sc;
  v[0] = 0.5f;
#pragma unroll
  for (int k = 1; k < ACT; ++k) v[k] = ((mask >> k) & 1u) ? v[k] : 0.f;
  tot = 0.f;
#pragma unroll
  for (int k = 0; k < ACT; ++k) tot += v[k];
  int pick = 0;
  if (greedy) {
#pragma unroll
    for (int k = 1; k < ACT; ++k)
      if (v[k] > v[pick]) pick = k;
  } else {
    const uint64_t r = mix64(mix64(seed ^ mix64((uint64_t)a)) + draw);
    const float u = (float)(r >> 40) * (1.0f / 16777216.0f) * tot;  // [0, tot)
    float c = 0.f;
    bool found = false;
    pick = ACT - 1;
#pragma unroll
    for (int k = 0; k < ACT - 1; ++k) {
      c += v[k];
      if (!found && u < c) pick = k, found = true;
    }
  }
  return pick;
}

// k_act with the mask word of the agent and the distribution the action was drawn from as a third, optional output
__global__ void k_act_masked(const float *probs, const uint32_t *mask, float *action_input, ActStr as, uint64_t seed,
                             uint64_t draw, int greedy, uint8_t *cmd, int32_t *action, float *probs_out, int agents) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= agents) return;
  float v[ACT];
#pragma unroll
  for (int k = 0; k < ACT; ++k) v[k] = probs[(size_t)a * ACT + k];
  float tot;
  const int pick = act_pick_masked(v, mask[a], seed, draw, greedy, a, tot);
#pragma unroll
  for (int k = 0; k < ACT; ++k) action_input[(size_t)a * ACT + k] = (k == pick) ? 1.f : 0.f;
  cmd[a] = (uint8_t)as.c[pick];
  if (action) action[a] = pick;
  if (probs_out) {
#pragma unroll
    for (int k = 0; k < ACT; ++k) probs_out[(size_t)a * ACT + k] = __fdiv_rn(v[k], tot);
  }
}

}  // namespace sfp
