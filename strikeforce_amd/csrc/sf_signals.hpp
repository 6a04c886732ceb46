// sf_signals.hpp — the device side of sf_signals_step (strikeforce.h): per (arena, agent) the levels of what the game knows
// about a commanded human (vitals), what changed since the previous call (delta) and a weighted sum of it (reward), from
// the state buffers and the result latch the step kernels wrote.  Nothing of the environment is written.
//
// The per-agent body is a plain SF_HD function over pointers: k_signals (sf_api.hip) calls it with one lane per (arena,
// agent), the tests' CPU runtime (tests/emu/sf_emu.cpp) in a loop, and both compile this text.
//
// A signals object keeps SIG_BASE_WORDS words per (arena, agent): what the previous call saw.  The arena's words (seed,
// step count, episode count, done flag) are kept once per AGENT, not once per arena: the lanes of one arena may sit in
// different wavefronts, and a shared record would be read by one while another rewrites it.  Every lane of an arena loads
// the same scalar block and the same arena words of its own copy, so the decisions of rules 1-3 come out the same on all
// of them without any exchange.  The rules are in strikeforce.h; `signals_agent` follows their order.
//
// All loads — eight words of slot g's row of hum, the scalar block's words, the latch row, the baseline row, the rebase
// byte — are issued before the first value is looked at; the optional outputs are skipped by pointer.  No LDS, no scratch;
// the two counters of sf_signals_status are device counters (one atomic add on the rare paths that count).
#pragma once
#include "../../include/strikeforce.h"
#include "sf_types.hpp"

namespace sf {

// the baseline row of one (arena, agent)
enum { SB_VALID = 0, SB_TB_LO, SB_TB_HI, SB_SR_LO, SB_SR_HI, SB_STEPS, SB_EPISODES, SB_DONE,
       SB_C0 /* the six counters of sf_results' words 0..5 */, SB_PRESENT = SB_C0 + 6, SB_PAD, SIG_BASE_WORDS = 16 };
enum { SIG_UNRESOLVED = 0, SIG_DETECTED, SIG_COUNTERS = 4 };  // the device counters (sf_signals_status)

// What k_signals takes, by value in the kernel arguments.  A struct of its own, like ResetSel and Snap: Params stays as it is.
struct Signals {
  const uint32_t *hum;      // Params::hum  [HW_WORDS][A][H]
  const int32_t *scal;      // Params::scal [A][SC_WORDS]
  const int32_t *results;   // Params::results [A][n_agents][8]
  int32_t *base;            // [A * n_agents][SIG_BASE_WORDS]
  unsigned long long *counters;  // [SIG_COUNTERS]
  int32_t *vitals;          // null, or [A * n_agents][SF_VITALS_WORDS]
  int32_t *delta;           // null, or [A * n_agents][SF_DELTA_WORDS]
  float *reward;            // null, or [A * n_agents]
  const uint8_t *rebase;    // null, or [A * n_agents]
  int32_t A, H, n_agents, pad;
  sf_reward_weights w;
};

#if defined(__HIP_DEVICE_COMPILE__)
#define SF_SIG_G __attribute__((address_space(1)))
template <class T>
static __device__ __forceinline__ const SF_SIG_G T *sig_g(const T *p) { return (const SF_SIG_G T *)p; }
template <class T>
static __device__ __forceinline__ SF_SIG_G T *sig_g(T *p) { return (SF_SIG_G T *)p; }
static __device__ __forceinline__ void sig_count(unsigned long long *c) {
  (void)__hip_atomic_fetch_add(sig_g(c), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#else
template <class T>
static inline T *sig_g(T *p) { return p; }
static inline void sig_count(unsigned long long *c) { ++*c; }
#endif

// lane i = arena * n_agents + agent; the caller has checked i < A * n_agents
SF_HD inline void signals_agent(const Signals &k, int i) {
#pragma clang fp contract(off)
  const int a = i / k.n_agents, g = i - a * k.n_agents;
  // ---- every load ----
  const size_t AH = (size_t)k.A * (size_t)k.H, row = (size_t)a * (size_t)k.H + (size_t)g;
  const auto *hum = sig_g(k.hum);
  const uint32_t pos = hum[HW_POS * AH + row], fl = hum[HW_FLAGS * AH + row], hp = hum[HW_HP * AH + row];
  const uint32_t st = hum[HW_STAMINA * AH + row], md = hum[HW_MINDAMAGE * AH + row], hk = hum[HW_KILLS * AH + row];
  const uint32_t hd = hum[HW_DAMAGE * AH + row], he = hum[HW_EFFECT * AH + row];
  const auto *sc = sig_g(k.scal) + (size_t)a * SC_WORDS;
  const int32_t kills = sc[SC_KILLS], tkills = sc[SC_TKILLS], loot = sc[SC_LOOT], steps = sc[SC_STEPS];
  const int32_t episodes = sc[SC_EPISODES], done = sc[SC_DONE] != 0, sc_outcome = sc[SC_OUTCOME];
  const int32_t tb_lo = sc[SC_TB_LO], tb_hi = sc[SC_TB_HI], sr_lo = sc[SC_SR_LO], sr_hi = sc[SC_SR_HI];
  const auto *lr = sig_g(k.results) + (size_t)i * 8u;
  int32_t latch[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) latch[j] = lr[j];
  auto *bp = sig_g(k.base) + (size_t)i * SIG_BASE_WORDS;
  int32_t b[SIG_BASE_WORDS];
#pragma unroll
  for (int j = 0; j < SIG_BASE_WORDS; ++j) b[j] = bp[j];
  const bool announced = k.rebase ? sig_g(k.rebase)[i] != 0 : false;

  // ---- the rules ----
  const bool present = (fl & (HF_ALIVE | HF_CTRL)) == (HF_ALIVE | HF_CTRL);
  const bool was = b[SB_PRESENT] != 0;
  const int32_t cur[6] = {(int32_t)hk, tkills, loot, (int32_t)hd, (int32_t)he, (int32_t)hp};
  const int32_t n = episodes - b[SB_EPISODES], ds = steps - b[SB_STEPS];
  const bool other_seed = tb_lo != b[SB_TB_LO] || tb_hi != b[SB_TB_HI] || sr_lo != b[SB_SR_LO] || sr_hi != b[SB_SR_HI];
  const bool detected = n < 0 || (n == 0 && (other_seed || ds < 0));
  uint32_t flags = present ? (uint32_t)SF_SIG_PRESENT : 0u;
  int32_t d[6] = {0, 0, 0, 0, 0, 0}, outcome = 0;
  bool credit = was;  // whether the reward counts this agent as present in the baseline
  if (!b[SB_VALID] || announced || detected) {  // rule 1
    flags |= SF_SIG_REBASED;
    credit = false;
    if (b[SB_VALID] && !announced) sig_count(k.counters + SIG_DETECTED);
  } else if (n >= 2) {  // rule 2
    flags |= SF_SIG_ENDED | SF_SIG_UNRESOLVED;
    outcome = latch[7];
  } else if (n == 1) {  // rule 3
    flags |= SF_SIG_ENDED;
    outcome = latch[7];
    if (was) {
#pragma unroll
      for (int j = 0; j < 6; ++j) d[j] = latch[j] - b[SB_C0 + j];
    }
  } else {  // rule 4: the same game
    if (done && b[SB_DONE]) flags |= SF_SIG_IDLE;
    if (done && !b[SB_DONE]) flags |= SF_SIG_ENDED, outcome = sc_outcome;  // a replayed stream ran out (SF_SAMPLE_END)
    if (was) {
      if (present || (!(fl & HF_ALIVE) && ds == 1)) {  // its own row: living, or its corpse of this one step
#pragma unroll
        for (int j = 0; j < 6; ++j) d[j] = cur[j] - b[SB_C0 + j];
      } else {  // the row may be a spawned NPC's: only the arena's counters and the loss of its Hp are its own
        d[1] = cur[1] - b[SB_C0 + 1], d[2] = cur[2] - b[SB_C0 + 2], d[5] = -b[SB_C0 + 5];
        if (ds > 1) flags |= SF_SIG_UNRESOLVED;
      }
      if (!present) flags |= SF_SIG_DIED;
    }
  }
  if (flags & SF_SIG_UNRESOLVED) sig_count(k.counters + SIG_UNRESOLVED);

  // ---- the baseline becomes the current state ----
  bp[SB_VALID] = 1, bp[SB_TB_LO] = tb_lo, bp[SB_TB_HI] = tb_hi, bp[SB_SR_LO] = sr_lo, bp[SB_SR_HI] = sr_hi;
  bp[SB_STEPS] = steps, bp[SB_EPISODES] = episodes, bp[SB_DONE] = done;
#pragma unroll
  for (int j = 0; j < 6; ++j) bp[SB_C0 + j] = cur[j];
  bp[SB_PRESENT] = present ? 1 : 0;

  // ---- outputs ----
  if (k.vitals) {
    auto *v = sig_g(k.vitals) + (size_t)i * SF_VITALS_WORDS;
    const bool placed = present && pos != POS_NONE;
    v[0] = (int32_t)flags;
    v[1] = present ? (int32_t)hp : 0, v[2] = present ? (int32_t)st : 0, v[3] = present ? (int32_t)md : 0;
    v[4] = present ? (int32_t)hk : 0, v[5] = present ? (int32_t)hd : 0, v[6] = present ? (int32_t)he : 0;
    v[7] = placed ? pos_f(pos) : 0, v[8] = placed ? pos_r(pos) : 0, v[9] = placed ? pos_c(pos) : 0;
    v[10] = present ? (int32_t)(fl & HF_WAY_MASK) : 0, v[11] = present ? (int32_t)((fl >> HF_TEAM_SH) & 255u) : 0;
    v[12] = kills, v[13] = tkills, v[14] = loot, v[15] = steps;
  }
  if (k.delta) {
    auto *o = sig_g(k.delta) + (size_t)i * SF_DELTA_WORDS;
    o[0] = (int32_t)flags;
#pragma unroll
    for (int j = 0; j < 6; ++j) o[1 + j] = d[j];
    o[7] = outcome;
  }
  if (k.reward) {
    float r = 0.f;
    if (!(flags & (SF_SIG_REBASED | SF_SIG_IDLE))) {
      if (credit) {
        r = k.w.per_step;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          const float t = k.w.w[j] * (float)d[j];
          r = r + t;
        }
      }
      if (flags & SF_SIG_DIED) r = r + k.w.died;
      if ((flags & SF_SIG_ENDED) && credit && !(flags & SF_SIG_UNRESOLVED)) {
        float oc = 0.f;  // (a select per code: the weights stay kernel arguments, no indexed copy of them)
#pragma unroll
        for (int j = 0; j < 8; ++j) oc = (outcome & 7) == j ? k.w.outcome[j] : oc;
        r = r + oc;
      }
    }
    sig_g(k.reward)[i] = r;
  }
}

}  // namespace sf
