// sf_policy_tail.hpp — the layers behind the convolutions (HIP only; sf_policy.hip includes it and launches them):
//   k_norm, k_gru0, k_gru1, k_res, k_heads, k_reward_head   one wavefront per agent row, between the separate GEMMs
//   k_tail<REWARD>                                           all of them and their matrix products in one launch
//   k_reset_memory, k_act                                    the recurrent state and the draw of an action
#pragma once
#include <cmath>

#include "sf_policy_gemm.hpp"

namespace sfp {

// ---------------------------------------------------------------------------------------------------------
// Row kernels: one wavefront per agent, lane l owns elements l, l+64, l+128 (< 160) of a 160-vector.
// ---------------------------------------------------------------------------------------------------------
__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
struct Row3 {
  float v[3];
};
__device__ inline Row3 row_load(const float *p, int l) {
  Row3 r;
  r.v[0] = p[l], r.v[1] = p[l + 64], r.v[2] = (l < HID - 128) ? p[l + 128] : 0.f;
  return r;
}
__device__ inline void row_store(float *p, int l, const Row3 &r) {
  p[l] = r.v[0], p[l + 64] = r.v[1];
  if (l < HID - 128) p[l + 128] = r.v[2];
}
// x * 160 / (sum|x| + 1e-8)   Modules.hpp:43,46,108,112,126,130
__device__ inline Row3 row_norm(const Row3 &x) {
  const float s = wave_sum(fabsf(x.v[0]) + fabsf(x.v[1]) + fabsf(x.v[2])) + 1e-8f;
  Row3 y;
#pragma unroll
  for (int i = 0; i < 3; ++i) y.v[i] = x.v[i] * (float)HID / s;
  return y;
}
__device__ inline float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }
// the f32 log of an f32, rounded once (the device's logf was two f32 steps from that on half of the reward tests' inputs; one
// lane per agent takes it: the f64 path costs nothing that shows); log_f32(0) = -inf
__device__ inline float log_f32(float x) { return (float)log((double)x); }

// torch GRU cell, gate order r,z,n; gi = W_ih x + b_ih, gh = W_hh h + b_hh (both from k_gemm):
//   r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r * gh_n), h' = (1 - z) * n + z * h
__device__ inline Row3 gru_cell(const float *gi, const float *gh, const Row3 &h, int l) {
  Row3 o;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int e = l + 64 * i;
    if (e < HID) {
      const float r = sigmoidf_(gi[e] + gh[e]);
      const float z = sigmoidf_(gi[HID + e] + gh[HID + e]);
      const float n = tanhf(gi[2 * HID + e] + r * gh[2 * HID + e]);
      o.v[i] = (1.f - z) * n + z * h.v[i];
    } else {
      o.v[i] = 0.f;
    }
  }
  return o;
}

#define SFP_ROW_PROLOGUE            \
  const int l = threadIdx.x & 63;   \
  const int a = blockIdx.x * 4 + (threadIdx.x >> 6); \
  if (a >= agents) return;

__global__ __launch_bounds__(256) void k_norm(const float *x, float *y, float *y2, int agents) {  // y2: optional copy
  SFP_ROW_PROLOGUE
  const Row3 r = row_norm(row_load(x + (size_t)a * HID, l));
  row_store(y + (size_t)a * HID, l, r);
  if (y2) row_store(y2 + (size_t)a * HID, l, r);
}

// gru0 + the assembly of `combined` (Modules.hpp:110-123): comb[0:160] = norm(h0') + feat_n,
// comb[160:329] = norm(pov), comb[329:352] = 0 (K padding)
// action_in (a reward model, RewardNet.hpp:162 update_actions(action) in front of the backbone): the one-hot is that of the
// action given — outside [0, 9): "no action" — and is stored as the agent's action_input; null: the stored row is read
__global__ __launch_bounds__(256) void k_gru0(const float *gi, const float *gh, float *h, const float *feat_n,
                                              const float *obs, float *action_input, const int32_t *action_in, float *comb, int agents) {
  SFP_ROW_PROLOGUE
  int given = 0;
  if (action_in) {
    given = action_in[a];
    given = (uint32_t)given < (uint32_t)ACT ? given : 0;
    if (l < ACT) action_input[(size_t)a * ACT + l] = (l == given) ? 1.f : 0.f;
  }
  float *hp = h + (size_t)a * HID;
  const Row3 hn = gru_cell(gi + (size_t)a * G3, gh + (size_t)a * G3, row_load(hp, l), l);
  row_store(hp, l, hn);
  const Row3 on = row_norm(hn), f = row_load(feat_n + (size_t)a * HID, l);
  Row3 c;
#pragma unroll
  for (int i = 0; i < 3; ++i) c.v[i] = on.v[i] + f.v[i];
  float *cp = comb + (size_t)a * COMB_PAD;
  row_store(cp, l, c);
  // pov: cells (-1,0) (0,-1) (0,0) (0,1) (1,0) around the centre, 32 channels each, then the action one-hot
  const float *op = obs + (size_t)a * OBS_F;
  float pv[3];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int e = l + 64 * i;
    float v = 0.f;
    if (e < 5 * OBS_C) {
      const int cell = e >> 5, ch = e & 31;
      const int dy = (cell == 0) ? -1 : (cell == 4) ? 1 : 0;
      const int dx = (cell == 1) ? -1 : (cell == 3) ? 1 : 0;
      v = op[(size_t)ch * OBS_W * OBS_W + (OBS_W / 2 + dy) * OBS_W + (OBS_W / 2 + dx)];
    } else if (e < POV) {
      v = action_in ? ((e - 5 * OBS_C == given) ? 1.f : 0.f) : action_input[(size_t)a * ACT + (e - 5 * OBS_C)];
    }
    pv[i] = v;
    s += fabsf(v);
  }
  s = wave_sum(s) + 1e-8f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int e = l + 64 * i;
    if (e < COMB_PAD - HID) cp[HID + e] = (e < POV) ? pv[i] * (float)HID / s : 0.f;
  }
}

// gru1 + residual (Modules.hpp:128-131): out = norm(h1') + gated_n
__global__ __launch_bounds__(256) void k_gru1(const float *gi, const float *gh, float *h, const float *gated_n,
                                              float *out, int agents) {
  SFP_ROW_PROLOGUE
  float *hp = h + (size_t)a * HID;
  const Row3 hn = gru_cell(gi + (size_t)a * G3, gh + (size_t)a * G3, row_load(hp, l), l);
  row_store(hp, l, hn);
  const Row3 on = row_norm(hn), gn = row_load(gated_n + (size_t)a * HID, l);
  Row3 o;
#pragma unroll
  for (int i = 0; i < 3; ++i) o.v[i] = on.v[i] + gn.v[i];
  row_store(out + (size_t)a * HID, l, o);
}

// one ResB layer after its Linear (Modules.hpp:45-46): x <- norm(relu(lin) + x); blockIdx.y picks the head
__global__ __launch_bounds__(256) void k_res(const float *lin0, float *x0, const float *lin1, float *x1, int agents) {
  SFP_ROW_PROLOGUE
  const float *lin = blockIdx.y ? lin1 : lin0;
  float *x = blockIdx.y ? x1 : x0;
  float *xp = x + (size_t)a * HID;
  const Row3 y = row_load(lin + (size_t)a * HID, l), xv = row_load(xp, l);
  Row3 r;
#pragma unroll
  for (int i = 0; i < 3; ++i) r.v[i] = fmaxf(y.v[i], 0.f) + xv.v[i];
  row_store(xp, l, row_norm(r));
}

// the two output layers (Modules.hpp:172-175): p = softmax(W_p x_p + b_p) + 1e-8, v = sigmoid(W_v x_v + b_v)
__global__ __launch_bounds__(256) void k_heads(const float *xp, const float *xv, const float *wp, const float *bp,
                                               const float *wv, const float *bv, float *probs, float *value,
                                               int agents) {
  SFP_ROW_PROLOGUE
  const Row3 p = row_load(xp + (size_t)a * HID, l), v = row_load(xv + (size_t)a * HID, l);
  float logit[ACT];
#pragma unroll
  for (int k = 0; k < ACT; ++k) {
    const Row3 wr = row_load(wp + k * HID, l);
    logit[k] = wave_sum(p.v[0] * wr.v[0] + p.v[1] * wr.v[1] + p.v[2] * wr.v[2]) + bp[k];
  }
  const Row3 wr = row_load(wv, l);
  const float val = wave_sum(v.v[0] * wr.v[0] + v.v[1] * wr.v[1] + v.v[2] * wr.v[2]) + bv[0];
  float mx = logit[0];
#pragma unroll
  for (int k = 1; k < ACT; ++k) mx = fmaxf(mx, logit[k]);
  float e[ACT], s = 0.f;
#pragma unroll
  for (int k = 0; k < ACT; ++k) e[k] = expf(logit[k] - mx), s += e[k];
  if (l < ACT) {
    float mine = e[0];
#pragma unroll
    for (int k = 1; k < ACT; ++k) mine = (l == k) ? e[k] : mine;
    probs[(size_t)a * ACT + l] = mine / s + 1e-8f;
  }
  if (l == 0) value[a] = sigmoidf_(val);
}

// the reward model's output layer (RewardNet.hpp:165, :257): D = sigmoid(W x + b), reward = log D — the log of the f32 D as
// stored (D == 0: -inf, as torch::log gives).  Either output may be null.
__global__ __launch_bounds__(256) void k_reward_head(const float *x, const float *wv, const float *bv, float *disc, float *reward,
                                                     int agents) {
  SFP_ROW_PROLOGUE
  const Row3 v = row_load(x + (size_t)a * HID, l), wr = row_load(wv, l);
  const float d = sigmoidf_(wave_sum(v.v[0] * wr.v[0] + v.v[1] * wr.v[1] + v.v[2] * wr.v[2]) + bv[0]);
  if (l == 0) {
    if (disc) disc[a] = d;
    if (reward) reward[a] = log_f32(d);
  }
}

// ---------------------------------------------------------------------------------------------------------
// k_tail: everything behind conv2 in one launch (conv3, both GRU cells, combined_processor, the two heads: 7 matrix
// and 9 row launches before).  One 16-wave workgroup per 16 agents; the activations of those agents stay in LDS from
// layer to layer, the weights (3 MB in all) stream from L2 once per workgroup straight into MFMA operands.
//   matrix steps  v_mfma_f32_16x16x4_f32 (f32 in, f32 accumulate: the same fmaf-chain arithmetic as k_gemm): a wave
//                 owns 16-column tiles of the [16 agents][N] output; per 16 k it reads one float4 of its agent row
//                 from LDS and one float4 of its weight row from global memory (lane l: row / column l & 15,
//                 k = 4 (l >> 4) + j in MFMA j — any fixed permutation of k works as long as both operands use it),
//                 the weights of the wave's NEXT tile on their way while this one is multiplied (ts_tile160)
//   row steps     one wave per agent, the row kernels' own functions (row_norm, gru_cell) on LDS rows
// LDS rows that feed a matrix step are K + 8 floats apart: conflict-free for the ds_read_b128 lane groups.
// ---------------------------------------------------------------------------------------------------------
typedef float f32x4v __attribute__((ext_vector_type(4)));
constexpr int TL_R = 16, TL_T = 1024;
constexpr int TL_LD = HID + 8, TL_LDC = COMB_PAD + 8, TL_LDX = 9 * HID + 8;  // 168, 360, 1448
constexpr int TL_A = 0;                              // region A: conv3's input rows, later gi / gh / comb, later lin0 / lin1 / x0 / x1
constexpr int TL_GI = TL_A, TL_GH = TL_A + TL_R * G3, TL_COMB = TL_A + 2 * TL_R * G3;
constexpr int TL_LIN0 = TL_A, TL_LIN1 = TL_A + TL_R * TL_LD, TL_X0 = TL_COMB, TL_X1 = TL_COMB + TL_R * TL_LD;
constexpr int TL_B0 = TL_A + TL_R * TL_LDX;          // feat_n
constexpr int TL_B1 = TL_B0 + TL_R * TL_LD;          // h0, then h1
constexpr int TL_B2 = TL_B1 + TL_R * TL_LD;          // gated_n
constexpr int TL_Y0 = TL_B2 + TL_R * TL_LD;          // feat, then gated
constexpr int TL_PV = TL_Y0 + TL_R * TL_LD;          // raw pov values and h1, fetched at the start
constexpr int TL_LDP = 192;                          // a pov row: 169 values, three per lane
constexpr int TL_H1 = TL_PV + TL_R * TL_LDP;
constexpr int TL_FLOATS = TL_H1 + TL_R * TL_LD;
constexpr int TL_LDS = TL_FLOATS * 4;                // 158 720 bytes
static_assert(TL_COMB + TL_R * TL_LDC <= TL_B0 && TL_X1 + TL_R * TL_LD <= TL_B0, "region A holds its tenants");

__device__ inline uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct ActStr {
  char c[ACT];
};

// The tail of Agent::predict() (Agent.hpp:200-216) for agent a: v[0] = 0.5, the rest scaled to 0.5 in all, one draw from
// discrete_distribution(v) — or the arg-max.  One body for k_act and for k_tail's last lines (sf_policy_predict_sparse).
__device__ inline int act_pick(float (&v)[ACT], uint64_t seed, uint64_t draw, int greedy, int a) {
  const float sc = 0.5f / (1.f - v[0] + 1e-5f);
#pragma unroll
  for (int k = 1; k < ACT; ++k) v[k] *= sc;
  v[0] = 0.5f;
  int pick = 0;
  if (greedy) {
#pragma unroll
    for (int k = 1; k < ACT; ++k)
      if (v[k] > v[pick]) pick = k;
  } else {
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < ACT; ++k) tot += v[k];
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

struct TailArgs {
  const float *act2, *obs, *pov, *conv3_w;  // pov: the 160 centre values as a dense row per agent, or null (gather them from obs)
  const float *feat;                        // the folded convolution stack's output (k_feat_*): conv3 is then not run here
  const float *gru_w_ih[2], *gru_w_hh[2], *gru_b_ih[2], *gru_b_hh[2];
  const float *comb_w, *comb_b;
  const float *res_w[2][3], *res_b[2][3], *head_w[2], *head_b[2];
  float *h[2];
  float *action_input;  // (read at the start; written by the folded sf_policy_act)
  float *probs, *value;
  int agents;
  // sf_policy_predict_sparse: the calls around the forward folded into it
  //   before: sf_policy_reset_memory — an agent whose mask byte, or whose arena's word, is non-zero starts from h = 0 and
  //           the "no action" one-hot instead of what is stored
  //   after:  sf_policy_act — the draw, the one-hot for the next call, the command char (act != 0)
  const uint8_t *reset_mask;   // [agents] or null
  const int32_t *reset_words;  // word (a / reset_group) * reset_stride, or null (sf_done_view_device)
  int reset_stride, reset_group;
  int act, greedy;
  ActStr as;
  uint64_t seed, draw;
  uint8_t *cmd;
  int32_t *action;
  // k_tail<true>, a reward model (sf_reward_*): the action just drawn, whose one-hot is this call's action_input
  // (RewardNet.hpp:162), and where log D goes (D itself goes to `value`); either output may be null
  const int32_t *action_in;
  float *reward;
};

// out[r][n0 + c] = bias[n0 + c] + sum_k in[r][k] * W[n0 + c][k] for the 16 agents r and 16 columns c of one tile
template <int K>
__device__ inline void tail_tile(const float *in, int ldi, const float *W, const float *bias, float *out, int ldo, int n0, int l) {
  constexpr int STEPS = K / 16, U = 8, NBATCH = (STEPS + U - 1) / U;  // weight loads in batches of 8 float4, two batches in flight
  const int row = l & 15, g = l >> 4;
  const float *ap = in + row * ldi + 4 * g;
  const float *wp = W + (size_t)(n0 + row) * K + 4 * g;
  f32x4v acc = {0.f, 0.f, 0.f, 0.f};
  f32x4 wq[2][U];
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (u < STEPS) wq[0][u] = ldg4(wp + 16 * u);
#pragma unroll
  for (int b = 0; b < NBATCH; ++b) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if ((b + 1) * U + u < STEPS) wq[(b + 1) & 1][u] = ldg4(wp + 16 * ((b + 1) * U + u));
    __builtin_amdgcn_sched_barrier(0);  // (the compiler would sink every load to just in front of its MFMAs: 2 in flight)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (b * U + u >= STEPS) continue;
      const f32x4 a4 = *reinterpret_cast<const f32x4 *>(ap + 16 * (b * U + u));
      const f32x4 w4 = wq[b & 1][u];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, w4.x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, w4.y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, w4.z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, w4.w, acc, 0, 0, 0);
    }
  }
  const float bv = bias ? bias[n0 + row] : 0.f;  // lane l holds column n0 + (l & 15) of agents 4 g .. 4 g + 3
#pragma unroll
  for (int r = 0; r < 4; ++r) out[(4 * g + r) * ldo + n0 + row] = acc[r] + bv;
}

// ---- k_tail's weight stream ----------------------------------------------------------------------------------
// A wave's tiles follow each other — inside a layer and from layer to layer — and the weights do not depend on anything
// the kernel computes.  They are fetched in batches of five k-steps (of 16: a K = 160 tile is two batches) into two
// register buffers, always one batch ahead of the MFMAs: the second batch of a tile while its first is multiplied, the
// first batch of the wave's NEXT tile — of this layer or, across the barriers and the row steps in between, of the next
// one — while its second is.  What stays exposed is the very first batch of the kernel.  Same products in the same
// order as tail_tile: the results are the same bits.
constexpr int TS_U = 5;
struct TsBuf {  // (passed and returned by value: every element stays a register)
  f32x4 v[TS_U];
};
// The streamed weights are stored in the order the loads take them (upload_tiles(), sf_policy_create): tile (16 output
// columns) by tile, k-step (16 inputs) by k-step, lane by lane — one k-step of a tile is 1 KB that a wave's
// global_load_dwordx4 reads as eight whole 128-byte lines.  (From the row-major matrix the same load touched sixteen
// lines, half of each, and the vector L1's tag pipe — not the L2, not the matrix pipe — set the pace of the tile phases:
// in-kernel stamps, round 4.)
__device__ inline const float *ts_wp(const float *W, int K, int n0, int l) { return W + (size_t)(n0 >> 4) * ((size_t)K * 16) + 4 * l; }
template <int N>
__device__ inline TsBuf ts_issue(TsBuf b, const float *wp, int s0) {
#pragma unroll
  for (int u = 0; u < N; ++u) b.v[u] = ldg4(wp + 256 * (s0 + u));
  return b;
}
template <int N>
__device__ inline void ts_mma(f32x4v &acc, const TsBuf &b, const float *ap, int s0) {
#pragma unroll
  for (int u = 0; u < N; ++u) {
    const f32x4 a4 = *reinterpret_cast<const f32x4 *>(ap + 16 * (s0 + u));
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.x, b.v[u].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.y, b.v[u].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.z, b.v[u].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4.w, b.v[u].w, acc, 0, 0, 0);
  }
}
__device__ inline void ts_store(const f32x4v &acc, const float *bias, float *out, int ldo, int n0, int l) {
  const int row = l & 15, g = l >> 4;
  const float bv = bias ? bias[n0 + row] : 0.f;  // lane l holds column n0 + (l & 15) of agents 4 g .. 4 g + 3
#pragma unroll
  for (int r = 0; r < 4; ++r) out[(4 * g + r) * ldo + n0 + row] = acc[r] + bv;
}
// one K = 160 tile: its first batch is already on its way in b0; `next(b0)` requests the wave's next tile's first batch
template <class Next>
__device__ inline void ts_tile160(const float *in, int ldi, const float *wp, const float *bias, float *out, int ldo, int n0, int l,
                                  TsBuf &b0, TsBuf &b1, Next next) {
  const float *ap = in + (l & 15) * ldi + 4 * (l >> 4);
  b1 = ts_issue<5>(b1, wp, 5);
  __builtin_amdgcn_sched_barrier(0);  // (the compiler would sink the loads to just in front of their MFMAs)
  f32x4v acc = {0.f, 0.f, 0.f, 0.f};
  ts_mma<5>(acc, b0, ap, 0);
  b0 = next(b0);
  __builtin_amdgcn_sched_barrier(0);
  ts_mma<5>(acc, b1, ap, 5);
  ts_store(acc, bias, out, ldo, n0, l);
}
// the K = 352 tile of combined_processor: 22 k-steps as batches of 4 4 4 4 3 3 (an even number of batches: the next tile
// starts in b0 again); its first batch (four k-steps) is already on its way in b0
template <class Next>
__device__ inline void ts_tile352(const float *in, int ldi, const float *wp, const float *bias, float *out, int ldo, int n0, int l,
                                  TsBuf &b0, TsBuf &b1, Next next) {
  static_assert(COMB_PAD == 16 * 22, "combined_processor's padded K");
  const float *ap = in + (l & 15) * ldi + 4 * (l >> 4);
  f32x4v acc = {0.f, 0.f, 0.f, 0.f};
  b1 = ts_issue<4>(b1, wp, 4);
  __builtin_amdgcn_sched_barrier(0);
  ts_mma<4>(acc, b0, ap, 0);
  b0 = ts_issue<4>(b0, wp, 8);
  __builtin_amdgcn_sched_barrier(0);
  ts_mma<4>(acc, b1, ap, 4);
  b1 = ts_issue<4>(b1, wp, 12);
  __builtin_amdgcn_sched_barrier(0);
  ts_mma<4>(acc, b0, ap, 8);
  b0 = ts_issue<3>(b0, wp, 16);
  __builtin_amdgcn_sched_barrier(0);
  ts_mma<4>(acc, b1, ap, 12);
  b1 = ts_issue<3>(b1, wp, 19);
  __builtin_amdgcn_sched_barrier(0);
  ts_mma<3>(acc, b0, ap, 16);
  b0 = next(b0);
  __builtin_amdgcn_sched_barrier(0);
  ts_mma<3>(acc, b1, ap, 19);
  ts_store(acc, bias, out, ldo, n0, l);
}

// k_tail's waves hand data to each other through LDS only: its barriers order LDS traffic and leave global loads and
// stores (weights on their way, recurrent state on its way out) in flight
__device__ __forceinline__ void tail_barrier() {
#ifdef SF_TAIL_FULL_BARRIER
  __syncthreads();
#else
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
#endif
}

#ifdef SF_DIAG_TAIL  // diagnostic build only (tools/r04_tail_stamps.py): cycles per phase of k_tail, per wave of the last launch
__device__ uint32_t sf_diag_tail[4096 * 16 * 24];  // [workgroup][wave][phase]
#define TL_STAMP(ph)                                                                                         \
  do {                                                                                                       \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();                                              \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 4096u)                                                       \
      sf_diag_tail[(blockIdx.x * 16u + (threadIdx.x >> 6)) * 24u + (ph)] = (uint32_t)(t_ - tl_last_);        \
    tl_last_ = t_;                                                                                           \
  } while (0)
#else
#define TL_STAMP(ph)
#endif
// REWARD: the instance for bot-1's RewardModel (RewardNet.hpp:138-167) — the same backbone, then ONE head.  What differs:
// the action one-hot in pov is that of t.action_in (update_actions runs in front of the backbone there) and is stored as
// the agent's action_input; the ResB layers and the output layer are the tiles of one head (slot 0 of res_w / head_w holds
// the value head: 10 tiles a layer, waves 10..15 have none and fetch nothing); the last lines store D = sigmoid and log D.
template <bool REWARD>
__global__ __launch_bounds__(TL_T) void k_tail(TailArgs t) {
  constexpr int NH = REWARD ? 1 : 2;  // heads
  extern __shared__ __attribute__((aligned(16))) float tl[];
#ifdef SF_DIAG_TAIL
  unsigned long long tl_last_ = __builtin_amdgcn_s_memtime();
#endif
  // (readfirstlane: the wave index is uniform, and the compiler should know — tile choices become scalar branches)
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), l = threadIdx.x & 63;
  const int a_raw = blockIdx.x * TL_R + w;
  const bool valid = a_raw < t.agents;
  const int a = valid ? a_raw : t.agents - 1;  // a ragged last workgroup computes its missing rows on the last agent, stores nothing
  // the weight stream (see ts_tile160): where each of this wave's tiles lives
  TsBuf b0 = {}, b1 = {};
  auto gru_wp = [&](int g, int tt) {
    const int hh = tt >= G3 / 16, n0 = 16 * (tt - hh * (G3 / 16));
    return ts_wp(hh ? t.gru_w_hh[g] : t.gru_w_ih[g], HID, n0, l);
  };
  auto res_wp = [&](int i, int tt) {
    const int hd = tt >= HID / 16, n0 = 16 * (tt - hd * (HID / 16));
    return ts_wp(t.res_w[hd][i], HID, n0, l);
  };
  // ---- the prologue's global loads: the restart flags, h0, h1, the agent's pov (5 cells x 32 channels around the centre of
  // the observation, then the action one-hot), its feature row, the first weights.  All of them are issued before the
  // first is waited for: every load is unconditional, from an address that is valid whatever the options (written behind
  // uniform branches the compiler kept them in program order, a wait after each — eight round trips, 7 k cycles of the
  // kernel's start).
  const uint8_t *fmp = t.reset_mask ? t.reset_mask + a : reinterpret_cast<const uint8_t *>(t.h[0]);
  const int32_t *fwp = t.reset_words ? t.reset_words + (size_t)(a / t.reset_group) * (size_t)t.reset_stride : reinterpret_cast<const int32_t *>(t.h[0]);
  const uint8_t fm = *fmp;
  const int32_t fw = *fwp;
  int given = 0;
  if (REWARD) given = t.action_in[a];
  Row3 h0 = row_load(t.h[0] + (size_t)a * HID, l), h1 = row_load(t.h[1] + (size_t)a * HID, l);
  float pvv[3];
  {
    const float *op = t.obs + (size_t)a * OBS_F;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int e = l + 64 * i;
      const float *src = t.action_input + (size_t)a * ACT;  // (lanes past the row: any valid address, the value is dropped)
      if (e < 5 * OBS_C) {
        const int cell = e >> 5, ch = e & 31;
        const int dy = (cell == 0) ? -1 : (cell == 4) ? 1 : 0;
        const int dx = (cell == 1) ? -1 : (cell == 3) ? 1 : 0;
        src = t.pov ? t.pov + (size_t)a * (5 * OBS_C) + e : op + (size_t)ch * OBS_W * OBS_W + (OBS_W / 2 + dy) * OBS_W + (OBS_W / 2 + dx);
      } else if (e < POV && !REWARD) {
        src += e - 5 * OBS_C;
      }
      pvv[i] = *src;
    }
  }
  const Row3 fr = row_load((t.feat ? t.feat : t.h[0]) + (size_t)a * HID, l);
  if (t.feat) b0 = ts_issue<5>(b0, gru_wp(0, w), 0);  // folded form: gru0's first tile is this wave's first
  // a restarted game's agent is a new Agent (gameplay.hpp:481): zero memory, "no action" as its last action
  const bool fresh = __builtin_amdgcn_readfirstlane((int)((t.reset_mask && fm != 0) || (t.reset_words && fw != 0))) != 0;  // (uniform over the wave)
  if (fresh) h0 = Row3{}, h1 = Row3{};
  if (REWARD) {  // an index outside [0, 9) means "no action"; update_actions leaves the one-hot in the agent's memory
    given = (uint32_t)given < (uint32_t)ACT ? given : 0;
    if (valid && l < ACT) t.action_input[(size_t)a * ACT + l] = (l == given) ? 1.f : 0.f;
  }
  if (!t.feat) {  // conv3's input (act2 row = 9 pixels x 160 channels, the K order of the permuted weight)
    const f32x4 *src = reinterpret_cast<const f32x4 *>(t.act2 + (size_t)a * (9 * HID));
    f32x4 *dst = reinterpret_cast<f32x4 *>(tl + TL_A + w * TL_LDX);
    for (int i = l; i < 9 * HID / 4; i += 64) dst[i] = src[i];
  }
  row_store(tl + TL_B1 + w * TL_LD, l, h0);
  row_store(tl + TL_H1 + w * TL_LD, l, h1);  // (used after gru0)
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int e = l + 64 * i;
    float v = 0.f;
    if (e < 5 * OBS_C) v = pvv[i];
    else if (e < POV) v = REWARD ? (e - 5 * OBS_C == given ? 1.f : 0.f) : fresh ? (e == 5 * OBS_C ? 1.f : 0.f) : pvv[i];
    tl[TL_PV + w * TL_LDP + e] = v;
  }
  if (t.feat) {  // feat_n is a row of the wave's own agent                                                     :108
    row_store(tl + TL_B0 + w * TL_LD, l, row_norm(fr));
    TL_STAMP(0);
    TL_STAMP(1);
    TL_STAMP(2);
  } else {
    TL_STAMP(0);
    tail_barrier();
    TL_STAMP(1);
    if (w < HID / 16) tail_tile<9 * HID>(tl + TL_A, TL_LDX, t.conv3_w, nullptr, tl + TL_Y0, TL_LD, 16 * w, l);  // Modules.hpp:66-71
    b0 = ts_issue<5>(b0, gru_wp(0, w), 0);
    tail_barrier();
    row_store(tl + TL_B0 + w * TL_LD, l, row_norm(row_load(tl + TL_Y0 + w * TL_LD, l)));  // feat_n :108
    TL_STAMP(2);
  }
  tail_barrier();
  TL_STAMP(3);
  // ---- gru0: gi = W_ih feat_n + b_ih, gh = W_hh h0 + b_hh (30 + 30 tiles)                          :110-113
  for (int tt = w; tt < 2 * (G3 / 16); tt += TL_R) {
    const int hh = tt >= G3 / 16, n0 = 16 * (tt - hh * (G3 / 16));
    ts_tile160(tl + (hh ? TL_B1 : TL_B0), TL_LD, gru_wp(0, tt), hh ? t.gru_b_hh[0] : t.gru_b_ih[0], tl + (hh ? TL_GH : TL_GI), G3, n0, l,
               b0, b1, [&](TsBuf b) {
                 if (tt + TL_R < 2 * (G3 / 16)) return ts_issue<5>(b, gru_wp(0, tt + TL_R), 0);
                 if (w < HID / 16) return ts_issue<4>(b, ts_wp(t.comb_w, COMB_PAD, 16 * w, l), 0);  // next: combined_processor
                 return ts_issue<5>(b, gru_wp(1, w), 0);                                            // (no tile there: gru1)
               });
  }
  TL_STAMP(4);
  tail_barrier();
  TL_STAMP(5);
  {  // gru cell, combined = [norm(h0') + feat_n | norm(pov) | 0]                                        :110-123
    const Row3 hn = gru_cell(tl + TL_GI + w * G3, tl + TL_GH + w * G3, row_load(tl + TL_B1 + w * TL_LD, l), l);
    if (valid) row_store(t.h[0] + (size_t)a * HID, l, hn);
    const Row3 on = row_norm(hn), f = row_load(tl + TL_B0 + w * TL_LD, l);
    Row3 c;
#pragma unroll
    for (int i = 0; i < 3; ++i) c.v[i] = on.v[i] + f.v[i];
    float *cp = tl + TL_COMB + w * TL_LDC;
    row_store(cp, l, c);
    float pv[3];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int e = l + 64 * i;
      pv[i] = tl[TL_PV + w * TL_LDP + e];
      s += fabsf(pv[i]);
    }
    s = wave_sum(s) + 1e-8f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int e = l + 64 * i;
      if (e < COMB_PAD - HID) cp[HID + e] = (e < POV) ? pv[i] * (float)HID / s : 0.f;
    }
    row_store(tl + TL_B1 + w * TL_LD, l, row_load(tl + TL_H1 + w * TL_LD, l));  // h1 takes h0's place
  }
  TL_STAMP(6);
  tail_barrier();
  TL_STAMP(7);
  if (w < HID / 16)                                                                                         // :125
    ts_tile352(tl + TL_COMB, TL_LDC, ts_wp(t.comb_w, COMB_PAD, 16 * w, l), t.comb_b, tl + TL_Y0, TL_LD, 16 * w, l, b0, b1,
               [&](TsBuf b) { return ts_issue<5>(b, gru_wp(1, w), 0); });
  TL_STAMP(8);
  tail_barrier();
  TL_STAMP(9);
  row_store(tl + TL_B2 + w * TL_LD, l, row_norm(row_load(tl + TL_Y0 + w * TL_LD, l)));  // gated_n :126
  TL_STAMP(10);
  tail_barrier();
  TL_STAMP(11);
  for (int tt = w; tt < 2 * (G3 / 16); tt += TL_R) {  // gru1                                             :128-131
    const int hh = tt >= G3 / 16, n0 = 16 * (tt - hh * (G3 / 16));
    ts_tile160(tl + (hh ? TL_B1 : TL_B2), TL_LD, gru_wp(1, tt), hh ? t.gru_b_hh[1] : t.gru_b_ih[1], tl + (hh ? TL_GH : TL_GI), G3, n0, l,
               b0, b1, [&](TsBuf b) {
                 if (tt + TL_R < 2 * (G3 / 16)) return ts_issue<5>(b, gru_wp(1, tt + TL_R), 0);
                 if (REWARD && w >= HID / 16) return b;   // (one head: this wave has no ResB tile)
                 return ts_issue<5>(b, res_wp(0, w), 0);  // next: the first ResB layer
               });
  }
  TL_STAMP(12);
  tail_barrier();
  TL_STAMP(13);
  {  // out = norm(h1') + gated_n; both heads start from norm(out)
    const Row3 hn = gru_cell(tl + TL_GI + w * G3, tl + TL_GH + w * G3, row_load(tl + TL_B1 + w * TL_LD, l), l);
    if (valid) row_store(t.h[1] + (size_t)a * HID, l, hn);
    const Row3 on = row_norm(hn), gn = row_load(tl + TL_B2 + w * TL_LD, l);
    Row3 o;
#pragma unroll
    for (int i = 0; i < 3; ++i) o.v[i] = on.v[i] + gn.v[i];
    const Row3 xn = row_norm(o);
    row_store(tl + TL_X0 + w * TL_LD, l, xn);
    if (NH == 2) row_store(tl + TL_X1 + w * TL_LD, l, xn);
  }
  TL_STAMP(14);
  tail_barrier();
  TL_STAMP(15);
  for (int i = 0; i < 3; ++i) {  // ResB layers of the two heads (REWARD: of the one)                      :41-48
    for (int tt = w; tt < NH * (HID / 16); tt += TL_R) {
      const int hd = tt >= HID / 16, n0 = 16 * (tt - hd * (HID / 16));
      ts_tile160(tl + (hd ? TL_X1 : TL_X0), TL_LD, res_wp(i, tt), t.res_b[hd][i], tl + (hd ? TL_LIN1 : TL_LIN0), TL_LD, n0, l, b0, b1,
                 [&](TsBuf b) {
                   if (tt + TL_R < NH * (HID / 16)) return ts_issue<5>(b, res_wp(i, tt + TL_R), 0);
                   if (i < 2) return ts_issue<5>(b, res_wp(i + 1, w), 0);
                   if (w < NH) return ts_issue<5>(b, ts_wp(t.head_w[w], HID, 0, l), 0);  // next: the output layers
                   return b;
                 });
    }
    TL_STAMP(16);
    tail_barrier();
    TL_STAMP(17);
#pragma unroll
    for (int hd = 0; hd < NH; ++hd) {
      float *xp = tl + (hd ? TL_X1 : TL_X0) + w * TL_LD;
      const Row3 y = row_load(tl + (hd ? TL_LIN1 : TL_LIN0) + w * TL_LD, l), xv = row_load(xp, l);
      Row3 r;
#pragma unroll
      for (int q = 0; q < 3; ++q) r.v[q] = fmaxf(y.v[q], 0.f) + xv.v[q];
      row_store(xp, l, row_norm(r));
    }
    TL_STAMP(18);
    tail_barrier();
    TL_STAMP(19);
  }
  // p = softmax(W_p x_p + b_p) + 1e-8, v = sigmoid(W_v x_v + b_v)                                           :172-175
  // (the two output layers as one MFMA tile each: weights padded with zero rows to 16 columns)
  if (w < NH)
    ts_tile160(tl + (w ? TL_X1 : TL_X0), TL_LD, ts_wp(t.head_w[w], HID, 0, l), t.head_b[w], tl + (w ? TL_LIN1 : TL_LIN0), TL_LD, 0, l, b0, b1,
               [&](TsBuf b) { return b; });
  TL_STAMP(20);
  tail_barrier();
  TL_STAMP(21);
  if (REWARD) {  // D = sigmoid(value head), reward = log of the f32 D (D == 0: -inf)     RewardNet.hpp:165, :257
    if (valid && l == 0) {
      const float d = sigmoidf_(tl[TL_LIN0 + w * TL_LD]);
      if (t.value) t.value[a] = d;
      if (t.reward) t.reward[a] = log_f32(d);
    }
  } else if (valid) {
    const float *lg = tl + TL_LIN0 + w * TL_LD;
    float mx = lg[0];
#pragma unroll
    for (int k = 1; k < ACT; ++k) mx = fmaxf(mx, lg[k]);
    float s = 0.f, mine = 0.f;
#pragma unroll
    for (int k = 0; k < ACT; ++k) {
      const float e = expf(lg[k] - mx);
      s += e;
      mine = (l == k) ? e : mine;
    }
    const float pl = mine / s + 1e-8f;
    if (l < ACT) t.probs[(size_t)a * ACT + l] = pl;
    if (l == 0) t.value[a] = sigmoidf_(tl[TL_LIN1 + w * TL_LD]);
    if (t.act) {  // sf_policy_act on the probabilities just stored (lanes 0..8 hold them)
      float v[ACT];
#pragma unroll
      for (int k = 0; k < ACT; ++k) v[k] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pl), k));
      const int pick = act_pick(v, t.seed, t.draw, t.greedy, a);
      if (l < ACT) t.action_input[(size_t)a * ACT + l] = (l == pick) ? 1.f : 0.f;
      if (l == 0) {
        char c = t.as.c[0];
#pragma unroll
        for (int k = 1; k < ACT; ++k) c = (pick == k) ? t.as.c[k] : c;  // (a chain of selects: no indexed copy of the argument)
        t.cmd[a] = (uint8_t)c;
        if (t.action) t.action[a] = pick;
      }
    }
  }
  TL_STAMP(22);
#ifdef SF_DIAG_TAIL
  if ((threadIdx.x & 63) == 0 && blockIdx.x < 4096u)  // HW_ID: which SIMD / CU this wave ran on
    sf_diag_tail[(blockIdx.x * 16u + (threadIdx.x >> 6)) * 24u + 23u] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
#endif
}

__global__ void k_reset_memory(float *h0, float *h1, float *action_input, const uint8_t *mask, int agents) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int a = i / HID, e = i - a * HID;
  if (a >= agents || (mask && !mask[a])) return;
  h0[i] = 0.f, h1[i] = 0.f;
  if (e < ACT) action_input[(size_t)a * ACT + e] = (e == 0) ? 1.f : 0.f;
}

// Agent::predict tail + Agent::update (Agent.hpp:200-222)
__global__ void k_act(const float *probs, float *action_input, ActStr as, uint64_t seed, uint64_t draw, int greedy,
                      uint8_t *cmd, int32_t *action, int agents) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= agents) return;
  float v[ACT];
#pragma unroll
  for (int k = 0; k < ACT; ++k) v[k] = probs[(size_t)a * ACT + k];
  const int pick = act_pick(v, seed, draw, greedy, a);
#pragma unroll
  for (int k = 0; k < ACT; ++k) action_input[(size_t)a * ACT + k] = (k == pick) ? 1.f : 0.f;
  cmd[a] = (uint8_t)as.c[pick];
  if (action) action[a] = pick;
}

}  // namespace sfp
