// sf_policy.hip — batched on-device evaluation of the reference's bot network.
//
// What is computed, per agent, is AgentModel::forward of StrikeForce-client/bots/bot-0.5/Modules.hpp:54-179:
//   GameCNN (4x Conv2d 3x3 stride 2, no bias, no activation; 32->160 channels; 31->15->7->3->1)   :54-72
//   Backbone: L1-style normalisations x*160/(sum|x|+1e-8), gru0, "pov" (5 centre cells x 32 channels + last
//   action one-hot), Linear(329->160), gru1 with a residual                                        :106-134
//   heads: ResB(160, 3) + Linear(160->9) -> softmax + 1e-8; ResB + Linear(160->1) -> sigmoid         :30-49,169-178
// The reference runs it with batch 1 on the host; here a "row" is one agent and all matrix work is f32 MFMA
// (v_mfma_f32_32x32x2_f32: f32 in, f32 accumulate, bit-for-bit a k-ordered fmaf chain), so results differ from
// libtorch only by summation order.
// bot-1's RewardModel (bots/bot-1/RewardNet.hpp:138-167: the same backbone, the value head alone, the action of this tick in
// pov, log of the output) is a second kind of the same object: sf_reward_*, k_tail<true>.
//
// Kernels
//   k_gemm<WAVES, MODE>   C[M][N] = A[M][K] * W[N][K]^T (+ bias), LDS-tiled, 32 rows x 160 columns per wave
//                         (5 accumulator tiles of 32x32; or 5 waves x 1 tile when M is small), K tile 16 or 32,
//                         global->register prefetch, double-buffered LDS, operand fragments read one product ahead.
//                         MODE selects how a row of A is addressed: a dense row, or the im2col row of a 3x3/stride-2
//                         convolution gathered on the fly from an NHWC activation (conv1..3) or from the NCHW
//                         observation buffer (conv0).  Activations between the convolutions are kept NHWC, which is
//                         simply the row-major C of the previous GEMM; the host permutes conv1..3's weights to the
//                         matching (ky, kx, cin) K-order once at load time.
//   k_*                   one wavefront per agent row for the 160-wide normalisations, the GRU gate math, the
//                         residual blocks' relu+skip and the two heads.
//
// The kernels are in sf_policy_gemm.hpp, sf_policy_conv.hpp and sf_policy_tail.hpp; the weight layouts that the host
// prepares for them are in sf_policy_stage.hpp (no HIP: tested on the CPU).  sf_policy_load.hpp builds the same layouts on
// the device from device pointers (sf_policy_load_weights).  This file is the host side and the C ABI.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/strikeforce_policy.h"
#include "sf_host.hpp"
#include "sf_policy_conv.hpp"
#include "sf_policy_gemm.hpp"
#include "sf_policy_stage.hpp"
#include "sf_policy_tail.hpp"
#include "sf_policy_mask.hpp"
#include "sf_rollout.hpp"
#include "sf_rollout_gae.hpp"
#include "sf_rollout_dense.hpp"

namespace sfp {

using sf::fail;

static_assert(SPLIT_BN == BN && SPLIT_BK == B3_BK, "split_weights builds the image k_gemm_b3 reads");

#define SFP_HIP(call)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) return sf::fail(SF_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)
// passes on a failure that has set sf_last_error already
#define SFP_RC(x)                   \
  do {                              \
    if (const int rc_ = (x)) return rc_; \
  } while (0)

// an SF_POLICY_* / SF_DIAG_* switch: set and starting with `ch` (ch = 0: set at all)
static bool env_flag(const char *name, char ch) {
  const char *e = std::getenv(name);
  return e && (!ch || e[0] == ch);
}
template <class K>
static bool allow_lds(K *kernel, size_t bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

struct Policy {
  int device = 0, max_agents = 0;
  // sf_reward_create: bot-1's RewardModel (RewardNet.hpp:138-167) — the same backbone and ONE head, kept in slot 0 of
  // res_w / res_b / head_w / head_b (slot 1 stays empty); evaluated by sf_reward_forward / sf_reward_sparse only
  bool reward = false;
  hipStream_t stream = nullptr;
  uint64_t draws = 0;
  // parameters
  float *conv0_wt = nullptr;  // conv0 weights as [c][ky][kx][n] for k_conv0_sparse
  bool dense_conv0 = false;   // SF_POLICY_DENSE_CONV0=1: the implicit-GEMM conv0 instead (A/B, tests)
  void *conv_w3[4] = {};      // conv1, conv2: the weights split into bf16 hi / mid / lo parts for k_gemm_b3
  bool f32_conv = false;      // SF_POLICY_F32_CONV=1: conv1, conv2 on the f32 matrix pipe instead (A/B, tests)
  uint32_t *d_overflows = nullptr;  // sf_policy_forward_sparse: agents whose list did not fit since the last query
  bool fused_tail = true;     // SF_POLICY_FUSED_TAIL=0: the layers behind conv2 as 16 separate launches instead (A/B, tests)
  float *fold = nullptr;      // F: the four convolutions composed into one matrix (k_fold), [FD_ROWS][160]
  bool folded = true;         // SF_POLICY_LAYERED=1: the four convolutions one after the other instead (cross-check, tests)
  float *conv_w[4] = {}, *gru_w_ih[2] = {}, *gru_w_hh[2] = {}, *gru_b_ih[2] = {}, *gru_b_hh[2] = {};
  float *comb_w = nullptr, *comb_b = nullptr;
  float *res_w[2][3] = {}, *res_b[2][3] = {}, *head_w[2] = {}, *head_b[2] = {};  // [0] policy, [1] value (reward model: [0] value)
  float *head_w16[2] = {}, *head_b16[2] = {};  // the same padded with zero rows to one 16-column MFMA tile (k_tail)
  // k_tail's copies of its matrices in the order its weight stream reads them (stage_tiles), ONE block in the order of use
  // (2.09 MB)
  float *tail_w = nullptr;
  size_t gru_w_ih_t[2] = {}, gru_w_hh_t[2] = {}, comb_w_t = 0, res_w_t[2][3] = {}, head_w16_t[2] = {};  // offsets in floats
  // per-agent state and scratch
  float *h[2] = {}, *action_input = nullptr;
  float *act[3] = {};  // NHWC conv outputs 15x15, 7x7, 3x3
  float *feat = nullptr, *feat_n = nullptr, *gi = nullptr, *gh = nullptr, *comb = nullptr, *gated = nullptr,
        *gated_n = nullptr, *out = nullptr, *x[2] = {}, *lin[2] = {};
  std::vector<void *> owned;
  // sf_policy_load_weights: the fold's f64 workspace (allocated by the first load of a folded object, in `owned`);
  // sf_policy_weights_digest: its result buffer (allocated by the first query)
  double *fold_ws[4] = {};
  unsigned long long *d_digest = nullptr;
  // timing of the matrix launches: an event pair and a kind per launch, the flop per kind.  Kinds: 0 k_gemm (f32 MFMA),
  // 1 k_gemm_b3 (bf16 split), 2 the convolutions on the non-zeros (k_feat_*, k_conv0_sparse<true>), 3 k_tail
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  std::vector<char> event_kind;
  size_t used_events = 0;
  double flop_kind[4] = {0, 0, 0, 0};

  ~Policy() {
    for (void *p : owned) (void)hipFree(p);
    for (auto &ev : events) (void)hipEventDestroy(ev.first), (void)hipEventDestroy(ev.second);
  }
  int dalloc(float **p, size_t floats) {
    void *d = nullptr;
    if (hipMalloc(&d, floats * sizeof(float)) != hipSuccess) return fail(SF_ERR_MEMORY, "hipMalloc failed (policy)");
    owned.push_back(d);
    *p = (float *)d;
    return SF_OK;
  }
  int upload(float **p, const float *src, size_t floats) {
    if (!src) return fail(SF_ERR_ARG, "sf_policy_weights has a null pointer");
    SFP_RC(dalloc(p, floats));
    SFP_HIP(hipMemcpy(*p, src, floats * sizeof(float), hipMemcpyHostToDevice));
    return SF_OK;
  }

  // Resident blocks of the large-M shape: its 76 KB of LDS pins two 4-wave blocks on each CU (set in create())
  int sk_blocks = 512;
  float *part = nullptr;  // [sk_blocks][2][128*160]

  // The work split of both GEMM forms: one run per row tile of BM rows (the classic decomposition), or, for a one-strip
  // product with at least four units per resident block, `resident` equal runs and k_gemm_fixup for the tiles they cut.
  // launch(g, G) starts the G x N/160 blocks of the product itself.
  template <int BM, class Launch>
  void launch_runs(Gemm g, int KT, int resident, bool may_cut, Launch launch) {
    g.ntiles = (g.M + BM - 1) / BM;
    g.part = part;
    const long units = (long)g.ntiles * KT;
    int G = g.ntiles;
    if (g.N == BN && may_cut && units >= 4L * resident) G = resident;
    g.unit_base = (int)(units / G), g.unit_rem = (int)(units % G);
    launch(g, (unsigned)G);
    if (G != g.ntiles)
      hipLaunchKernelGGL((k_gemm_fixup<BM>), dim3((unsigned)(G - 1), (unsigned)(g.N / BN)), dim3(256), 0, stream, g, KT, G);
  }
  template <int WM, int WN, int BKT, int MODE>
  void launch_t(const Gemm &g) {  // (both block shapes cut: conv3 is the small-M case; a pair of products never does)
    launch_runs<WM * 32>(g, g.K / BKT, sk_blocks, !g.A2, [this](const Gemm &s, unsigned G) {
      hipLaunchKernelGGL((k_gemm<WM, WN, BKT, MODE>), dim3(G, (unsigned)(s.N / BN), s.A2 ? 2u : 1u), dim3(WM * WN * 64), 0, stream, s);
    });
  }
  // the bf16-split form: one 8-wave block per CU
  template <int MODE>
  void launch_b3(const Gemm &g) {
    launch_runs<B3_BM>(g, g.K / B3_BK, sk_blocks / 2, true, [this](const Gemm &s, unsigned G) {
      hipLaunchKernelGGL((k_gemm_b3<MODE>), dim3(G, (unsigned)(s.N / BN)), dim3(B3_T), B3_LDS, stream, s);
    });
  }
  template <int MODE>
  void launch_m(const Gemm &g) {
    if (g.W3 && MODE != MODE_NCHW) launch_b3<MODE == MODE_NCHW ? MODE_NHWC : MODE>(g);
    else if (g.M >= 16384) launch_t<4, 1, 32, MODE>(g);
    else launch_t<1, 5, 32, MODE>(g);
  }
  // timing of one launch of `kind`: records the start event, returns the end event to record behind the launch
  int time_begin(double fl, int kind, hipEvent_t *e1) {
    *e1 = nullptr;
    if (!timing) return SF_OK;
    if (used_events == events.size()) {
      hipEvent_t a, b;
      SFP_HIP(hipEventCreate(&a));
      SFP_HIP(hipEventCreate(&b));
      events.emplace_back(a, b);
      event_kind.push_back(0);
    }
    const hipEvent_t e0 = events[used_events].first;
    *e1 = events[used_events].second;
    event_kind[used_events] = (char)kind;
    ++used_events;
    flop_kind[kind] += fl;
    SFP_HIP(hipEventRecord(e0, stream));
    return SF_OK;
  }
  // waits for the stream, sums the timed launches per kind, forgets them and arms (or disarms) the timing
  int take_times(int enable, float ms[4], double flop[4], int32_t launches[4]) {
    SFP_HIP(hipSetDevice(device));
    SFP_HIP(hipStreamSynchronize(stream));
    for (int k = 0; k < 4; ++k) ms[k] = 0.f, flop[k] = flop_kind[k], launches[k] = 0;
    for (size_t i = 0; i < used_events; ++i) {
      float t = 0.f;
      SFP_HIP(hipEventElapsedTime(&t, events[i].first, events[i].second));
      ms[(int)event_kind[i]] += t;
      ++launches[(int)event_kind[i]];
    }
    for (double &fl : flop_kind) fl = 0;
    used_events = 0;
    timing = enable != 0;
    return SF_OK;
  }
  int gemm(const Gemm &g, int mode) {
    if (g.K % 32 || g.N % BN || g.M < 1) return fail(SF_ERR_ARG, "policy gemm: unsupported shape");
    hipEvent_t e1 = nullptr;
    SFP_RC(time_begin(2.0 * g.M * g.N * g.K * (g.A2 ? 2 : 1), g.W3 && mode != MODE_NCHW ? 1 : 0, &e1));
    switch (mode) {
      case MODE_DENSE: launch_m<MODE_DENSE>(g); break;
      case MODE_NHWC: launch_m<MODE_NHWC>(g); break;
      default: launch_m<MODE_NCHW>(g); break;
    }
    SFP_HIP(hipGetLastError());
    if (e1) SFP_HIP(hipEventRecord(e1, stream));
    return SF_OK;
  }
  static Gemm dense_args(const float *A, int lda, const float *W, const float *bias, float *C, int ldc, int M, int N, int K) {
    Gemm g{};
    g.A = A, g.W = W, g.bias = bias, g.C = C;
    g.M = M, g.N = N, g.K = K, g.lda = lda, g.ldc = ldc;
    return g;
  }
  // W3: W split on the device (sf_policy_gemm_split)
  int dense(const float *A, int lda, const float *W, const float *bias, float *C, int ldc, int M, int N, int K, const void *W3 = nullptr) {
    Gemm g = dense_args(A, lda, W, bias, C, ldc, M, N, K);
    g.W3 = W3;
    return gemm(g, MODE_DENSE);
  }
  // two independent products of one shape in one launch
  int dense2(const float *A, const float *W, const float *bias, float *C, const float *A2, const float *W2,
             const float *bias2, float *C2, int lda, int ldc, int M, int N, int K) {
    Gemm g = dense_args(A, lda, W, bias, C, ldc, M, N, K);
    g.A2 = A2, g.W2 = W2, g.bias2 = bias2, g.C2 = C2;
    return gemm(g, MODE_DENSE);
  }
  int conv(const float *in, const float *W, float *outp, int agents, int S, int Cin, int nchw, const void *W3 = nullptr) {
    Gemm g{};
    g.S = S, g.Cin = Cin, g.So = (S - 3) / 2 + 1;
    g.A = in, g.W = W, g.C = outp;
    g.M = agents * g.So * g.So, g.N = HID, g.K = Cin * 9, g.ldc = HID;
    if (W3 && g.M >= 16384 && !f32_conv) g.W3 = W3;
    return gemm(g, nchw ? MODE_NCHW : MODE_NHWC);
  }

  // ---- GameCNN's launches (forward, sf_policy_features) ----
  // one block per agent, at most `most`
  static dim3 per_agent(int agents, int most) { return dim3((unsigned)(agents < most ? agents : most)); }
  void feat_list(int agents, const C0List &li) {
    hipLaunchKernelGGL(k_feat_list, dim3((unsigned)agents), dim3(64), 0, stream, fold, feat, agents, li);
  }
  // F on the dense observation of every agent, or (redo) of the agents whose list did not fit
  void feat_dense(const float *d_obs, float *to, int agents, const C0List *redo = nullptr) {
    hipLaunchKernelGGL(k_feat_dense, per_agent(agents, redo ? sk_blocks : 4 * sk_blocks), dim3(FD_T), 0, stream, d_obs, fold, to, agents,
                       redo ? *redo : C0List{});
  }
  template <bool LIST>
  void conv0_sparse(const float *d_obs, int agents, const C0List &li) {
    hipLaunchKernelGGL(k_conv0_sparse<LIST>, per_agent(agents, sk_blocks / 2), dim3(C0_T), C0_LDS, stream, d_obs, conv0_wt, act[0], agents, li);
  }
  // conv1 and conv2 behind conv0's act[0], and conv3 into `to` unless that is null (k_tail does it)
  int conv123(int agents, float *to) {
    SFP_RC(conv(act[0], conv_w[1], act[1], agents, 15, HID, 0, conv_w3[1]));
    SFP_RC(conv(act[1], conv_w[2], act[2], agents, 7, HID, 0, conv_w3[2]));
    return to ? conv(act[2], conv_w[3], to, agents, 3, HID, 0) : SF_OK;
  }
};

static int check_agents(Policy *p, int agents) {
  if (!p) return fail(SF_ERR_ARG, "null policy");
  if (agents < 1 || agents > p->max_agents) return fail(SF_ERR_ARG, "agents out of range for this policy");
  return SF_OK;
}

static int create(const sf_policy_weights *w, int max_agents, int device, sf_policy **out, bool reward = false) {
  if (!w || !out) return fail(SF_ERR_ARG, "null argument");
  if (w->abi_version != SF_POLICY_ABI_VERSION) return fail(SF_ERR_ARG, "sf_policy_weights.abi_version mismatch");
  if (max_agents < 1 || max_agents > (1 << 20)) return fail(SF_ERR_ARG, "max_agents must be 1..1048576");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
    return fail(SF_ERR_DEVICE, "no HIP device: the policy network has no CPU path");
  if (device < 0 || device >= n) return fail(SF_ERR_DEVICE, "device ordinal out of range");
  SFP_HIP(hipSetDevice(device));
  // (the one owner until *out has it: every return below frees the device buffers and events allocated so far)
  std::unique_ptr<Policy> p(new Policy());
  p->device = device, p->max_agents = max_agents, p->reward = reward;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
      p->sk_blocks = 2 * prop.multiProcessorCount;
  }
  for (int i = 0; i < 4; ++i)
    if (!w->conv_w[i]) return fail(SF_ERR_ARG, "conv weight is null");
  SFP_RC(p->upload(&p->conv_w[0], w->conv_w[0], (size_t)HID * OBS_C * 9));
  {
    const std::vector<float> tr = conv0_transpose(w->conv_w[0], HID, OBS_C * 9);
    SFP_RC(p->upload(&p->conv0_wt, tr.data(), tr.size()));
    p->dense_conv0 = env_flag("SF_POLICY_DENSE_CONV0", '1');
    if (!allow_lds(k_conv0_sparse<false>, C0_LDS) || !allow_lds(k_conv0_sparse<true>, C0_LDS))
      return fail(SF_ERR_DEVICE, "k_conv0_sparse needs 157 KB of LDS per workgroup");
  }
  for (int i = 1; i < 4; ++i) {
    const std::vector<float> perm = conv_permute(w->conv_w[i], HID, HID);
    SFP_RC(p->upload(&p->conv_w[i], perm.data(), perm.size()));
    if (i < 3) {
      const std::vector<uint16_t> img = split_weights(perm.data(), HID, HID * 9);
      float *d = nullptr;
      SFP_RC(p->dalloc(&d, img.size() / 2));
      SFP_HIP(hipMemcpy(d, img.data(), img.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
      p->conv_w3[i] = d;
    }
  }
  // F = conv3 o conv2 o conv1 o conv0 as one matrix (see k_fold): T3 = conv3's rows, then three transposed convolutions
  p->folded = !env_flag("SF_POLICY_LAYERED", '1');
  if (p->folded) {
    double *T[4] = {nullptr, nullptr, nullptr, nullptr};
    const int side[4] = {31, 15, 7, 3};
    const size_t elems[4] = {(size_t)HID * 31 * 31 * OBS_C, (size_t)HID * 15 * 15 * HID, (size_t)HID * 7 * 7 * HID, (size_t)HID * 9 * HID};
    bool ok = true;
    for (int i = 0; i < 4 && ok; ++i) ok = hipMalloc(reinterpret_cast<void **>(&T[i]), elems[i] * sizeof(double)) == hipSuccess;
    if (ok) ok = p->dalloc(&p->fold, (size_t)FD_ROWS * HID) == SF_OK;
    if (ok) {
      (void)hipMemset(p->fold, 0, (size_t)FD_ROWS * HID * sizeof(float));
      hipLaunchKernelGGL(k_to_f64, dim3((unsigned)((elems[3] + 255) / 256)), dim3(256), 0, nullptr, p->conv_w[3], T[3], elems[3]);
      for (int i = 2; i >= 0; --i)  // T[i]: the map from conv i's input to feat
        hipLaunchKernelGGL(k_fold, dim3((unsigned)((elems[i] + 255) / 256)), dim3(256), 0, nullptr, T[i + 1], p->conv_w[i], T[i],
                           side[i + 1], side[i], HID, i ? HID : OBS_C, i ? 1 : 0);
      hipLaunchKernelGGL(k_fold_out, dim3((unsigned)(((size_t)OBS_F * HID + 255) / 256)), dim3(256), 0, nullptr, T[0], p->fold);
      // (a launch that never started — a bad configuration — reports here, not at the synchronise: F would stay all zero)
      ok = hipGetLastError() == hipSuccess;
      ok = hipDeviceSynchronize() == hipSuccess && ok;
    }
    for (int i = 0; i < 4; ++i)  // (on every path: T is not the object's)
      if (T[i]) (void)hipFree(T[i]);
    if (!ok) return fail(SF_ERR_DEVICE, "composing the convolution stack failed");
  }
  p->f32_conv = env_flag("SF_POLICY_F32_CONV", '1');
  p->fused_tail = !env_flag("SF_POLICY_FUSED_TAIL", '0');
  if (!allow_lds(k_tail<false>, TL_LDS) || !allow_lds(k_tail<true>, TL_LDS)) return fail(SF_ERR_DEVICE, "k_tail needs 155 KB of LDS per workgroup");
  if (!allow_lds(k_gemm_b3<MODE_NHWC>, B3_LDS) || !allow_lds(k_gemm_b3<MODE_DENSE>, B3_LDS))
    return fail(SF_ERR_DEVICE, "k_gemm_b3 needs 78 KB of LDS per workgroup");
  for (int g = 0; g < 2; ++g) {
    SFP_RC(p->upload(&p->gru_w_ih[g], w->gru_w_ih[g], (size_t)G3 * HID));
    SFP_RC(p->upload(&p->gru_w_hh[g], w->gru_w_hh[g], (size_t)G3 * HID));
    SFP_RC(p->upload(&p->gru_b_ih[g], w->gru_b_ih[g], G3));
    SFP_RC(p->upload(&p->gru_b_hh[g], w->gru_b_hh[g], G3));
  }
  // k_tail's block, in the order the kernel goes through it (every matrix staged was uploaded, so checked, before)
  std::vector<float> tail;
  {
    if (!w->comb_w) return fail(SF_ERR_ARG, "combined_processor weight is null");
    const std::vector<float> pad = pad_zero(w->comb_w, HID, COMB, HID, COMB_PAD);
    SFP_RC(p->upload(&p->comb_w, pad.data(), pad.size()));
    p->gru_w_ih_t[0] = stage_tiles(tail, w->gru_w_ih[0], G3, HID);
    p->gru_w_hh_t[0] = stage_tiles(tail, w->gru_w_hh[0], G3, HID);
    p->comb_w_t = stage_tiles(tail, pad.data(), HID, COMB_PAD);
    p->gru_w_ih_t[1] = stage_tiles(tail, w->gru_w_ih[1], G3, HID);
    p->gru_w_hh_t[1] = stage_tiles(tail, w->gru_w_hh[1], G3, HID);
    SFP_RC(p->upload(&p->comb_b, w->comb_b, HID));
  }
  // head slot -> the head it holds: a reward model has the value head alone (the policy_* fields are not looked at), and
  // only its three ResB matrices and output layer enter k_tail's block
  const int heads = reward ? 1 : 2;
  for (int i = 0; i < 3; ++i)
    for (int g = 0; g < heads; ++g) {
      const bool val = reward || g;
      SFP_RC(p->upload(&p->res_w[g][i], val ? w->value_res_w[i] : w->policy_res_w[i], (size_t)HID * HID));
      p->res_w_t[g][i] = stage_tiles(tail, val ? w->value_res_w[i] : w->policy_res_w[i], HID, HID);
      SFP_RC(p->upload(&p->res_b[g][i], val ? w->value_res_b[i] : w->policy_res_b[i], HID));
    }
  for (int g = 0; g < heads; ++g) {
    const bool val = reward || g;
    const int rows = val ? 1 : ACT;
    SFP_RC(p->upload(&p->head_w[g], val ? w->value_w : w->policy_w, (size_t)rows * HID));
    SFP_RC(p->upload(&p->head_b[g], val ? w->value_b : w->policy_b, rows));
    const std::vector<float> wpad = pad_zero(val ? w->value_w : w->policy_w, rows, HID, 16, HID);
    const std::vector<float> bpad = pad_zero(val ? w->value_b : w->policy_b, rows, 1, 16, 1);
    SFP_RC(p->upload(&p->head_w16[g], wpad.data(), wpad.size()));
    p->head_w16_t[g] = stage_tiles(tail, wpad.data(), 16, HID);
    SFP_RC(p->upload(&p->head_b16[g], bpad.data(), bpad.size()));
  }
  SFP_RC(p->upload(&p->tail_w, tail.data(), tail.size()));
  const size_t B = (size_t)max_agents;
  SFP_RC(p->dalloc(&p->h[0], B * HID));
  SFP_RC(p->dalloc(&p->h[1], B * HID));
  SFP_RC(p->dalloc(&p->action_input, B * ACT));
  if (!p->folded)  // the layered path's activations (181 KB per agent)
    for (int i = 0; i < 3; ++i) SFP_RC(p->dalloc(&p->act[i], B * (i == 0 ? 225 : i == 1 ? 49 : 9) * HID));
  SFP_RC(p->dalloc(&p->feat, B * HID));
  SFP_RC(p->dalloc(&p->feat_n, B * HID));
  SFP_RC(p->dalloc(&p->gi, B * G3));
  SFP_RC(p->dalloc(&p->gh, B * G3));
  SFP_RC(p->dalloc(&p->comb, B * COMB_PAD));
  for (float **buf : {&p->gated, &p->gated_n, &p->out, &p->x[0], &p->x[1], &p->lin[0], &p->lin[1]}) SFP_RC(p->dalloc(buf, B * HID));
  SFP_RC(p->dalloc(&p->part, (size_t)p->sk_blocks * 2 * 128 * BN));
  {
    float *f = nullptr;
    SFP_RC(p->dalloc(&f, 1));
    p->d_overflows = reinterpret_cast<uint32_t *>(f);
    SFP_HIP(hipMemset(p->d_overflows, 0, sizeof(uint32_t)));
  }
  *out = reinterpret_cast<sf_policy *>(p.release());
  return sf_policy_reset_memory(*out, nullptr);
}

// One evaluation of the network, as the entry points ask for it and forward() checks it.
struct ForwardReq {
  bool reward_model;  // asked through sf_reward_*: k_tail<true>, one head, the outputs below
  // the observation: dense, or li + d_pov: its non-zeros as lists, with d_obs as the dense fallback for the agents whose
  // list did not fit (d_obs need only be valid for those: sf_observe_overflow_device)
  const float *d_obs, *d_pov;
  const C0List *li;
  float *probs, *value;  // a policy's outputs
  // memory resets folded into the call (see TailArgs)
  const uint8_t *reset_mask;
  const int32_t *reset_words;
  int reset_stride, reset_group;
  // sf_policy_predict_sparse: sf_policy_act folded into the call
  bool act;
  ActStr as;
  uint64_t seed;
  int greedy;
  uint8_t *cmd;
  int32_t *action;
  // a reward model: the action of this tick, and where D and log D go (either may be null)
  const int32_t *action_in;
  float *disc, *reward;
};
// every entry point that evaluates a network is for one kind of object
static int check_kind(const Policy *p, bool reward, const char *entry) {
  if (!p) return fail(SF_ERR_ARG, "null policy");
  if (p->reward == reward) return SF_OK;
  return fail(SF_ERR_STATE, std::string(entry) + (reward ? ": this object is a policy (sf_policy_create), not a reward model (sf_reward_create)"
                                                         : ": this object is a reward model (sf_reward_create): sf_reward_forward and sf_reward_sparse evaluate it"));
}
// the list arguments of the sparse entry points (`rest`: the other buffers an entry point counts among them)
static int check_lists(const uint32_t *keys, const float *vals, const uint32_t *counts, const float *pov, int cap, bool rest = true) {
  if (!keys || !vals || !counts || !pov || !rest || cap < 1) return fail(SF_ERR_ARG, "null buffer or cap < 1");
  // (above it the kernels' own list limit would call an agent "overflowed" whose dense row sf_observe_overflow_device,
  // which only knows cap, never wrote)
  if (cap > SF_POLICY_LIST_MAX) return fail(SF_ERR_ARG, "cap above SF_POLICY_LIST_MAX (2048)");
  return SF_OK;
}
static int check_resets(const int32_t *words, int stride, int group) {
  if (words && (stride < 1 || group < 1)) return fail(SF_ERR_ARG, "reset_stride and reset_group must be positive");
  return SF_OK;
}
static int forward(Policy *p, int agents, const ForwardReq &r) {
  SFP_RC(check_agents(p, agents));
  const bool rw = r.reward_model;
  const C0List *li = r.li;
  if (p->reward != rw) return fail(SF_ERR_STATE, "wrong kind of object for this forward");
  if ((!r.d_obs && !li) || (rw ? !r.action_in || (!r.disc && !r.reward) : !r.probs || !r.value)) return fail(SF_ERR_ARG, "null buffer");
  // (sf_policy_predict_sparse answers as the list form it is)
  if (li && !p->fused_tail)
    return fail(SF_ERR_STATE, std::string(rw ? "sf_reward_sparse" : "sf_policy_forward_sparse") + " needs the fused tail (SF_POLICY_FUSED_TAIL=0 is set)");
  SFP_HIP(hipSetDevice(p->device));
  const dim3 rg((unsigned)((agents + 3) / 4)), rb(256);
  hipStream_t st = p->stream;
  // GameCNN                                                                    Modules.hpp:66-71
  if (p->folded || li) {
    // on the non-zeros, timed as kind 2: the four convolutions as one matrix (k_feat_*), or conv0 on the lists
    hipEvent_t e0 = nullptr;
    SFP_RC(p->time_begin(0.0, 2, &e0));  // useful flop depends on the lists: the caller counts the non-zeros
    if (!p->folded) p->conv0_sparse<true>(nullptr, agents, *li);
    else if (li) p->feat_list(agents, *li);
    else p->feat_dense(r.d_obs, p->feat, agents);
    if (e0) SFP_HIP(hipEventRecord(e0, st));
    if (li && r.d_obs) {  // redo the agents whose list did not fit from their dense observation (none, normally: the launch is idle)
      if (p->folded) p->feat_dense(r.d_obs, p->feat, agents, li);
      else p->conv0_sparse<false>(r.d_obs, agents, *li);
    }
  } else if (p->dense_conv0) {
    SFP_RC(p->conv(r.d_obs, p->conv_w[0], p->act[0], agents, 31, OBS_C, 1));
  } else {
    p->conv0_sparse<false>(r.d_obs, agents, C0List{});
  }
  if (!p->folded) SFP_RC(p->conv123(agents, p->fused_tail ? nullptr : p->feat));
  if (p->fused_tail) {
    // (timed as one launch on the f32 pipe: conv3 unless folded + 4 GRU gate products + combined_processor + 6 ResB layers)
    hipEvent_t e1 = nullptr;
    SFP_RC(p->time_begin(2.0 * agents * ((p->folded ? 0.0 : (double)HID * 9 * HID) + 4.0 * G3 * HID + (double)HID * COMB_PAD + (rw ? 3.0 : 6.0) * HID * HID), 3, &e1));
    TailArgs t{};
    t.act2 = p->act[2], t.obs = r.d_obs, t.pov = r.d_pov, t.conv3_w = p->conv_w[3];
    t.feat = p->folded ? p->feat : nullptr;
    for (int g = 0; g < 2; ++g) {
      // (the matrices in k_tail's stream order, stage_tiles)
      t.gru_w_ih[g] = p->tail_w + p->gru_w_ih_t[g], t.gru_w_hh[g] = p->tail_w + p->gru_w_hh_t[g], t.gru_b_ih[g] = p->gru_b_ih[g], t.gru_b_hh[g] = p->gru_b_hh[g];
      t.h[g] = p->h[g];
      if (g && rw) continue;  // (a reward model: one head, slot 0)
      t.head_w[g] = p->tail_w + p->head_w16_t[g], t.head_b[g] = p->head_b16[g];
      for (int i = 0; i < 3; ++i) t.res_w[g][i] = p->tail_w + p->res_w_t[g][i], t.res_b[g][i] = p->res_b[g][i];
    }
    t.comb_w = p->tail_w + p->comb_w_t, t.comb_b = p->comb_b, t.action_input = p->action_input;
    t.agents = agents;
    t.probs = r.probs, t.value = rw ? r.disc : r.value;
    t.action_in = r.action_in, t.reward = r.reward;
    t.reset_mask = r.reset_mask, t.reset_words = r.reset_words, t.reset_stride = r.reset_stride;
    t.reset_group = r.reset_group > 0 ? r.reset_group : 1;
    if (r.act) t.act = 1, t.greedy = r.greedy, t.as = r.as, t.seed = r.seed, t.draw = p->draws++, t.cmd = r.cmd, t.action = r.action;
    const dim3 tl_grid((unsigned)((agents + TL_R - 1) / TL_R));
    if (rw) hipLaunchKernelGGL(k_tail<true>, tl_grid, dim3(TL_T), TL_LDS, st, t);
    else hipLaunchKernelGGL(k_tail<false>, tl_grid, dim3(TL_T), TL_LDS, st, t);
#ifdef SF_DIAG_TAIL  // (diagnostic build: the stamps of a second launch, whose weights the first one left in the L2s)
    if (env_flag("SF_DIAG_TAIL_TWICE", 0) && !rw) hipLaunchKernelGGL(k_tail<false>, tl_grid, dim3(TL_T), TL_LDS, st, t);
#endif
    SFP_HIP(hipGetLastError());
    if (e1) SFP_HIP(hipEventRecord(e1, st));
    return SF_OK;
  }
  float *const none = nullptr;
  hipLaunchKernelGGL(k_norm, rg, rb, 0, st, p->feat, p->feat_n, none, agents);               // :108
  // gru0 (both gate products in one launch)                                                    :110-113
  SFP_RC(p->dense2(p->feat_n, p->gru_w_ih[0], p->gru_b_ih[0], p->gi, p->h[0], p->gru_w_hh[0], p->gru_b_hh[0], p->gh, HID, G3, agents, G3, HID));
  hipLaunchKernelGGL(k_gru0, rg, rb, 0, st, p->gi, p->gh, p->h[0], p->feat_n, r.d_obs, p->action_input, r.action_in, p->comb, agents);
  // combined_processor                                                                         :125-126
  SFP_RC(p->dense(p->comb, COMB_PAD, p->comb_w, p->comb_b, p->gated, HID, agents, HID, COMB_PAD));
  hipLaunchKernelGGL(k_norm, rg, rb, 0, st, p->gated, p->gated_n, none, agents);
  // gru1                                                                                       :128-131
  SFP_RC(p->dense2(p->gated_n, p->gru_w_ih[1], p->gru_b_ih[1], p->gi, p->h[1], p->gru_w_hh[1], p->gru_b_hh[1], p->gh, HID, G3, agents, G3, HID));
  hipLaunchKernelGGL(k_gru1, rg, rb, 0, st, p->gi, p->gh, p->h[1], p->gated_n, p->out, agents);
  if (rw) {  // a reward model's one head: ResB, Linear, sigmoid, log                          RewardNet.hpp:161-165, :257
    hipLaunchKernelGGL(k_norm, rg, rb, 0, st, p->out, p->x[0], none, agents);
    for (int i = 0; i < 3; ++i) {
      SFP_RC(p->dense(p->x[0], HID, p->res_w[0][i], p->res_b[0][i], p->lin[0], HID, agents, HID, HID));
      hipLaunchKernelGGL(k_res, dim3(rg.x, 1), rb, 0, st, p->lin[0], p->x[0], (const float *)nullptr, none, agents);
    }
    hipLaunchKernelGGL(k_reward_head, rg, rb, 0, st, p->x[0], p->head_w[0], p->head_b[0], r.disc, r.reward, agents);
    SFP_HIP(hipGetLastError());
    return SF_OK;
  }
  // heads: ResB then Linear; layer i of both heads shares a launch                             :41-48,172-175
  hipLaunchKernelGGL(k_norm, rg, rb, 0, st, p->out, p->x[0], p->x[1], agents);
  for (int i = 0; i < 3; ++i) {
    SFP_RC(p->dense2(p->x[0], p->res_w[0][i], p->res_b[0][i], p->lin[0], p->x[1], p->res_w[1][i], p->res_b[1][i], p->lin[1], HID, HID, agents, HID, HID));
    hipLaunchKernelGGL(k_res, dim3(rg.x, 2), rb, 0, st, p->lin[0], p->x[0], p->lin[1], p->x[1], agents);
  }
  hipLaunchKernelGGL(k_heads, rg, rb, 0, st, p->x[0], p->x[1], p->head_w[0], p->head_b[0], p->head_w[1], p->head_b[1], r.probs, r.value, agents);
  SFP_HIP(hipGetLastError());
  return SF_OK;
}

}  // namespace sfp

#include "sf_policy_load.hpp"
#include "sf_policy_memory.hpp"

using sfp::Policy;

extern "C" {

int sf_policy_abi_version(void) { return SF_POLICY_ABI_VERSION; }

int sf_policy_create(const sf_policy_weights *w, int32_t max_agents, int32_t device, sf_policy **out) {
  return sfp::create(w, max_agents, device, out);
}

void sf_policy_destroy(sf_policy *p) { delete reinterpret_cast<Policy *>(p); }

int sf_policy_reset_memory_n(sf_policy *pp, const uint8_t *d_mask, int32_t agents) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  SFP_RC(sfp::check_agents(p, agents));
  SFP_HIP(hipSetDevice(p->device));
  const int n = agents * sfp::HID;
  hipLaunchKernelGGL(sfp::k_reset_memory, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, p->stream, p->h[0], p->h[1],
                     p->action_input, d_mask, agents);
  SFP_HIP(hipGetLastError());
  return SF_OK;
}
int sf_policy_reset_memory(sf_policy *pp, const uint8_t *d_mask) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  if (!p) return sfp::fail(SF_ERR_ARG, "null policy");
  return sf_policy_reset_memory_n(pp, d_mask, p->max_agents);
}

int sf_policy_forward(sf_policy *pp, const float *d_obs, int32_t agents, float *d_probs, float *d_value) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  SFP_RC(sfp::check_kind(p, false, "sf_policy_forward"));
  sfp::ForwardReq r{};
  r.d_obs = d_obs, r.probs = d_probs, r.value = d_value;
  return sfp::forward(p, agents, r);
}

int sf_reward_create(const sf_policy_weights *w, int32_t max_agents, int32_t device, sf_policy **out) {
  return sfp::create(w, max_agents, device, out, true);
}

int sf_reward_forward(sf_policy *pp, const float *d_obs, const int32_t *d_action, int32_t agents, float *d_disc, float *d_reward) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  SFP_RC(sfp::check_kind(p, true, "sf_reward_forward"));
  sfp::ForwardReq r{};
  r.reward_model = true, r.d_obs = d_obs, r.action_in = d_action, r.disc = d_disc, r.reward = d_reward;
  return sfp::forward(p, agents, r);
}

int sf_reward_sparse(sf_policy *pp, const sf_reward_io *io, int32_t agents) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  if (!p || !io) return sfp::fail(SF_ERR_ARG, "null policy or io");
  SFP_RC(sfp::check_kind(p, true, "sf_reward_sparse"));
  SFP_RC(sfp::check_lists(io->d_keys, io->d_vals, io->d_counts, io->d_pov, io->cap));
  SFP_RC(sfp::check_resets(io->d_reset_words, io->reset_stride, io->reset_group));
  // (without d_dense: lists that do not fit are counted, as in sf_policy_forward_sparse)
  const sfp::C0List li{io->d_keys, io->d_vals, io->d_counts, io->cap, io->d_dense ? nullptr : p->d_overflows};
  sfp::ForwardReq r{};
  r.reward_model = true, r.d_obs = io->d_dense, r.li = &li, r.d_pov = io->d_pov;
  r.reset_mask = io->d_reset_mask, r.reset_words = io->d_reset_words, r.reset_stride = io->reset_stride, r.reset_group = io->reset_group;
  r.action_in = io->d_action, r.disc = io->d_disc, r.reward = io->d_reward;
  return sfp::forward(p, agents, r);
}

int sf_policy_features(sf_policy *pp, const float *d_obs, int32_t agents, float *d_feat) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  SFP_RC(sfp::check_kind(p, false, "sf_policy_features"));
  SFP_RC(sfp::check_agents(p, agents));
  if (!d_obs || !d_feat) return sfp::fail(SF_ERR_ARG, "null buffer");
  SFP_HIP(hipSetDevice(p->device));
  if (p->folded) {
    p->feat_dense(d_obs, d_feat, agents);
  } else {
    p->conv0_sparse<false>(d_obs, agents, sfp::C0List{});
    SFP_RC(p->conv123(agents, d_feat));
  }
  SFP_HIP(hipGetLastError());
  return SF_OK;
}

int sf_policy_forward_sparse(sf_policy *pp, const uint32_t *d_keys, const float *d_vals, const uint32_t *d_counts,
                             const float *d_pov, int32_t cap, int32_t agents, float *d_probs, float *d_value) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  SFP_RC(sfp::check_kind(p, false, "sf_policy_forward_sparse"));
  SFP_RC(sfp::check_lists(d_keys, d_vals, d_counts, d_pov, cap));
  const sfp::C0List li{d_keys, d_vals, d_counts, cap, p->d_overflows};
  sfp::ForwardReq r{};
  r.li = &li, r.d_pov = d_pov, r.probs = d_probs, r.value = d_value;
  return sfp::forward(p, agents, r);
}

int sf_policy_forward_sparse_or_dense(sf_policy *pp, const uint32_t *d_keys, const float *d_vals, const uint32_t *d_counts,
                                      const float *d_pov, int32_t cap, int32_t agents, const float *d_dense, float *d_probs,
                                      float *d_value) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  SFP_RC(sfp::check_kind(p, false, "sf_policy_forward_sparse_or_dense"));
  SFP_RC(sfp::check_lists(d_keys, d_vals, d_counts, d_pov, cap, d_dense != nullptr));
  const sfp::C0List li{d_keys, d_vals, d_counts, cap, nullptr};
  sfp::ForwardReq r{};
  r.d_obs = d_dense, r.li = &li, r.d_pov = d_pov, r.probs = d_probs, r.value = d_value;
  return sfp::forward(p, agents, r);
}

int sf_policy_predict_sparse(sf_policy *pp, const sf_policy_predict_io *io, int32_t agents) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  if (!p || !io) return sfp::fail(SF_ERR_ARG, "null policy or io");
  SFP_RC(sfp::check_kind(p, false, "sf_policy_predict_sparse"));
  SFP_RC(sfp::check_lists(io->d_keys, io->d_vals, io->d_counts, io->d_pov, io->cap));
  if (!io->d_cmd || !io->action_string) return sfp::fail(SF_ERR_ARG, "null buffer");
  if (std::strlen(io->action_string) != (size_t)sfp::ACT) return sfp::fail(SF_ERR_ARG, "action_string must have 9 chars");
  SFP_RC(sfp::check_resets(io->d_reset_words, io->reset_stride, io->reset_group));
  // (without d_dense: lists that do not fit are counted, as in sf_policy_forward_sparse)
  const sfp::C0List li{io->d_keys, io->d_vals, io->d_counts, io->cap, io->d_dense ? nullptr : p->d_overflows};
  sfp::ForwardReq r{};
  r.d_obs = io->d_dense, r.li = &li, r.d_pov = io->d_pov, r.probs = io->d_probs, r.value = io->d_value;
  r.reset_mask = io->d_reset_mask, r.reset_words = io->d_reset_words, r.reset_stride = io->reset_stride, r.reset_group = io->reset_group;
  r.act = true, r.seed = io->seed, r.greedy = io->greedy, r.cmd = io->d_cmd, r.action = io->d_action;
  std::memcpy(r.as.c, io->action_string, sfp::ACT);
  return sfp::forward(p, agents, r);
}

#ifdef SF_DIAG_TAIL
int sf_policy_diag_tail_read(uint32_t *out, int32_t workgroups) {  // diagnostic build only: [workgroups][16 waves][24 phases] cycles
  if (hipDeviceSynchronize() != hipSuccess) return SF_ERR_DEVICE;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(sfp::sf_diag_tail), (size_t)workgroups * 16 * 24 * sizeof(uint32_t)) == hipSuccess ? SF_OK : SF_ERR_DEVICE;
}
#endif
int sf_policy_sparse_overflows(sf_policy *pp, int32_t *count) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  if (!p || !count) return sfp::fail(SF_ERR_ARG, "null argument");
  SFP_HIP(hipSetDevice(p->device));
  SFP_HIP(hipStreamSynchronize(p->stream));
  uint32_t n = 0;
  SFP_HIP(hipMemcpy(&n, p->d_overflows, sizeof(n), hipMemcpyDeviceToHost));
  SFP_HIP(hipMemset(p->d_overflows, 0, sizeof(n)));
  *count = (int32_t)n;
  return SF_OK;
}

int sf_policy_act(sf_policy *pp, const float *d_probs, int32_t agents, const char *action_string, uint64_t seed,
                  int32_t greedy, uint8_t *d_cmd, int32_t *d_action) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  SFP_RC(sfp::check_kind(p, false, "sf_policy_act"));
  SFP_RC(sfp::check_agents(p, agents));
  if (!d_probs || !d_cmd || !action_string) return sfp::fail(SF_ERR_ARG, "null buffer");
  if (std::strlen(action_string) != (size_t)sfp::ACT) return sfp::fail(SF_ERR_ARG, "action_string must have 9 chars");
  sfp::ActStr as;
  std::memcpy(as.c, action_string, sfp::ACT);
  SFP_HIP(hipSetDevice(p->device));
  hipLaunchKernelGGL(sfp::k_act, dim3((unsigned)((agents + 255) / 256)), dim3(256), 0, p->stream, d_probs,
                     p->action_input, as, seed, p->draws++, greedy, d_cmd, d_action, agents);
  SFP_HIP(hipGetLastError());
  return SF_OK;
}

int sf_policy_act_masked(sf_policy *pp, const float *d_probs, int32_t agents, const char *action_string, uint64_t seed,
                         int32_t greedy, const uint32_t *d_action_mask, uint8_t *d_cmd, int32_t *d_action, float *d_probs_out) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  SFP_RC(sfp::check_kind(p, false, "sf_policy_act_masked"));
  SFP_RC(sfp::check_agents(p, agents));
  if (!d_probs || !d_cmd || !action_string || !d_action_mask) return sfp::fail(SF_ERR_ARG, "null buffer");
  if (std::strlen(action_string) != (size_t)sfp::ACT) return sfp::fail(SF_ERR_ARG, "action_string must have 9 chars");
  sfp::ActStr as;
  std::memcpy(as.c, action_string, sfp::ACT);
  SFP_HIP(hipSetDevice(p->device));
  hipLaunchKernelGGL(sfp::k_act_masked, dim3((unsigned)((agents + 255) / 256)), dim3(256), 0, p->stream, d_probs, d_action_mask,
                     p->action_input, as, seed, p->draws++, greedy, d_cmd, d_action, d_probs_out, agents);
  SFP_HIP(hipGetLastError());
  return SF_OK;
}

int sf_policy_gemm(sf_policy *pp, const float *d_a, int32_t lda, const float *d_w, const float *d_bias, float *d_c,
                   int32_t ldc, int32_t m, int32_t n, int32_t k) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  if (!p || !d_a || !d_w || !d_c) return sfp::fail(SF_ERR_ARG, "null argument");
  if (lda % 4 || ldc % 4 || lda < k || ldc < n) return sfp::fail(SF_ERR_ARG, "policy gemm: bad leading dimension");
  SFP_HIP(hipSetDevice(p->device));
  return p->dense(d_a, lda, d_w, d_bias, d_c, ldc, m, n, k);
}

int sf_policy_gemm_split(sf_policy *pp, const float *d_a, int32_t lda, const float *d_w, const float *d_bias, float *d_c,
                         int32_t ldc, int32_t m, int32_t n, int32_t k) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  if (!p || !d_a || !d_w || !d_c) return sfp::fail(SF_ERR_ARG, "null argument");
  if (lda % 4 || ldc % 4 || lda < k || ldc < n) return sfp::fail(SF_ERR_ARG, "policy gemm: bad leading dimension");
  if (k % 32 || n % sfp::BN || m < 1) return sfp::fail(SF_ERR_ARG, "policy gemm: unsupported shape");
  SFP_HIP(hipSetDevice(p->device));
  void *img = nullptr;
  if (hipMalloc(&img, (size_t)n * k * 3 * sizeof(uint16_t)) != hipSuccess) return sfp::fail(SF_ERR_MEMORY, "hipMalloc failed (split W)");
  const size_t elems = (size_t)n * k;
  hipLaunchKernelGGL(sfp::k_split_weights, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, p->stream, d_w,
                     (uint16_t *)img, n, k);
  int rc = p->dense(d_a, lda, d_w, d_bias, d_c, ldc, m, n, k, img);
  if (hipStreamSynchronize(p->stream) != hipSuccess && !rc) rc = sfp::fail(SF_ERR_DEVICE, "policy gemm (split) failed");
  (void)hipFree(img);
  return rc;
}

int sf_policy_get_memory(sf_policy *pp, int32_t agent, float *h, float *action_input) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  if (!p || agent < 0 || agent >= p->max_agents || !h || !action_input) return sfp::fail(SF_ERR_ARG, "bad argument");
  SFP_HIP(hipSetDevice(p->device));
  SFP_HIP(hipStreamSynchronize(p->stream));
  for (int g = 0; g < 2; ++g)
    SFP_HIP(hipMemcpy(h + g * sfp::HID, p->h[g] + (size_t)agent * sfp::HID, sfp::HID * sizeof(float), hipMemcpyDeviceToHost));
  SFP_HIP(hipMemcpy(action_input, p->action_input + (size_t)agent * sfp::ACT, sfp::ACT * sizeof(float), hipMemcpyDeviceToHost));
  return SF_OK;
}

int sf_policy_set_memory(sf_policy *pp, int32_t agent, const float *h, const float *action_input) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  if (!p || agent < 0 || agent >= p->max_agents || !h || !action_input) return sfp::fail(SF_ERR_ARG, "bad argument");
  SFP_HIP(hipSetDevice(p->device));
  SFP_HIP(hipStreamSynchronize(p->stream));
  for (int g = 0; g < 2; ++g)
    SFP_HIP(hipMemcpy(p->h[g] + (size_t)agent * sfp::HID, h + g * sfp::HID, sfp::HID * sizeof(float), hipMemcpyHostToDevice));
  SFP_HIP(hipMemcpy(p->action_input + (size_t)agent * sfp::ACT, action_input, sfp::ACT * sizeof(float), hipMemcpyHostToDevice));
  return SF_OK;
}

int sf_policy_memory_rows(sf_policy *pp, int32_t to_rows, float *d_h, float *d_action, const int32_t *d_row_of_agent, int32_t rows,
                          int32_t agents) {
  return sfp::memory_rows(reinterpret_cast<Policy *>(pp), to_rows, d_h, d_action, d_row_of_agent, rows, agents);
}

int sf_policy_set_stream(sf_policy *pp, void *hip_stream) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  if (!p) return sfp::fail(SF_ERR_ARG, "null policy");
  p->stream = reinterpret_cast<hipStream_t>(hip_stream);
  return SF_OK;
}

int sf_policy_synchronize(sf_policy *pp) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  if (!p) return sfp::fail(SF_ERR_ARG, "null policy");
  SFP_HIP(hipSetDevice(p->device));
  SFP_HIP(hipStreamSynchronize(p->stream));
  return SF_OK;
}

int sf_policy_kernel_time_by_kernel(sf_policy *pp, int32_t enable, float ms[4], double flop[4], int32_t launches[4]) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  if (!p || !ms || !flop || !launches) return sfp::fail(SF_ERR_ARG, "null argument");
  return p->take_times(enable, ms, flop, launches);
}

// [0] the f32 matrix pipe (k_gemm and k_tail), [1] k_gemm_b3; the convolutions on the non-zeros are no matrix launches
int sf_policy_kernel_time_ex(sf_policy *pp, int32_t enable, float ms[2], double flop[2], int32_t launches[2]) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  if (!p) return sfp::fail(SF_ERR_ARG, "null policy");
  float t[4];
  double fl[4];
  int32_t n[4];
  SFP_RC(p->take_times(enable, t, fl, n));
  if (ms) ms[0] = t[0] + t[3], ms[1] = t[1];
  if (flop) flop[0] = fl[0] + fl[3], flop[1] = fl[1];
  if (launches) launches[0] = n[0] + n[3], launches[1] = n[1];
  return SF_OK;
}

int sf_policy_kernel_time(sf_policy *pp, int32_t enable, float *ms, double *flop, int32_t *launches) {
  float m[2];
  double f[2];
  int32_t n[2];
  SFP_RC(sf_policy_kernel_time_ex(pp, enable, m, f, n));
  if (ms) *ms = m[0] + m[1];
  if (flop) *flop = f[0] + f[1];
  if (launches) *launches = n[0] + n[1];
  return SF_OK;
}

}  // extern "C"

// ---- the rollout buffer (sf_rollout_*): the caller's storage, the library's cursors and counters -------------------------
namespace sfp {
struct Rollout {
  int device = 0, agents = 0;
  hipStream_t stream = nullptr;
  RolloutDst d{};
  uint8_t *first = nullptr;  // the caller's [T][agents], set: the continuing rule (sf_rollout_continue)
  float *v = nullptr;        // [T][agents], sf_rollout_gae's V when the caller takes none; made by the first call that needs it
  ~Rollout() {
    if (v) (void)hipFree(v);
    if (d.fill) (void)hipFree(d.fill);
    if (d.counters) (void)hipFree(d.counters);
  }
};
static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static dim3 per_lane(int n) { return dim3((unsigned)((n + 255) / 256)); }
}  // namespace sfp
using sfp::Rollout;

extern "C" {

int sf_rollout_create(const sf_rollout_buffers *b, int32_t agents, int32_t T, int32_t list_cap, int32_t device, sf_rollout **out) {
  if (!b || !out) return sfp::fail(SF_ERR_ARG, "null argument");
  if (agents < 1 || agents > (1 << 20)) return sfp::fail(SF_ERR_ARG, "agents must be 1..1048576");
  if (T < 2 || T % 2) return sfp::fail(SF_ERR_ARG, "T must be even and at least 2");
  if (b->keys && (list_cap % 4 || list_cap < 4 || list_cap > SF_POLICY_LIST_MAX))
    return sfp::fail(SF_ERR_ARG, "list_cap must be a multiple of 4 in [4, SF_POLICY_LIST_MAX]");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return sfp::fail(SF_ERR_DEVICE, "no HIP device: the rollout buffer has no CPU path");
  if (device < 0 || device >= n) return sfp::fail(SF_ERR_DEVICE, "device ordinal out of range");
  if (!b->action || !b->logp || !b->value || !b->reward || (b->keys && (!b->vals || !b->counts || !b->pov)))
    return sfp::fail(SF_ERR_ARG, "sf_rollout_buffers has a null pointer");
  if (b->keys && (!sfp::aligned16(b->keys) || !sfp::aligned16(b->vals) || !sfp::aligned16(b->pov)))
    return sfp::fail(SF_ERR_ARG, "keys, vals and pov must be 16-byte aligned");
  SFP_HIP(hipSetDevice(device));
  std::unique_ptr<Rollout> r(new Rollout());
  r->device = device, r->agents = agents;
  sfp::RolloutDst &d = r->d;
  d.keys = b->keys, d.vals = b->vals, d.counts = b->counts, d.pov = b->pov, d.action = b->action, d.logp = b->logp;
  d.value = b->value, d.reward = b->reward, d.disc = b->disc, d.imitate = b->imitate;
  d.stride = agents, d.T = T, d.list_cap = b->keys ? list_cap : 0;
  if (hipMalloc(reinterpret_cast<void **>(&d.fill), (size_t)agents * sizeof(int32_t)) != hipSuccess ||
      hipMalloc(reinterpret_cast<void **>(&d.counters), 3 * sizeof(unsigned long long)) != hipSuccess)
    return sfp::fail(SF_ERR_MEMORY, "hipMalloc failed (rollout)");
  SFP_HIP(hipMemset(d.fill, 0, (size_t)agents * sizeof(int32_t)));
  SFP_HIP(hipMemset(d.counters, 0, 3 * sizeof(unsigned long long)));
  *out = reinterpret_cast<sf_rollout *>(r.release());
  return SF_OK;
}

void sf_rollout_destroy(sf_rollout *r) { delete reinterpret_cast<Rollout *>(r); }

int sf_rollout_set_stream(sf_rollout *rr, void *hip_stream) {
  Rollout *r = reinterpret_cast<Rollout *>(rr);
  if (!r) return sfp::fail(SF_ERR_ARG, "null rollout");
  r->stream = reinterpret_cast<hipStream_t>(hip_stream);
  return SF_OK;
}

int sf_rollout_synchronize(sf_rollout *rr) {
  Rollout *r = reinterpret_cast<Rollout *>(rr);
  if (!r) return sfp::fail(SF_ERR_ARG, "null rollout");
  SFP_HIP(hipSetDevice(r->device));
  SFP_HIP(hipStreamSynchronize(r->stream));
  return SF_OK;
}

int sf_rollout_record(sf_rollout *rr, const sf_rollout_step *io) {
  Rollout *r = reinterpret_cast<Rollout *>(rr);
  if (!r || !io) return sfp::fail(SF_ERR_ARG, "null rollout or io");
  if (io->agents < 1 || io->agents > r->agents) return sfp::fail(SF_ERR_ARG, "agents out of range for this rollout");
  const bool keep = r->d.keys != nullptr;
  if (keep) SFP_RC(sfp::check_lists(io->d_keys, io->d_vals, io->d_counts, io->d_pov, io->cap));
  if (!io->d_probs || !io->d_value || !io->d_action || !io->d_reward || (r->d.disc && !io->d_disc) || (r->d.imitate && !io->d_imitate))
    return sfp::fail(SF_ERR_ARG, "null buffer");
  SFP_RC(sfp::check_resets(io->d_reset_words, io->reset_stride, io->reset_group));
  sfp::RolloutSrc s{};
  if (keep) {
    s.keys = io->d_keys, s.vals = io->d_vals, s.counts = io->d_counts, s.pov = io->d_pov, s.cap = io->cap;
    s.vec = io->cap % 4 == 0 && sfp::aligned16(io->d_keys) && sfp::aligned16(io->d_vals);
    s.pov_vec = sfp::aligned16(io->d_pov);
  }
  s.probs = io->d_probs, s.value = io->d_value, s.action = io->d_action, s.reward = io->d_reward, s.disc = io->d_disc, s.imitate = io->d_imitate;
  s.reset_mask = io->d_reset_mask, s.reset_words = io->d_reset_words, s.reset_stride = io->reset_stride;
  s.reset_group = io->reset_group > 0 ? io->reset_group : 1;
  s.agents = io->agents;
  SFP_HIP(hipSetDevice(r->device));
  const dim3 grid((unsigned)((io->agents + 3) / 4));
  if (r->first)
    hipLaunchKernelGGL(sfp::k_rollout_record_cont, grid, dim3(256), 0, r->stream, r->d, s, r->first);
  else
    hipLaunchKernelGGL(sfp::k_rollout_record, grid, dim3(256), 0, r->stream, r->d, s);
  SFP_HIP(hipGetLastError());
  return SF_OK;
}

int sf_rollout_continue(sf_rollout *rr, uint8_t *d_first) {
  Rollout *r = reinterpret_cast<Rollout *>(rr);
  if (!r) return sfp::fail(SF_ERR_ARG, "null rollout");
  SFP_HIP(hipSetDevice(r->device));
  SFP_HIP(hipMemsetAsync(r->d.fill, 0, (size_t)r->agents * sizeof(int32_t), r->stream));
  r->first = d_first;
  return SF_OK;
}

int sf_rollout_gae(sf_rollout *rr, const sf_rollout_gae_io *io) {
  Rollout *r = reinterpret_cast<Rollout *>(rr);
  if (!r || !io) return sfp::fail(SF_ERR_ARG, "null rollout or io");
  if (!(io->gamma >= 0.f && io->gamma <= 1.f) || !(io->lambda >= 0.f && io->lambda <= 1.f))
    return sfp::fail(SF_ERR_ARG, "gamma and lambda must lie in [0, 1]");
  if (io->d_next_mask && io->d_next_words) return sfp::fail(SF_ERR_ARG, "the next tick's restart flags: d_next_mask or d_next_words, not both");
  SFP_RC(sfp::check_resets(io->d_next_words, io->next_stride, io->next_group));
  if (!io->d_returns && !io->d_v && !io->d_adv) return sfp::fail(SF_ERR_ARG, "null buffer");
  SFP_HIP(hipSetDevice(r->device));
  const sfp::RolloutDst &d = r->d;
  // V: the stored values themselves when nobody asks for a copy or a logarithm of them
  const float *v = d.value;
  if (io->log_values || io->d_v) {
    float *out = io->d_v;
    if (!out) {
      if (!r->v && hipMalloc(reinterpret_cast<void **>(&r->v), (size_t)d.T * (size_t)r->agents * sizeof(float)) != hipSuccess)
        return sfp::fail(SF_ERR_MEMORY, "hipMalloc failed (sf_rollout_gae's V)");
      out = r->v;
    }
    const dim3 grid((unsigned)((r->agents + 255) / 256), (unsigned)((d.T + sfp::GV_ROWS - 1) / sfp::GV_ROWS));
    hipLaunchKernelGGL(sfp::k_rollout_gae_v, grid, dim3(256), 0, r->stream, d.fill, d.value, out, d.T, d.stride, io->log_values ? 1 : 0, r->agents);
    SFP_HIP(hipGetLastError());
    v = out;
  }
  if (io->d_returns || io->d_adv) {
    sfp::GaeArgs g{};
    g.gamma = io->gamma, g.lambda = io->lambda, g.scale = io->reward_scale, g.log_values = io->log_values ? 1 : 0;
    g.next_value = io->d_next_value, g.next_mask = io->d_next_mask, g.next_words = io->d_next_words;
    g.next_stride = io->next_stride, g.next_group = io->next_group > 0 ? io->next_group : 1;
    g.first = r->first, g.v = v, g.returns = io->d_returns, g.adv = io->d_adv, g.agents = r->agents;
    hipLaunchKernelGGL(sfp::k_rollout_gae, dim3((unsigned)((r->agents + 63) / 64)), dim3(64), 0, r->stream, d, g);
    SFP_HIP(hipGetLastError());
  }
  return SF_OK;
}

int sf_rollout_dense(sf_rollout *rr, const sf_rollout_dense_io *io) {
  Rollout *r = reinterpret_cast<Rollout *>(rr);
  if (!io) return sfp::fail(SF_ERR_ARG, "null io");
  // what the struct alone decides, then the object
  if (io->rows < 1 || io->rows > SF_ROLLOUT_DENSE_ROWS_MAX) return sfp::fail(SF_ERR_ARG, "sf_rollout_dense: rows must be 1..SF_ROLLOUT_DENSE_ROWS_MAX");
  if (io->dtype != SF_DENSE_F32 && io->dtype != SF_DENSE_BF16 && io->dtype != SF_DENSE_F16)
    return sfp::fail(SF_ERR_ARG, "sf_rollout_dense: unknown dtype");
  if (io->layout != SF_DENSE_NCHW && io->layout != SF_DENSE_NHWC) return sfp::fail(SF_ERR_ARG, "sf_rollout_dense: unknown layout");
  if (!io->d_dense || !sfp::aligned16(io->d_dense)) return sfp::fail(SF_ERR_ARG, "sf_rollout_dense: d_dense must be set and 16-byte aligned");
  if (!r) return sfp::fail(SF_ERR_ARG, "null rollout");
  const sfp::RolloutDst &d = r->d;
  if (!d.keys) return sfp::fail(SF_ERR_STATE, "sf_rollout_dense: this rollout keeps no states (keys == NULL at sf_rollout_create)");
  if (!io->d_cells && (io->slot < 0 || io->slot >= d.T || io->agent0 < 0 || io->rows > r->agents - io->agent0))
    return sfp::fail(SF_ERR_ARG, "sf_rollout_dense: slot or agents out of range for this rollout");
  sfp::DenseArgs g{};
  g.keys = d.keys, g.vals = reinterpret_cast<const uint32_t *>(d.vals), g.counts = d.counts, g.cells = io->d_cells;
  const uint64_t n_cells = (uint64_t)d.T * (uint64_t)d.stride;  // (a cell is an int32: none reaches 2^31)
  g.n_cells = (uint32_t)(n_cells < 0x80000000ull ? n_cells : 0x80000000ull);
  // (slot * agents + agent0 is below n_cells; where that is capped no int32 holds it and d_cells is the way in)
  if (!io->d_cells) {
    const uint64_t c0 = (uint64_t)io->slot * (uint64_t)d.stride + (uint64_t)io->agent0;
    if (c0 + (uint64_t)io->rows > 0x80000000ull) return sfp::fail(SF_ERR_ARG, "sf_rollout_dense: the slot's cells do not fit an int32");
    g.cell0 = (int32_t)c0;
  }
  g.list_cap = d.list_cap, g.dense = io->d_dense, g.valid = io->d_valid;
  SFP_HIP(hipSetDevice(r->device));
  const dim3 grid((unsigned)io->rows), block(sfp::DENSE_WG);
  g.nhwc = io->layout == SF_DENSE_NHWC ? 1 : 0;
  if (io->dtype == SF_DENSE_F32)
    hipLaunchKernelGGL(sfp::k_rollout_dense<0>, grid, block, 0, r->stream, g);
  else if (io->dtype == SF_DENSE_BF16)
    hipLaunchKernelGGL(sfp::k_rollout_dense<1>, grid, block, 0, r->stream, g);
  else
    hipLaunchKernelGGL(sfp::k_rollout_dense<2>, grid, block, 0, r->stream, g);
  SFP_HIP(hipGetLastError());
  return SF_OK;
}

int sf_rollout_fill_device(sf_rollout *rr, const int32_t **d_fill) {
  Rollout *r = reinterpret_cast<Rollout *>(rr);
  if (!r || !d_fill) return sfp::fail(SF_ERR_ARG, "null argument");
  *d_fill = r->d.fill;
  return SF_OK;
}

int sf_rollout_ready_device(sf_rollout *rr, uint8_t *d_mask) {
  Rollout *r = reinterpret_cast<Rollout *>(rr);
  if (!r || !d_mask) return sfp::fail(SF_ERR_ARG, "null argument");
  SFP_HIP(hipSetDevice(r->device));
  hipLaunchKernelGGL(sfp::k_rollout_ready, sfp::per_lane(r->agents), dim3(256), 0, r->stream, r->d.fill, r->d.T, d_mask,
                     (unsigned long long *)nullptr, r->agents);
  SFP_HIP(hipGetLastError());
  return SF_OK;
}

int sf_rollout_status(sf_rollout *rr, int32_t *ready, int64_t *dropped, int64_t *missing_states) {
  Rollout *r = reinterpret_cast<Rollout *>(rr);
  if (!r) return sfp::fail(SF_ERR_ARG, "null rollout");
  SFP_HIP(hipSetDevice(r->device));
  SFP_HIP(hipMemsetAsync(r->d.counters + 2, 0, sizeof(unsigned long long), r->stream));
  hipLaunchKernelGGL(sfp::k_rollout_ready, sfp::per_lane(r->agents), dim3(256), 0, r->stream, r->d.fill, r->d.T, (uint8_t *)nullptr,
                     r->d.counters + 2, r->agents);
  SFP_HIP(hipGetLastError());
  unsigned long long c[3] = {0, 0, 0};
  SFP_HIP(hipMemcpyAsync(c, r->d.counters, sizeof(c), hipMemcpyDeviceToHost, r->stream));
  SFP_HIP(hipStreamSynchronize(r->stream));
  if (dropped) *dropped = (int64_t)c[0];
  if (missing_states) *missing_states = (int64_t)c[1];
  if (ready) *ready = (int32_t)c[2];
  return SF_OK;
}

int sf_rollout_returns(sf_rollout *rr, float gamma, float *d_returns, float *d_logv, float *d_adv, float *d_stats) {
  Rollout *r = reinterpret_cast<Rollout *>(rr);
  if (!r) return sfp::fail(SF_ERR_ARG, "null rollout");
  if (!d_returns && !d_logv && !d_adv && !d_stats) return sfp::fail(SF_ERR_ARG, "null buffer");
  if (!sfp::aligned16(d_stats)) return sfp::fail(SF_ERR_ARG, "d_stats must be 16-byte aligned");
  SFP_HIP(hipSetDevice(r->device));
  hipLaunchKernelGGL(sfp::k_rollout_returns, sfp::per_lane(r->agents), dim3(256), 0, r->stream, r->d, gamma, d_returns, d_logv, d_adv,
                     d_stats, r->agents);
  SFP_HIP(hipGetLastError());
  return SF_OK;
}

int sf_rollout_release(sf_rollout *rr, const uint8_t *d_mask) {
  Rollout *r = reinterpret_cast<Rollout *>(rr);
  if (!r) return sfp::fail(SF_ERR_ARG, "null rollout");
  SFP_HIP(hipSetDevice(r->device));
  hipLaunchKernelGGL(sfp::k_rollout_release, sfp::per_lane(r->agents), dim3(256), 0, r->stream, r->d.fill, r->d.T, d_mask, r->agents);
  SFP_HIP(hipGetLastError());
  return SF_OK;
}

int sf_rollout_state(sf_rollout *rr, int32_t t, const uint32_t **d_keys, const float **d_vals, const uint32_t **d_counts,
                     const float **d_pov, int32_t *cap) {
  Rollout *r = reinterpret_cast<Rollout *>(rr);
  if (!r || !d_keys || !d_vals || !d_counts || !d_pov || !cap) return sfp::fail(SF_ERR_ARG, "null argument");
  if (!r->d.keys) return sfp::fail(SF_ERR_STATE, "sf_rollout_state: this rollout keeps no states (keys == NULL at sf_rollout_create)");
  if (t < 0 || t >= r->d.T) return sfp::fail(SF_ERR_ARG, "slot out of range for this rollout");
  const size_t row = (size_t)t * (size_t)r->d.stride;
  *d_keys = r->d.keys + row * r->d.list_cap, *d_vals = r->d.vals + row * r->d.list_cap;
  *d_counts = r->d.counts + row, *d_pov = r->d.pov + row * sfp::HID, *cap = r->d.list_cap;
  return SF_OK;
}

int sf_policy_update_actions(sf_policy *pp, const int32_t *d_action, int32_t agents) {
  Policy *p = reinterpret_cast<Policy *>(pp);
  SFP_RC(sfp::check_agents(p, agents));
  if (!d_action) return sfp::fail(SF_ERR_ARG, "null buffer");
  SFP_HIP(hipSetDevice(p->device));
  hipLaunchKernelGGL(sfp::k_update_actions, sfp::per_lane(agents * sfp::ACT), dim3(256), 0, p->stream, p->action_input, d_action, agents);
  SFP_HIP(hipGetLastError());
  return SF_OK;
}

int sf_policy_load_weights(sf_policy *pp, const sf_policy_weights *d_w) {
  return sfp::load_weights(reinterpret_cast<Policy *>(pp), d_w);
}

int sf_policy_weights_digest(sf_policy *pp, uint64_t *out_host, int32_t *count) {
  return sfp::weights_digest(reinterpret_cast<Policy *>(pp), out_host, count);
}

}  // extern "C"

#include "sf_policy_route.hpp"
