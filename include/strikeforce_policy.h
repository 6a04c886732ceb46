/* strikeforce_policy.h — C-ABI of the batched on-device policy network.
 *
 * The reference evaluates its bot network once per agent per tick on the host with libtorch, batch 1
 * (StrikeForce-client/bots/bot-0.5/Agent.hpp:178-214 predict(), Modules.hpp:54-179 AgentModel).  This
 * library evaluates the same network for every agent of an arena batch in one pass on the GPU, reading
 * the observation buffer sf_observe_device() wrote and producing the command chars sf_step_device()
 * consumes, so the 123 KB/agent observation never leaves HBM.  Inputs, outputs and state are f32.
 *
 * The convolution stack.  GameCNN::forward (Modules.hpp:66-71) applies four bias-free 3x3 / stride-2 convolutions with
 * nothing between them: one linear map of the 32 x 31 x 31 observation onto 160 features.  sf_policy_create composes the
 * four weight tensors into that map's matrix once (f64 on the device, rounded to f32), and a forward pass adds up one
 * row of it per non-zero float of the observation (about 1 % of the floats are non-zero): f32 fmaf chains per pair of
 * channels, combined in f64.  Same function as the layer-by-layer evaluation, 0.1 instead of 48.6 MFLOP per agent; the
 * difference from the reference's f32 layer-by-layer result is of the size of that result's own rounding (tests: |err| <=
 * 1e-6 + 5e-5 |ref| on probabilities, value and recurrent state against the reference's own AgentModel).
 * SF_POLICY_LAYERED=1 in the environment at sf_policy_create evaluates the four layers one after the other instead
 * (conv0 on the non-zeros; conv1 and conv2 — at 16 384 rows and more — on the bf16 MFMA with every f32 operand split
 * into three bf16 parts, |err| <= 2e-6 * sum|a*w|; conv3 on the f32 MFMA; SF_POLICY_F32_CONV=1 keeps all of them on the
 * f32 pipe): the cross-check path, held to the same tests.
 * Everything behind the convolutions (two GRU cells, combined_processor, the ResB heads) runs on the f32-input MFMA
 * (bit for bit an fmaf chain).  Every agent keeps its own recurrent state exactly as one
 * reference `Agent` object does.  Inference only: the PPO learner (Agent.hpp:270-420) is out of scope.
 *
 * Same conventions as strikeforce.h: plain pointers and sizes, 0 = success, sf_last_error() for text,
 * no CPU path (SF_ERR_DEVICE without a GPU).
 */
#ifndef STRIKEFORCE_POLICY_H
#define STRIKEFORCE_POLICY_H

#include <stdint.h>

#include "strikeforce.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SF_POLICY_ABI_VERSION 1
#define SF_POLICY_HIDDEN 160   /* hidden_size   Modules.hpp:83,144 */
#define SF_POLICY_ACTIONS 9    /* num_actions   Modules.hpp:83,144; action string "+xzqeawsd" Custom.hpp:162 */
#define SF_POLICY_CONVS 4      /* GameCNN(num_channels, hidden_size, 4, grid_x)  Modules.hpp:86 */
#define SF_POLICY_RES_LAYERS 3 /* LAYER_INDEX   Modules.hpp:28 */
#define SF_POLICY_POV (5 * SF_OBS_CHANNELS + SF_POLICY_ACTIONS) /* 169: the 5 centre cells + last action  Modules.hpp:115-122 */

/* Host pointers to the parameters, in the layouts torch uses for the reference's modules (row-major,
 * f32).  Names follow the reference's register_module() names. */
typedef struct sf_policy_weights {
  int32_t abi_version;
  /* backbone.cnn.conv{i}.weight: conv0 [160][32][3][3], conv1..3 [160][160][3][3]; stride 2, no padding, no
   * bias (Modules.hpp:58-64) */
  const float *conv_w[SF_POLICY_CONVS];
  /* backbone.gru{g}.weight_ih_l0 / weight_hh_l0 [480][160], bias_ih_l0 / bias_hh_l0 [480]; gate order r,z,n
   * (torch::nn::GRU, Modules.hpp:87,91) */
  const float *gru_w_ih[2], *gru_w_hh[2], *gru_b_ih[2], *gru_b_hh[2];
  /* backbone.combined_processor.0.weight [160][2*160+9], .bias [160]  (Modules.hpp:88-90) */
  const float *comb_w, *comb_b;
  /* value.0.lin{i}.weight [160][160], .bias [160]; value.1.weight [1][160], .bias [1]   (Modules.hpp:147-149) */
  const float *value_res_w[SF_POLICY_RES_LAYERS], *value_res_b[SF_POLICY_RES_LAYERS], *value_w, *value_b;
  /* policy.0.lin{i}.weight, .bias; policy.1.weight [9][160], .bias [9]                 (Modules.hpp:150-152) */
  const float *policy_res_w[SF_POLICY_RES_LAYERS], *policy_res_b[SF_POLICY_RES_LAYERS], *policy_w, *policy_b;
} sf_policy_weights;

typedef struct sf_policy sf_policy;

/* new AgentModel + load of its parameters (Agent.hpp:77-110), for `max_agents` independent agents (each has
 * its own h_state[2] and action_input, Modules.hpp:81).  Memory starts as after reset_memory(). */
int sf_policy_create(const sf_policy_weights *w, int32_t max_agents, int32_t device, sf_policy **out);
void sf_policy_destroy(sf_policy *p);

/* Backbone::reset_memory() (Modules.hpp:95-100) for the agents whose byte in d_mask (device) is non-zero; NULL resets
 * every agent.  Call it with the done flags when an arena restarts: the reference builds a new Agent per game
 * (Custom.hpp prepare()).  d_mask must hold `max_agents` bytes (the count given to sf_policy_create): every agent of
 * the policy is looked at.  A caller that runs fewer agents, with a mask of that many bytes (the sf_done_device output
 * of a smaller env), uses sf_policy_reset_memory_n: only agents [0, agents) are looked at. */
int sf_policy_reset_memory(sf_policy *p, const uint8_t *d_mask);
int sf_policy_reset_memory_n(sf_policy *p, const uint8_t *d_mask, int32_t agents);

/* AgentModel::forward (Modules.hpp:106-134,169-178) for agents [0, agents): d_obs is the device buffer of
 * sf_observe_device ([agents][32][31][31] f32); writes d_probs [agents][9] (softmax + 1e-8) and d_value [agents]
 * (sigmoid), and advances every agent's h_state. */
int sf_policy_forward(sf_policy *p, const float *d_obs, int32_t agents, float *d_probs, float *d_value);

/* sf_policy_forward on the observation in list form (sf_observe_sparse_device: d_keys / d_vals [agents][cap],
 * d_counts [agents], d_pov [agents][160]): the convolution stack takes the non-zeros as they come instead of scanning a
 * dense 123 KB buffer per agent for them, and the five centre cells come from d_pov.  Same results as the dense call,
 * bit for bit (same values applied in the same order).  cap is at most SF_POLICY_LIST_MAX (SF_ERR_ARG otherwise): with
 * that, "the list did not fit" means the same here as in sf_observe_overflow_device — count > cap, or the 0xffffffff
 * marker — and the two libraries never disagree about which agents fall back to the dense row.  Such an agent is
 * evaluated on an empty observation and counted: sf_policy_sparse_overflows() returns (and
 * clears) that count — non-zero means the caller should have taken the dense pair of calls for that step. */
#define SF_POLICY_LIST_MAX 2048 /* an observation of the BASELINE configurations has ~250-300 non-zeros */
int sf_policy_forward_sparse(sf_policy *p, const uint32_t *d_keys, const float *d_vals, const uint32_t *d_counts,
                             const float *d_pov, int32_t cap, int32_t agents, float *d_probs, float *d_value);
/* The same with a dense fallback, so that no agent is ever evaluated on a blank window: the agents whose list did not
 * fit are redone from their rows of d_dense (what sf_observe_overflow_device wrote: [agents][32][31][31]; the other rows
 * are never read) by a second launch that is idle when every list fitted.  Results equal the dense pair of calls
 * bit for bit for every agent; nothing is counted in sf_policy_sparse_overflows. */
int sf_policy_forward_sparse_or_dense(sf_policy *p, const uint32_t *d_keys, const float *d_vals, const uint32_t *d_counts,
                                      const float *d_pov, int32_t cap, int32_t agents, const float *d_dense,
                                      float *d_probs, float *d_value);
int sf_policy_sparse_overflows(sf_policy *p, int32_t *count);

/* The tail of Agent::predict() + Agent::update() (Agent.hpp:200-222): v[0] = 0.5, v[i>0] *= 0.5/(1-v[0]+1e-5),
 * draw from discrete_distribution(v) (greedy != 0: arg-max of v instead), store the one-hot as the agent's
 * action_input (update_actions) and write command char action_string[a] to d_cmd[agent] (gameplay::bot,
 * Custom.hpp:160-163).  The reference seeds std::mt19937 from std::random_device per call, so only the
 * distribution is specified; here draw i of agent a is a counter-based hash of (seed, a, i).
 * d_action (device, int32 per agent) may be NULL. */
int sf_policy_act(sf_policy *p, const float *d_probs, int32_t agents, const char *action_string, uint64_t seed,
                  int32_t greedy, uint8_t *d_cmd, int32_t *d_action);

/* sf_policy_act under an action mask: the draw honours what sf_action_mask_device (strikeforce.h) says would do anything.
 * d_action_mask: device uint32 per agent, bit j = action_string[j] is effective — sf_action_mask_io.d_actions for the same
 * action string.  Per agent: v is scaled as in sf_policy_act (v[0] = 0.5, the rest scaled to 0.5 in all); every v[k] whose
 * bit is clear becomes 0; bit 0 counts as set whatever the word says, so the word 0 of a dead seat yields action 0 ('+' in
 * the bots' strings); then the same sum, the same hashed draw (greedy != 0: the arg-max, first maximum) and the same one-hot
 * into action_input follow, and d_cmd, d_action and the policy's draw counter advance exactly as in sf_policy_act.  With
 * every bit set the call is sf_policy_act bit for bit: command, action, memory, and the next call's draws.  A masked action
 * is never drawn.
 * d_probs_out (device, float32 [agents][9], may be NULL) receives v[k] / tot (IEEE division): the distribution the action was
 * drawn from, which is what sf_rollout_record takes as d_probs.  A masked entry is exactly 0 there, so its log is -inf: a
 * learner takes log-probabilities of the drawn action only (never masked), or masks the entropy term the same way.
 * One launch on the policy's stream.  The fused sf_policy_predict_sparse keeps drawing unmasked: the masked closed loop is
 * the forward (act = 0) + sf_action_mask_device + this call. */
int sf_policy_act_masked(sf_policy *p, const float *d_probs, int32_t agents, const char *action_string, uint64_t seed,
                         int32_t greedy, const uint32_t *d_action_mask /* sf_action_mask_io.d_actions */,
                         uint8_t *d_cmd, int32_t *d_action /* may be NULL */, float *d_probs_out /* may be NULL, [agents][9] */);

/* Agent::predict() + Agent::update() as the ONE call they are in the reference (Agent.hpp:200-222), for the closed loop
 * on the device: sf_policy_reset_memory + sf_policy_forward_sparse(_or_dense) + sf_policy_act in the forward's two
 * launches, with the same results bit for bit as the three calls in that order (tests/test_gpu_policy.py).
 *   d_keys .. cap   the observation lists (sf_observe_sparse_device), as sf_policy_forward_sparse takes them
 *   d_dense         optional: dense rows for the lists that did not fit (sf_observe_overflow_device); without it such
 *                   agents are evaluated on a blank window and counted (sf_policy_sparse_overflows)
 *   d_reset_mask    optional, one byte per agent (sf_done_device's layout): non-zero = this agent's game restarted, it
 *                   starts from a new Agent's memory (zero state, "no action" as its last action) — gameplay.hpp:481
 *   d_reset_words   optional, the same flags where the environment keeps them (sf_done_view_device): agent a reads
 *                   word (a / reset_group) * reset_stride — saves the sf_done_device launch
 *   action_string, seed, greedy, d_cmd, d_action (may be NULL)   as in sf_policy_act
 *   d_probs, d_value   as in sf_policy_forward_sparse
 * The masks are read by the launch, in stream order: what sf_step_device left there is what counts. */
typedef struct sf_policy_predict_io {
  const uint32_t *d_keys;
  const float *d_vals;
  const uint32_t *d_counts;
  const float *d_pov;
  int32_t cap;
  const float *d_dense;
  const uint8_t *d_reset_mask;
  const int32_t *d_reset_words;
  int32_t reset_stride, reset_group;
  const char *action_string;
  uint64_t seed;
  int32_t greedy;
  float *d_probs, *d_value;
  uint8_t *d_cmd;
  int32_t *d_action;
} sf_policy_predict_io;
int sf_policy_predict_sparse(sf_policy *p, const sf_policy_predict_io *io, int32_t agents);

/* ---- bot-1's reward network (StrikeForce-client/bots/bot-1/RewardNet.hpp) -------------------------------------------
 * The newer bots evaluate a second network every tick: RewardNet::get_reward(one_hot(action), imitate, state)
 * (Agent.hpp:227, RewardNet.hpp:244-259) runs the GAIL discriminator RewardModel on the observation and the action just
 * drawn and returns log D — the only per-step reward the reference has.  RewardModel (RewardNet.hpp:138-167) is the
 * network above with one head: ResB, GameCNN and Backbone (RewardNet.hpp:26-136) are Modules.hpp:26-136 character for
 * character, and its head is AgentModel's `value` head, ResB(160, 3) + Linear(160, 1) + sigmoid (:147-149, :161-165).
 * What differs: forward(action, x) calls update_actions(action) first (:162), so the one-hot inside pov is the action of
 * THIS tick; there is no policy head; the caller takes torch::log of the output (:257).
 *
 * A reward model is an sf_policy object of a second kind.  It has its own recurrent state per agent (every game builds a
 * new Agent and with it a new RewardNet, Agent.hpp:95) and shares sf_policy_destroy, sf_policy_reset_memory(_n),
 * sf_policy_get_memory / _set_memory, sf_policy_set_stream / _synchronize, sf_policy_kernel_time* and
 * sf_policy_sparse_overflows with the policy.  The entries that evaluate a network are per kind: sf_policy_forward*,
 * sf_policy_predict_sparse, sf_policy_act and sf_policy_features on a reward model, or sf_reward_forward /
 * sf_reward_sparse on a policy, return SF_ERR_STATE.  Inference only: training (RewardNet.hpp:265-) is out of
 * scope, as the PPO learner is.
 *
 * new RewardNet + load of RewardModel's parameters (RewardNet.hpp:172-216): the backbone.* and value.* fields of w; the
 * policy_* fields are not looked at and may be NULL.  Same environment switches as sf_policy_create (SF_POLICY_LAYERED,
 * SF_POLICY_FUSED_TAIL, ...).  Memory starts as after reset_memory(). */
int sf_reward_create(const sf_policy_weights *w, int32_t max_agents, int32_t device, sf_policy **out);

/* RewardModel::forward(one_hot(d_action[a]), obs) (RewardNet.hpp:161-166) for agents [0, agents) on the dense
 * observation, the cross-check form as sf_policy_forward is for the policy: d_disc[a] = sigmoid(value head)  (:165),
 * d_reward[a] = the f32 log of d_disc[a], the f32 value as stored, rounded once (:257; D == 0 gives -inf as torch::log
 * does, never NaN).  Either output may be NULL, not both.  d_action (device, int32 per agent) is the index of the action drawn this
 * tick — sf_policy_predict_sparse's d_action; an index outside [0, 9) means 0, "no action" (undefined in the reference).
 * Its one-hot is the agent's action_input after the call (what update_actions leaves; sf_policy_get_memory shows it),
 * and every agent's h_state advances. */
int sf_reward_forward(sf_policy *r, const float *d_obs, const int32_t *d_action, int32_t agents, float *d_disc, float *d_reward);

/* The same on the observation in list form, with the restart flags folded in: the hot path, two launches and no host
 * synchronisation, to be issued right behind sf_policy_predict_sparse on the same stream (it reads that call's
 * d_action).  Needs the fused tail.
 *   d_keys .. cap, d_dense                            as in sf_policy_predict_io; same results as sf_reward_forward on the
 *                                                     dense image bit for bit
 *   d_reset_mask / d_reset_words, reset_stride, reset_group   as in sf_policy_predict_io: a restarted game's agent starts
 *                                                     from h = 0 (a new RewardNet, Agent.hpp:95); its action slot is still
 *                                                     the action given, since forward() overwrites what reset_memory() sets
 *   d_action, d_disc, d_reward                        as in sf_reward_forward */
typedef struct sf_reward_io {
  const uint32_t *d_keys;
  const float *d_vals;
  const uint32_t *d_counts;
  const float *d_pov;
  int32_t cap;
  const float *d_dense;
  const uint8_t *d_reset_mask;
  const int32_t *d_reset_words;
  int32_t reset_stride, reset_group;
  const int32_t *d_action;
  float *d_disc, *d_reward;
} sf_reward_io;
int sf_reward_sparse(sf_policy *r, const sf_reward_io *io, int32_t agents);

/* Read/write one agent's recurrent state for tests: h [2][160] and the action one-hot [9] (host buffers). */
int sf_policy_get_memory(sf_policy *p, int32_t agent, float *h, float *action_input);
int sf_policy_set_memory(sf_policy *p, int32_t agent, const float *h, const float *action_input);

/* The same for many agents in one launch, storage the caller's: the network memory that goes with a saved or forked arena
 * (strikeforce.h sf_snapshot_save / sf_snapshot_load), for policy and reward objects alike.  Agents [0, agents) are looked
 * at.  Many agents may name one row when reading rows (the fork); two agents writing one row is a caller error whose only
 * guarantee is memory safety.  A row index outside [-1, rows) is skipped like -1 and never dereferenced.  One launch in
 * stream order on the object's stream: no allocation, no copy, no host synchronisation.  SF_ERR_ARG: a null object or
 * buffer, agents outside [1, max_agents], rows < 1, or a buffer that is not device memory of the object's device, is not
 * 4-byte aligned or is shorter than stated (the checks sf_policy_load_weights makes); nothing is launched then. */
/* to_rows != 0: agent g's h[2][160] and action one-hot[9] -> row d_row_of_agent[g];  0: row -> agent.  -1: agent skipped. */
int sf_policy_memory_rows(sf_policy *p, int32_t to_rows, float *d_h /*[rows][2][160]*/, float *d_action /*[rows][9]*/,
                          const int32_t *d_row_of_agent, int32_t rows, int32_t agents);

int sf_policy_set_stream(sf_policy *p, void *hip_stream);
int sf_policy_synchronize(sf_policy *p);

/* Device time of the matrix kernels of the forward passes since the last call (HIP events on the library's
 * stream): *ms = summed duration of the MFMA GEMM launches, *flop = their algorithmic flop count
 * (2*M*N*K each), *launches = how many. */
int sf_policy_kernel_time(sf_policy *p, int32_t enable, float *ms, double *flop, int32_t *launches);
/* The same, split by matrix pipe: index 0 = launches on the f32 MFMA (k_gemm), index 1 = launches of the bf16-split
 * kernel (k_gemm_b3: conv1 / conv2 at M >= 16 384).  flop[] is the algorithmic 2*M*N*K in both; the split kernel
 * executes six bf16 products per algorithmic one. */
int sf_policy_kernel_time_ex(sf_policy *p, int32_t enable, float ms[2], double flop[2], int32_t launches[2]);
/* The same by kernel: 0 k_gemm (f32 MFMA) + fix-ups, 1 k_gemm_b3 (conv1 / conv2 on the bf16 pipe; layered form only),
 * 2 the launch that takes the observation's non-zeros — k_feat_list, the composed convolution stack (layered form:
 * k_conv0_sparse); flop[2] = 0: the useful work depends on the lists, 2 * 160 per non-zero — 3 k_tail (GRU cells +
 * combined_processor + heads; conv3 too in the layered form). */
int sf_policy_kernel_time_by_kernel(sf_policy *p, int32_t enable, float ms[4], double flop[4], int32_t launches[4]);

/* The matrix kernel on its own, for unit tests and roofline measurements: C[M][ldc] = A[M][lda] * W[N][K]^T + bias
 * (bias may be NULL), all device pointers, f32; K % 32 == 0, N % 160 == 0, lda % 4 == 0.  Every Linear / GRU gate
 * product of the network goes through this path; the convolutions use the same kernel with an im2col gather. */
int sf_policy_gemm(sf_policy *p, const float *d_a, int32_t lda, const float *d_w, const float *d_bias, float *d_c,
                   int32_t ldc, int32_t m, int32_t n, int32_t k);

/* The same product through the bf16-split kernel that conv1 and conv2 use once M >= 16 384 (k_gemm_b3: every f32
 * operand as three bf16 parts, six v_mfma_f32_32x32x16_bf16 per block instead of eight f32 ones, f32-level error:
 * |err| <= 2e-6 * sum|a*w|).  W is split on the device by this call (the network's own weights are split once at
 * sf_policy_create); synchronous.  For unit tests and roofline measurements. */
int sf_policy_gemm_split(sf_policy *p, const float *d_a, int32_t lda, const float *d_w, const float *d_bias, float *d_c,
                         int32_t ldc, int32_t m, int32_t n, int32_t k);

/* Test hook: GameCNN::forward alone (Modules.hpp:66-71) — the 160 features behind the four convolutions, before any
 * normalisation — for agents [0, agents) from the dense observations d_obs, into d_feat [agents][160] (device).  The
 * composed matrix by default, the four layers one after the other under SF_POLICY_LAYERED=1.  No recurrent state is
 * touched. */
int sf_policy_features(sf_policy *p, const float *d_obs, int32_t agents, float *d_feat);

int sf_policy_abi_version(void);

/* ---- the rollout buffer: bot-1's T-step record, returns and advantages (StrikeForce-client/bots/bot-1/Agent.hpp) --------
 * One reference `Agent` keeps five vectors per game — states, log_probs, values, rewards, actions (Agent.hpp:200-204, 227,
 * 233-234, 301-302) — fills them for T = 1024 ticks, then runs computeReturns() (:333-339) and train_log() (:341-351) over
 * them; its PPO epochs and RewardNet::train_epoch forward states[i] again from a fresh memory (:389-396,
 * RewardNet.hpp:265-274).  An sf_rollout does that bookkeeping and that gradient-free arithmetic for every agent of a
 * batch on the device, behind sf_policy_predict_sparse and sf_reward_sparse.  The learners themselves — gradients, AdamW,
 * backups — stay out of scope.
 *
 * Storage is the caller's, as every other buffer of this library is: device pointers, slot-major, for the `agents` and T
 * given to sf_rollout_create.  The library owns the per-agent cursor fill[agents] and three counters.
 *   keys, vals   [T][agents][list_cap]   states.push_back(state) (:201) as the observation list; 16-byte aligned
 *   counts       [T][agents]             the list's count as it came
 *   pov          [T][agents][160]        the five centre cells; 16-byte aligned
 *   action       [T][agents] int32       actions.push_back(action) (:234)
 *   logp         [T][agents][9]          log_probs.push_back(torch::log(output[0])) (:204): the f32 log, rounded once
 *   value        [T][agents]             values.push_back(output[1]) (:203)
 *   reward       [T][agents]             rewards.push_back(get_reward(...)) (:227)
 *   disc         [T][agents]             optional (NULL: not kept): D beside its log
 *   imitate      [T][agents] u8          optional (NULL: not kept): get_reward's `imitate` argument
 * keys == NULL: states are not kept (vals, counts and pov are not looked at).  Every other pointer is required. */
typedef struct sf_rollout sf_rollout;
typedef struct sf_rollout_buffers {
  uint32_t *keys;
  float *vals;
  uint32_t *counts;
  float *pov;
  int32_t *action;
  float *logp, *value, *reward;
  float *disc;
  uint8_t *imitate;
} sf_rollout_buffers;

/* SF_ERR_ARG: T odd or below 2 (the reference's sum_rewards[i / (T / 2)], :344, indexes out of bounds for an odd T);
 * list_cap % 4 != 0 or outside [4, SF_POLICY_LIST_MAX] (only looked at when states are kept); agents outside
 * [1, 1048576]; a required pointer NULL or keys / vals / pov not 16-byte aligned.  Every cursor starts at 0. */
int sf_rollout_create(const sf_rollout_buffers *b, int32_t agents, int32_t T, int32_t list_cap, int32_t device, sf_rollout **out);
void sf_rollout_destroy(sf_rollout *r);
int sf_rollout_set_stream(sf_rollout *r, void *hip_stream);
int sf_rollout_synchronize(sf_rollout *r);

/* One tick of agents [0, agents): Agent::predict()'s and Agent::update()'s push_backs (:201-204, 227, 234).  One launch,
 * no synchronisation; issue it behind sf_reward_sparse and in front of sf_step_device on the same stream, so that it
 * reads the restart flags those two calls read.
 *   d_keys .. cap        this tick's observation lists, as in sf_policy_predict_io; not looked at when states are not kept
 *   d_probs [agents][9], d_value [agents], d_action [agents]   sf_policy_predict_sparse's outputs
 *   d_reward [agents]    sf_reward_sparse's output; d_disc [agents], d_imitate [agents]: required exactly when the
 *                        buffer of that name is kept, not looked at otherwise
 *   d_reset_mask / d_reset_words, reset_stride, reset_group    as in sf_policy_predict_io
 * Per agent, in this order:
 *   1. fill == T: the agent is ready.  Nothing is written, its restart flag is not looked at, the tick is counted in
 *      `dropped` — the `if (is_training ...) return;` of :219.
 *   2. its restart flag is set: fill = 0 (a new Agent per game; ~Agent trains nothing from a partial buffer).
 *   3. the tick is appended at slot `fill`: min(count, list_cap) list entries (never more than cap) and the 160 pov floats;
 *      the count as it came — above list_cap, or the 0xffffffff marker, it is stored unchanged and counted in
 *      `missing_states`, so that sf_policy_forward_sparse on the stored row sees "did not fit" as the live call did;
 *      action, value, reward, disc and imitate bit for bit; logp[j] = the f32 log of d_probs[j]; then fill += 1.
 *      Entries of a stored row behind the count are not written. */
typedef struct sf_rollout_step {
  const uint32_t *d_keys;
  const float *d_vals;
  const uint32_t *d_counts;
  const float *d_pov;
  int32_t cap;
  int32_t agents;
  const float *d_probs, *d_value;
  const int32_t *d_action;
  const float *d_reward, *d_disc;
  const uint8_t *d_imitate;
  const uint8_t *d_reset_mask;
  const int32_t *d_reset_words;
  int32_t reset_stride, reset_group;
} sf_rollout_step;
int sf_rollout_record(sf_rollout *r, const sf_rollout_step *io);

/* *d_fill: the cursors (device, int32 per agent, the library's; valid until sf_rollout_destroy).  d_mask[a] (device, one
 * byte per agent) = fill[a] == T, the mask sf_policy_reset_memory takes (model->reset_memory(), :432).  sf_rollout_status
 * synchronises: *ready = how many agents are ready now; *dropped and *missing_states count since sf_rollout_create.
 * Any of its outputs may be NULL. */
int sf_rollout_fill_device(sf_rollout *r, const int32_t **d_fill);
int sf_rollout_ready_device(sf_rollout *r, uint8_t *d_mask);
int sf_rollout_status(sf_rollout *r, int32_t *ready, int64_t *dropped, int64_t *missing_states);

/* For the READY agents only (rows of the others are not touched), all [T][agents] device arrays, each may be NULL:
 *   d_returns[T-1] = (1 - gamma) * reward[T-1];  d_returns[i] = gamma * d_returns[i+1] + (1 - gamma) * reward[i]   (:333-339)
 *   d_logv = the f32 log of value (:401, :407);  d_adv = d_returns - d_logv   (:407)
 *   d_stats [agents][4] (16-byte aligned) = r_avg0, r_avg1 — the sums of reward over each half of the buffer, DIVIDED BY T
 *   as :347-348 divide them — and n_avg0, n_avg1, the share of action 0 in each half (:349-350)
 * f32 in the reference's operation order: (1 - gamma) is an f32 subtraction, every product is rounded before the add (no
 * fused multiply-add), the sums are sequential in slot order; infinities and NaNs fall out as IEEE gives them (D == 0 is a
 * reward of -inf).  train_log's mean of exp(log_probs) is a log line and is left to the caller. */
int sf_rollout_returns(sf_rollout *r, float gamma, float *d_returns, float *d_logv, float *d_adv, float *d_stats);

/* clear() of the five vectors (:430-431): fill = 0 for every ready agent (d_mask NULL), or for the agents whose byte in
 * d_mask (device, one per agent) is non-zero, ready or not. */
int sf_rollout_release(sf_rollout *r, const uint8_t *d_mask);

/* The four device pointers of slot t, with *cap = list_cap: states[t] of every agent, as sf_policy_forward_sparse and
 * sf_reward_sparse take it.  SF_ERR_STATE when states are not kept; SF_ERR_ARG for t outside [0, T). */
int sf_rollout_state(sf_rollout *r, int32_t t, const uint32_t **d_keys, const float **d_vals, const uint32_t **d_counts,
                     const float **d_pov, int32_t *cap);

/* AgentModel::update_actions(one_hot(d_action[a])) (Agent.hpp:396, RewardNet.hpp:271-272) for agents [0, agents) of a
 * policy or a reward model; an index outside [0, 9) means 0, as in sf_reward_forward.  With it the stored rollout can be
 * replayed: a fresh agent always starts at slot 0, so sf_policy_reset_memory followed by rows 0..T-1 — forward on
 * the state of slot t, then this call on action[t] — reproduces every ready agent's sequence.
 * A block stored under the continuing rule (sf_rollout_continue) stays replayable: with the memory the agents had at slot 0
 * restored, the following sequence reproduces every stored logp and value.  For each t: sf_policy_reset_memory_n(first[t]),
 * then forward on sf_rollout_state(t), then this call on action[t].  The memory at slot 0 comes from resetting at the
 * hand-over, as Agent.hpp:432 does, or from keeping it with sf_policy_memory_rows. */
int sf_policy_update_actions(sf_policy *p, const int32_t *d_action, int32_t agents);

/* ---- the rollout buffer across game ends: a [T][agents] block every T ticks, and GAE(lambda) over it ---------------------
 * The per-game rule above is the reference Agent's; a learner that trains on fixed-length blocks wants every tick kept, the
 * game ends inside a block marked, and returns that bootstrap from the state behind the last slot.
 *
 * sf_rollout_continue switches an sf_rollout to the continuing rule (d_first set: the caller's [T][agents] bytes, device)
 * or back to the per-game rule (d_first NULL).  Stream-ordered, no synchronisation; it sets every cursor to 0.  Under the
 * continuing rule sf_rollout_record does, per agent, in this order:
 *   1. fill == T: the agent is ready.  Nothing is written, the tick is counted in `dropped`, as under the per-game rule.
 *   2. otherwise the tick is appended at slot `fill`: everything the per-game rule stores, bit for bit, and
 *      first[slot] = 1 if the agent's restart flag is set in this call (d_reset_mask, or d_reset_words / reset_stride /
 *      reset_group; neither given: 0), else 0; then fill += 1.  A set restart flag never moves the cursor.
 * sf_rollout_ready_device, sf_rollout_status, sf_rollout_release and sf_rollout_state work under both rules unchanged. */
int sf_rollout_continue(sf_rollout *r, uint8_t *d_first);

/* Returns, values and advantages of the READY agents (rows of the others are not touched), under either rule; under the
 * per-game rule `first` counts as all zero.  Per agent, in f32, every product rounded before its add (no fused
 * multiply-add), in slot order from T-1 down:
 *   V_t   = the f32 log of value[t] when log_values is set (the reference's head, :401,407), else value[t]; V_T the same
 *           of d_next_value
 *   x_t   = reward_scale * reward[t]
 *   end_t = first[t+1] for t < T-1; for t = T-1 the next tick's restart flag (d_next_mask, or d_next_words / next_stride /
 *           next_group as in sf_rollout_step; both NULL: that tick continues the game)
 *   G_t   = x_t                      if end_t is set, or if t = T-1 and d_next_value is NULL — the other term is ABSENT,
 *                                    not a zero that is added
 *         = gamma * boot_t + x_t     otherwise, with boot_{T-1} = V_T and for t < T-1
 *           boot_t = G_{t+1} (lambda == 1), V_{t+1} (lambda == 0), else (1 - lambda) * V_{t+1} + lambda * G_{t+1} with
 *           (1 - lambda) an f32 subtraction
 *   d_returns = G, d_v = V, d_adv = G - V     ([T][agents] device arrays, each may be NULL, not all three)
 * This is GAE(lambda): G_t - V_t = delta_t + gamma * lambda * (1 - end_t) * (G_{t+1} - V_{t+1}).  Skipping a term, where a
 * product with an exact 0 or 1 would stand, keeps a reward of -inf or a log of 0 from turning its neighbours into NaN, and
 * makes the reference a special case: lambda = 1, log_values = 1, reward_scale = 1.f - gamma (in f32), no next value and no
 * game end give sf_rollout_returns' d_returns, d_logv and d_adv in every bit.
 * A restart by sf_reset_arenas (a step limit) is a game end like any other: bootstrapping a cut game from its own last
 * state is out of scope.
 * Two launches — V, fully parallel; then the recursion, one lane per agent — on the rollout's stream, no synchronisation.
 * With d_v NULL and log_values set, V goes to a [T][agents] array of the library's, allocated by the first such call.
 * SF_ERR_ARG: gamma or lambda outside [0, 1] or NaN; both d_next_mask and d_next_words given; next_stride or next_group
 * below 1 with d_next_words; every output NULL. */
typedef struct sf_rollout_gae_io {
  float gamma, lambda, reward_scale;
  int32_t log_values;
  const float *d_next_value;
  const uint8_t *d_next_mask;
  const int32_t *d_next_words;
  int32_t next_stride, next_group;
  float *d_returns, *d_v, *d_adv;
} sf_rollout_gae_io;
int sf_rollout_gae(sf_rollout *r, const sf_rollout_gae_io *io);

/* ---- the rollout buffer's states as dense rows: what a learner's own network reads --------------------------------------
 * The reference's epochs run model->forward(states[i]) with gradients on the dense 32 x 31 x 31 observation
 * (Agent.hpp:392, RewardNet.hpp:265-274); the buffer keeps states[i] as the observation's list.  This call expands stored
 * lists into dense rows of the caller's, in the element type and layout the caller's module wants.  One launch on the
 * rollout's stream, no synchronisation.
 *
 * Row b is the cell d_cells[b] = t * agents + agent (any order, repeats allowed), or with d_cells NULL the cell
 * (slot, agent0 + b).  Every one of a row's 30 752 elements is written:
 *   a good cell — inside [0, T * agents), stored count <= list_cap: for each entry e < count the element at the position
 *     the key k names holds vals[e]; NCHW position ((k & 511) / 9 * 31 + (k >> 9 & 31)) * 31 + (k >> 14 & 31), NHWC the
 *     same three numbers as ((k >> 9 & 31) * 31 + (k >> 14 & 31)) * 32 + (k & 511) / 9; every other element is +0;
 *     d_valid[b] = 1.  Lists need not be sorted; of two entries that name one position either value stays.  An entry whose
 *     key names no position (channel above 31, row or column above 30; the simulator writes none) is skipped.
 *   a bad cell — its list did not fit (count > list_cap, the 0xffffffff marker included) or the cell lies outside the
 *     buffer: the whole row is +0 and d_valid[b] = 0.  Nothing is read through an out-of-range cell.
 * SF_DENSE_F32 keeps the value's bits (-0, infinities, NaN payloads); SF_DENSE_BF16 and SF_DENSE_F16 round the f32 value
 * to nearest even (F16 overflows to infinity and keeps subnormals; a NaN stays a NaN, payload unspecified).
 * `fill` is not looked at: a slot behind an agent's cursor expands to whatever is stored there.
 * SF_ERR_STATE: states are not kept.  SF_ERR_ARG: rows outside [1, SF_ROLLOUT_DENSE_ROWS_MAX] (the cap keeps every
 * destination offset below 2^31 bytes); with d_cells NULL, slot outside [0, T), agent0 < 0 or agent0 + rows > agents;
 * an unknown dtype or layout; d_dense NULL or not 16-byte aligned. */
#define SF_DENSE_F32 0
#define SF_DENSE_BF16 1
#define SF_DENSE_F16 2
#define SF_DENSE_NCHW 0   /* [rows][32][31][31], sf_observe_device's own order */
#define SF_DENSE_NHWC 1   /* [rows][31][31][32], channel fastest */
#define SF_ROLLOUT_DENSE_ROWS_MAX 16384
typedef struct sf_rollout_dense_io {
  const int32_t *d_cells;  /* device, [rows]: cell = t * agents + agent; NULL: cells (slot, agent0 + b) */
  int32_t slot, agent0;    /* looked at only when d_cells is NULL */
  int32_t rows;
  int32_t dtype, layout;
  void *d_dense;           /* device, [rows][30752] elements of dtype, contiguous, 16-byte aligned */
  uint8_t *d_valid;        /* device, [rows], may be NULL */
} sf_rollout_dense_io;
int sf_rollout_dense(sf_rollout *r, const sf_rollout_dense_io *io);

/* ---- parameters in: what a learner hands back ---------------------------------------------------------------------------
 * The parameters the next forward sees are these (optimizer->step(), bots/bot-1/Agent.hpp:415-417, then model->forward,
 * :202; RewardNet::train_epoch does the same to the discriminator, :428): d_w holds DEVICE pointers, same fields / shapes /
 * torch layouts as for sf_policy_create.  Works on a policy and on a reward model (policy_* fields not looked at there).
 *
 * Images refreshed.  Every image sf_policy_create derives is derived again, in the form the object was created in (folded
 *   or layered, fused tail or not, f32-conv, dense-conv0: the environment switches are NOT read again): conv0's weights and
 *   their transpose, the permuted conv1..3, the bf16-split images of conv1 and conv2, the composed matrix F; the GRU
 *   matrices and biases, the padded combined_processor; the ResB layers, the heads and their 16-row paddings; k_tail's whole
 *   weight block in its stream order.
 * Bit for bit.  After the call every image holds bit for bit what sf_policy_create would have put there for the same
 *   parameters; pad regions stay zero.  (Parameters are finite: a NaN the bf16 split makes of an infinity has no
 *   specified sign.)
 * Stream order.  All work is launched on the object's stream (sf_policy_set_stream), the composition of F too.  A forward
 *   issued before the call sees the old parameters, one issued after it the new ones; no host synchronisation is needed
 *   between them.  The sources are read in stream order and must stay valid and unchanged until the stream has passed the
 *   call.
 * Allocation and synchronisation.  The first call on an object in the folded form allocates the composition's f64 workspace,
 *   97.3 MB, and keeps it until sf_policy_destroy (layered form: nothing).  Later calls allocate nothing; no call
 *   synchronises.
 * State left alone.  Per-agent memory (h, action_input), stream, timers and the overflow counter are untouched: the caller
 *   calls sf_policy_reset_memory as Agent.hpp:432 does.
 * Validation.  Everything is validated before the first launch, and a failed call leaves the object exactly as it was:
 *   SF_ERR_ARG for a NULL object or struct, an abi_version mismatch, a NULL field this kind of object needs, a pointer that
 *   is not 4-byte aligned, a pointer that is not device memory of the object's device (hipPointerGetAttributes), or one
 *   whose extent — the field's float count — does not lie inside its allocation (hipMemGetAddressRange).  A host pointer
 *   handed to a kernel would fault the device: that is what the guard is for.
 * Alignment.  Sources need only 4-byte alignment (parameters carved out of one flat tensor). */
int sf_policy_load_weights(sf_policy *p, const sf_policy_weights *d_w);

/* Test hook: one 64-bit digest per device image the object derives from its parameters, over the WHOLE allocation of each
 * (pads included), into out_host.  *count in: capacity, out: how many (SF_ERR_ARG if the capacity is too small; 40 is
 * enough).  Order: conv0's weights, their transpose, the permuted conv1, conv2, conv3, the split images of conv1 and conv2,
 * F (folded form only: the layered form has one entry less); per GRU cell g = 0, 1: weight_ih, weight_hh, bias_ih, bias_hh;
 * combined_processor's padded weight, its bias; per head (a policy: policy, value; a reward model: value) the three ResB
 * weights, the three ResB biases, the output weight, its bias, the 16-row weight, the 16-row bias; k_tail's block.  39
 * entries for a folded policy, 29 for a folded reward model.  A digest is the sum mod 2^64 of a position-keyed mix of the
 * image's 32-bit words: equal images give equal digests, on any object.  Synchronises the object's stream. */
int sf_policy_weights_digest(sf_policy *p, uint64_t *out_host, int32_t *count);

/* ---- several networks in one match: routing agents to parameter sets ----------------------------------------------------
 * In the reference every commanded human owns its network: gameplay::prepare does `player.agent = new Agent`
 * (bots/bot-0.5/Custom.hpp:161-165), the constructor loads that agent's own backup_dir/model.pt (bots/bot-1/Agent.hpp:84-101),
 * and every seat of an online Battle is a client of its own, built with its own bot and holding its own checkpoint
 * (gameplay.hpp:57-207, selected_agent.hpp:25): that is how two bots, or two checkpoints of one, meet in one match.  An
 * sf_policy has ONE parameter set and evaluates rows [0, agents) of the buffers it is given.  An sf_route is the static
 * assignment of an environment's agents to up to SF_ROUTE_MAX_NETS such objects: sf_route_gather copies each network's
 * agents into rows of that network's own, sf_route_scatter copies the results back into the environment's order, both on
 * the device in stream order with no host work per tick.  Between them every entry above (sf_policy_predict_sparse,
 * sf_reward_sparse, sf_rollout_record, sf_policy_load_weights) works per network, unchanged, on count(k) rows.
 *
 * Slots.  Agent a of network k = assign[a] gets slot s = its rank among k's agents in ascending a.  The mapping never
 *   changes, so slot s of network k is one agent's h_state / action_input for the whole run (one `Agent` object).
 * Action draws.  sf_policy_predict_sparse keys its draw by the row it sees: behind a route, draw i of slot s is the hash of
 *   (seed, s, i), not of (seed, a, i).  Give every network a seed of its own, or slot s of two networks draws alike. */
#define SF_ROUTE_MAX_NETS 8
typedef struct sf_route sf_route;

/* assign (host, [agents]): assign[a] in [0, nets), or -1 for nobody's — a scripted, random or remote player (Custom.hpp:
 * 161-165 only builds an Agent for a commanded human).  SF_ERR_ARG: a NULL pointer, agents outside [1, 1048576], nets
 * outside [1, SF_ROUTE_MAX_NETS], an assign[a] outside [-1, nets).  The object owns two small device tables: (net, slot) per
 * agent, and the agent per (net, slot). */
int sf_route_create(const int32_t *assign, int32_t agents, int32_t nets, int32_t device, sf_route **out);
void sf_route_destroy(sf_route *r);
int sf_route_set_stream(sf_route *r, void *hip_stream);
int sf_route_synchronize(sf_route *r);
/* *n = how many agents network `net` has (a network may have none); *d_agent_of_slot = its agents by slot (device, int32
 * [count], the library's; valid until sf_route_destroy).  SF_ERR_ARG for net outside [0, nets). */
int sf_route_count(sf_route *r, int32_t net, int32_t *n);
int sf_route_agents_device(sf_route *r, int32_t net, const int32_t **d_agent_of_slot);

/* One tick's observation, environment order, exactly as sf_policy_predict_io takes it (the state every Agent::predict() of
 * the tick is handed, Agent.hpp:200-201), and one network's rows of it: the caller's storage, count(k) rows. */
typedef struct sf_route_src {
  const uint32_t *d_keys;
  const float *d_vals;
  const uint32_t *d_counts;
  const float *d_pov;
  int32_t cap;
  const float *d_dense;          /* optional: [agents][32][31][31], rows of the agents whose list did not fit */
  const uint8_t *d_reset_mask;   /* optional, one byte per agent */
  const int32_t *d_reset_words;  /* optional: agent a reads word (a / reset_group) * reset_stride */
  int32_t reset_stride, reset_group;
} sf_route_src;
typedef struct sf_route_dst {
  uint32_t *d_keys; /* [n_k][cap] */
  float *d_vals;    /* [n_k][cap] */
  uint32_t *d_counts;
  float *d_pov;     /* [n_k][160] */
  int32_t cap;      /* the source's cap (SF_ERR_ARG otherwise) */
  float *d_dense;   /* optional: [n_k][32][31][31] */
  uint8_t *d_reset_mask; /* optional: [n_k] bytes, what sf_policy_predict_io.d_reset_mask takes */
} sf_route_dst;
/* ONE launch for all networks (dst[nets] travels in the kernel arguments; nothing is allocated or copied ahead of it).  Per
 * assigned agent, into row `slot` of its network: min(count, cap) list entries — nothing behind the count is written; the
 * count as it came, the 0xffffffff marker included, so that "did not fit" means to the network what it meant to the
 * environment; the 160 pov floats; the restart flag as one byte (a non-zero source byte or word gives 1, else 0: gameplay.hpp:
 * 481, a new Agent per game); the dense row ONLY for an agent whose list did not fit, and only if both src->d_dense and
 * dst[k].d_dense are given.  A network without agents, or a dst[k] whose pointers are all NULL, is skipped.  Copies are
 * 16 bytes wide where cap % 4 == 0 and both bases are 16-byte aligned, dwords otherwise.  SF_ERR_ARG: NULL r, src or dst; a
 * NULL list pointer or a cap outside [1, SF_POLICY_LIST_MAX] in src; a dst[k] that is neither complete (d_keys, d_vals,
 * d_counts, d_pov) nor all NULL, or whose cap differs from src->cap. */
int sf_route_gather(sf_route *r, const sf_route_src *src, const sf_route_dst *dst);

/* What the networks answered (Agent::predict()'s outputs and get_reward()'s, Agent.hpp:202-204, 227; the command char of
 * gameplay::bot, Custom.hpp:160-163): rows[k] is network k's compact storage, count(k) rows; env the environment-order
 * buffers of the same names, [agents] rows.  d_probs is [.][9].  Any pointer may be NULL on either side: that field is
 * skipped. */
typedef struct sf_route_rows {
  uint8_t *d_cmd;
  int32_t *d_action;
  float *d_probs, *d_value, *d_reward, *d_disc;
} sf_route_rows;
/* ONE launch for all networks: row a of every env buffer = row `slot` of the same-named buffer of a's network.  Rows of the
 * agents assigned to -1 are not touched: a scripted command the caller put into env->d_cmd survives. */
int sf_route_scatter(sf_route *r, const sf_route_rows *rows, const sf_route_rows *env);

#ifdef __cplusplus
}
#endif
#endif /* STRIKEFORCE_POLICY_H */
