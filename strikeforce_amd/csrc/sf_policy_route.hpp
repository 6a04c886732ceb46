// sf_policy_route.hpp — several networks in one match (include/strikeforce_policy.h, sf_route_*).  In the reference every
// commanded human owns its network: gameplay::prepare does `player.agent = new Agent` (StrikeForce-client/bots/bot-0.5/
// Custom.hpp:161-165), the constructor loads that agent's own backup_dir/model.pt (bots/bot-1/Agent.hpp:84-101), and every
// seat of an online Battle is a client built with its own bot (gameplay.hpp:57-207, selected_agent.hpp:25).  Here a network
// evaluates rows [0, n) of its buffers, so a route gives each network rows of its own: a static assignment of agents to
// networks, a gather of a tick's observation into each network's rows and a scatter of the results back into the
// environment's order.  Included at the end of sf_policy.hip (behind sf_rollout.hpp: rollout_copy2, and the host helpers).
//   k_route_gather    one wavefront per agent: its list, pov, count, restart flag (and dense row, if its list did not fit)
//                     into row `slot` of its network's buffers.  All networks in one launch: the destinations travel in the
//                     kernel arguments.
//   k_route_scatter   sixteen lanes per agent, one 32-bit word (or the command byte) each: a wave stores four agents'
//                     probabilities as 36 neighbouring floats.
// No LDS, no scratch; plain vector loads and stores.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <vector>

namespace sfp {

constexpr int ROUTE_NETS = SF_ROUTE_MAX_NETS;
constexpr int DENSE_FLOATS = SF_OBS_FLOATS;  // 30 752: 7 688 sixteen-byte units
static_assert(DENSE_FLOATS % 8 == 0, "a dense row is copied as two halves of whole 16-byte units");

// The environment-order buffers of one tick, as sf_policy_predict_io takes them.
struct RouteSrc {
  const uint32_t *keys;
  const float *vals;
  const uint32_t *counts;
  const float *pov;
  const float *dense;          // or null
  const uint8_t *reset_mask;   // [agents] or null
  const int32_t *reset_words;  // word (a / reset_group) * reset_stride, or null
  int reset_stride, reset_group;
  int cap, agents;
};
// One network's rows.  `vec`: bit 0 the list rows, bit 1 the pov rows, bit 2 the dense rows are 16-byte aligned on BOTH
// sides (the source's alignment is folded in by the host).  keys == null: the network is skipped.
struct RouteDst {
  uint32_t *keys;
  float *vals;
  uint32_t *counts;
  float *pov;
  float *dense;         // or null
  uint8_t *reset_mask;  // or null
  int vec;
};
struct RouteDsts {
  RouteDst net[ROUTE_NETS];
};
static_assert(sizeof(RouteDsts) + sizeof(RouteSrc) <= 1024, "the destinations travel in the kernel arguments");

__global__ __launch_bounds__(256) void k_route_gather(const int2 *__restrict__ slot_of, RouteSrc s, const RouteDsts d) {
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), l = threadIdx.x & 63;
  const int a = blockIdx.x * 4 + w;
  if (a >= s.agents) return;
  // (net, slot), the flags and the count: unconditional loads from addresses that are valid whatever the options
  const uint8_t *fmp = s.reset_mask ? s.reset_mask + a : reinterpret_cast<const uint8_t *>(slot_of);
  const int32_t *fwp = s.reset_words ? s.reset_words + (size_t)(a / s.reset_group) * (size_t)s.reset_stride : reinterpret_cast<const int32_t *>(slot_of);
  const int2 ns = slot_of[a];
  const uint8_t fm = *fmp;
  const int32_t fw = *fwp;
  uint32_t count = s.counts[a];
  const int net = __builtin_amdgcn_readfirstlane(ns.x), slot = __builtin_amdgcn_readfirstlane(ns.y);
  count = (uint32_t)__builtin_amdgcn_readfirstlane((int)count);
  const bool fresh = __builtin_amdgcn_readfirstlane((int)((s.reset_mask && fm != 0) || (s.reset_words && fw != 0))) != 0;
  if (net < 0) return;  // nobody's: a scripted, random or remote player
  const RouteDst &o = d.net[net];  // (uniform in the wave: scalar loads of the arguments)
  if (!o.keys) return;
  const int vec = o.vec;
  const uint32_t n = count < (uint32_t)s.cap ? count : (uint32_t)s.cap;  // the 0xffffffff marker: cap entries
  const uint32_t *sk = s.keys + (size_t)a * s.cap;
  const float *sv = s.vals + (size_t)a * s.cap;
  uint32_t *dk = o.keys + (size_t)slot * s.cap;
  float *dv = o.vals + (size_t)slot * s.cap;
  if (vec & 1) {
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
  float *dp = o.pov + (size_t)slot * HID;
  if (vec & 2) {
    if (l < HID / 4) reinterpret_cast<u32x4 *>(dp)[l] = reinterpret_cast<const u32x4 *>(sp)[l];
  } else {
    const Row3 r = row_load(sp, l);
    row_store(dp, l, r);
  }
  if (l == 0) {
    o.counts[slot] = count;  // as it came: "did not fit" means to the network what it meant to the environment
    if (o.reset_mask) o.reset_mask[slot] = fresh ? 1 : 0;
  }
  // the dense row, for an agent whose list did not fit only: the two halves of the row as rollout_copy2's two rows
  if (count > (uint32_t)s.cap && s.dense && o.dense) {
    const float *sd = s.dense + (size_t)a * DENSE_FLOATS;
    float *dd = o.dense + (size_t)slot * DENSE_FLOATS;
    if (vec & 4) rollout_copy2<u32x4, 4>(sd, sd + DENSE_FLOATS / 2, dd, dd + DENSE_FLOATS / 2, DENSE_FLOATS / 8, l);
    else rollout_copy2<uint32_t, 8>(sd, sd + DENSE_FLOATS / 2, dd, dd + DENSE_FLOATS / 2, DENSE_FLOATS / 2, l);
  }
}

// One network's compact result rows (a source), or the environment-order rows (the destination).  Any pointer may be null.
struct RouteRows {
  uint8_t *cmd;
  uint32_t *word[5];  // action (int32), value, reward, disc: one word per row; [4] probs: nine
};
struct RouteRowsAll {
  RouteRows net[ROUTE_NETS];
  RouteRows env;
};
constexpr int RS_LANES = 16;  // lanes per agent: 0..8 the probabilities, 9 action, 10 value, 11 reward, 12 disc, 13 the command

__global__ __launch_bounds__(256) void k_route_scatter(const int2 *__restrict__ slot_of, const RouteRowsAll r, int agents) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int a = e / RS_LANES, j = e % RS_LANES;
  if (a >= agents) return;
  const int2 ns = slot_of[a];
  if (ns.x < 0) return;  // nobody's: the row keeps what the caller put there
  const RouteRows &src = r.net[ns.x];
  if (j == 13) {
    if (src.cmd && r.env.cmd) r.env.cmd[a] = src.cmd[ns.y];
    return;
  }
  if (j > 13) return;
  const int f = j < ACT ? 4 : j - ACT;
  const uint32_t *from = src.word[f];
  uint32_t *to = r.env.word[f];
  if (!from || !to) return;
  const size_t so = j < ACT ? (size_t)ns.y * ACT + j : (size_t)ns.y, eo = j < ACT ? (size_t)a * ACT + j : (size_t)a;
  to[eo] = from[so];
}

// ---- the host side ----------------------------------------------------------------------------------------------------------
struct Route {
  int device = 0, agents = 0, nets = 0;
  hipStream_t stream = nullptr;
  int count[ROUTE_NETS] = {}, first[ROUTE_NETS] = {};  // agents of a network; where its agents start in agent_of
  int2 *slot_of = nullptr;     // [agents]: (net, slot), net = -1: nobody's
  int32_t *agent_of = nullptr;  // [assigned agents]: network 0's agents in ascending order, then network 1's, ...
  ~Route() {
    if (slot_of) (void)hipFree(slot_of);
    if (agent_of) (void)hipFree(agent_of);
  }
};
static int check_route(const Route *r, int net) {
  if (!r) return fail(SF_ERR_ARG, "null route");
  if (net < 0 || net >= r->nets) return fail(SF_ERR_ARG, "network index out of range for this route");
  return SF_OK;
}

}  // namespace sfp
using sfp::Route;

extern "C" {

int sf_route_create(const int32_t *assign, int32_t agents, int32_t nets, int32_t device, sf_route **out) {
  if (!assign || !out) return sfp::fail(SF_ERR_ARG, "null argument");
  if (agents < 1 || agents > (1 << 20)) return sfp::fail(SF_ERR_ARG, "agents must be 1..1048576");
  if (nets < 1 || nets > SF_ROUTE_MAX_NETS) return sfp::fail(SF_ERR_ARG, "nets must be 1..SF_ROUTE_MAX_NETS (8)");
  for (int a = 0; a < agents; ++a)
    if (assign[a] < -1 || assign[a] >= nets) return sfp::fail(SF_ERR_ARG, "assign[" + std::to_string(a) + "] is outside [-1, nets)");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return sfp::fail(SF_ERR_DEVICE, "no HIP device: a route has no CPU path");
  if (device < 0 || device >= n) return sfp::fail(SF_ERR_DEVICE, "device ordinal out of range");
  SFP_HIP(hipSetDevice(device));
  std::unique_ptr<Route> r(new Route());
  r->device = device, r->agents = agents, r->nets = nets;
  // slot = the agent's rank among its network's agents, in ascending agent order
  std::vector<int2> slot_of((size_t)agents);
  for (int a = 0; a < agents; ++a) {
    const int k = assign[a];
    slot_of[(size_t)a] = make_int2(k, k < 0 ? -1 : r->count[k]++);
  }
  int total = 0;
  for (int k = 0; k < nets; ++k) r->first[k] = total, total += r->count[k];
  std::vector<int32_t> agent_of((size_t)(total > 0 ? total : 1), -1);
  for (int a = 0; a < agents; ++a)
    if (assign[a] >= 0) agent_of[(size_t)(r->first[assign[a]] + slot_of[(size_t)a].y)] = a;
  if (hipMalloc(reinterpret_cast<void **>(&r->slot_of), slot_of.size() * sizeof(int2)) != hipSuccess ||
      hipMalloc(reinterpret_cast<void **>(&r->agent_of), agent_of.size() * sizeof(int32_t)) != hipSuccess)
    return sfp::fail(SF_ERR_MEMORY, "hipMalloc failed (route)");
  SFP_HIP(hipMemcpy(r->slot_of, slot_of.data(), slot_of.size() * sizeof(int2), hipMemcpyHostToDevice));
  SFP_HIP(hipMemcpy(r->agent_of, agent_of.data(), agent_of.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  *out = reinterpret_cast<sf_route *>(r.release());
  return SF_OK;
}

void sf_route_destroy(sf_route *r) { delete reinterpret_cast<Route *>(r); }

int sf_route_set_stream(sf_route *rr, void *hip_stream) {
  Route *r = reinterpret_cast<Route *>(rr);
  if (!r) return sfp::fail(SF_ERR_ARG, "null route");
  r->stream = reinterpret_cast<hipStream_t>(hip_stream);
  return SF_OK;
}

int sf_route_synchronize(sf_route *rr) {
  Route *r = reinterpret_cast<Route *>(rr);
  if (!r) return sfp::fail(SF_ERR_ARG, "null route");
  SFP_HIP(hipSetDevice(r->device));
  SFP_HIP(hipStreamSynchronize(r->stream));
  return SF_OK;
}

int sf_route_count(sf_route *rr, int32_t net, int32_t *n) {
  Route *r = reinterpret_cast<Route *>(rr);
  SFP_RC(sfp::check_route(r, net));
  if (!n) return sfp::fail(SF_ERR_ARG, "null argument");
  *n = r->count[net];
  return SF_OK;
}

int sf_route_agents_device(sf_route *rr, int32_t net, const int32_t **d_agent_of_slot) {
  Route *r = reinterpret_cast<Route *>(rr);
  SFP_RC(sfp::check_route(r, net));
  if (!d_agent_of_slot) return sfp::fail(SF_ERR_ARG, "null argument");
  *d_agent_of_slot = r->agent_of + r->first[net];
  return SF_OK;
}

int sf_route_gather(sf_route *rr, const sf_route_src *src, const sf_route_dst *dst) {
  Route *r = reinterpret_cast<Route *>(rr);
  if (!r) return sfp::fail(SF_ERR_ARG, "null route");
  if (!src || !dst) return sfp::fail(SF_ERR_ARG, "sf_route_gather: null src or dst");
  SFP_RC(sfp::check_lists(src->d_keys, src->d_vals, src->d_counts, src->d_pov, src->cap));
  SFP_RC(sfp::check_resets(src->d_reset_words, src->reset_stride, src->reset_group));
  sfp::RouteSrc s{};
  s.keys = src->d_keys, s.vals = src->d_vals, s.counts = src->d_counts, s.pov = src->d_pov, s.dense = src->d_dense;
  s.reset_mask = src->d_reset_mask, s.reset_words = src->d_reset_words, s.reset_stride = src->reset_stride;
  s.reset_group = src->reset_group > 0 ? src->reset_group : 1;
  s.cap = src->cap, s.agents = r->agents;
  const bool list_vec = src->cap % 4 == 0 && sfp::aligned16(src->d_keys) && sfp::aligned16(src->d_vals);
  sfp::RouteDsts d{};
  bool any = false;
  for (int k = 0; k < r->nets; ++k) {
    const sf_route_dst &g = dst[k];
    const bool lists = g.d_keys || g.d_vals || g.d_counts || g.d_pov;
    if (!lists && !g.d_dense && !g.d_reset_mask) continue;  // all NULL: skipped
    if (!r->count[k]) continue;                             // nobody to write
    if (!g.d_keys || !g.d_vals || !g.d_counts || !g.d_pov)
      return sfp::fail(SF_ERR_ARG, "sf_route_gather: dst[" + std::to_string(k) + "] has a null list buffer");
    if (g.cap != src->cap)
      return sfp::fail(SF_ERR_ARG, "sf_route_gather: dst[" + std::to_string(k) + "].cap differs from src->cap");
    sfp::RouteDst &o = d.net[k];
    o.keys = g.d_keys, o.vals = g.d_vals, o.counts = g.d_counts, o.pov = g.d_pov, o.dense = g.d_dense, o.reset_mask = g.d_reset_mask;
    o.vec = (list_vec && sfp::aligned16(g.d_keys) && sfp::aligned16(g.d_vals) ? 1 : 0) |
            (sfp::aligned16(src->d_pov) && sfp::aligned16(g.d_pov) ? 2 : 0) |
            (sfp::aligned16(src->d_dense) && sfp::aligned16(g.d_dense) ? 4 : 0);
    any = true;
  }
  if (!any) return SF_OK;
  SFP_HIP(hipSetDevice(r->device));
  hipLaunchKernelGGL(sfp::k_route_gather, dim3((unsigned)((r->agents + 3) / 4)), dim3(256), 0, r->stream, r->slot_of, s, d);
  SFP_HIP(hipGetLastError());
  return SF_OK;
}

int sf_route_scatter(sf_route *rr, const sf_route_rows *rows, const sf_route_rows *env) {
  Route *r = reinterpret_cast<Route *>(rr);
  if (!r) return sfp::fail(SF_ERR_ARG, "null route");
  if (!rows || !env) return sfp::fail(SF_ERR_ARG, "sf_route_scatter: null rows or env");
  const auto pack = [](const sf_route_rows &g) {
    sfp::RouteRows o{};
    o.cmd = g.d_cmd;
    o.word[0] = reinterpret_cast<uint32_t *>(g.d_action), o.word[1] = reinterpret_cast<uint32_t *>(g.d_value);
    o.word[2] = reinterpret_cast<uint32_t *>(g.d_reward), o.word[3] = reinterpret_cast<uint32_t *>(g.d_disc);
    o.word[4] = reinterpret_cast<uint32_t *>(g.d_probs);
    return o;
  };
  sfp::RouteRowsAll all{};
  for (int k = 0; k < r->nets; ++k) all.net[k] = pack(rows[k]);
  all.env = pack(*env);
  SFP_HIP(hipSetDevice(r->device));
  const long lanes = (long)r->agents * sfp::RS_LANES;
  hipLaunchKernelGGL(sfp::k_route_scatter, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, r->stream, r->slot_of, all, r->agents);
  SFP_HIP(hipGetLastError());
  return SF_OK;
}

}  // extern "C"
