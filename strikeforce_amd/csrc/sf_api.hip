// sf_api.hip — libstrikeforce_amd.so: the gfx950 runtime behind the C-ABI of include/strikeforce.h.
//
//   the thin __global__ wrappers around Core<..> (sf_core.hpp): k_reset, k_reset_sel, k_step, k_step_half <NB, HP, BM, ZL>, one wavefront
//     per arena (the instance a configuration runs: sf_types.hpp with_variant), k_step_fixed<Shape> (k_step with a listed
//     configuration's fields as constants: sf_types.hpp FixedShapes), k_agent_alive, k_done, k_ep_late, k_replay_fetch
//   k_rank (k_step's launch order) and the episode-log collection kernels k_ep_plan / k_ep_copy
//   k_snapshot<SAVE>, the copy between the state buffers and a snapshot object (sf_snapshot.hpp)
//   k_signals, vitals / delta / reward per (arena, agent) behind a step (sf_signals.hpp)
//   k_state_init / k_state_records, every arena's canonical records, counts and digest (sf_state_records.hpp)
//   k_put_init / k_put_check / k_put_write, arenas written from such records (sf_state_put.hpp)
//   k_record, k_record_plan / k_record_copy, games written out as command streams and their collection (sf_record.hpp)
//   HipRT, the runtime Env<RT> (sf_host.hpp) launches through
//   Comm, the RCCL exchange of the multi-GPU path
//   the extern "C" entry points
// The observation kernels are in sf_obs_kernels.hpp.
// There is no CPU path: without a HIP device every entry point fails with SF_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cstddef>

#include <new>
#include <utility>
#include <vector>

#include "wave_gfx950.hpp"
// clang-format off
#include "sf_core.hpp"
#include "sf_obs.hpp"
#include "sf_obs_kernels.hpp"
#include "sf_snapshot.hpp"
#include "sf_signals.hpp"
#include "sf_action_mask.hpp"
#include "sf_record.hpp"
#include "sf_host.hpp"
// clang-format on

namespace sf {

#ifdef SF_DIAG_STAMPS
__device__ uint32_t sf_diag_buffer[16 * 65536];  // diagnostic build only: [arena][phase] wave cycles of the last launch
__device__ unsigned long long sf_diag_times[4 * 65536];  // [workgroup]: s_memrealtime (100 MHz) at the wave's start, after load(), before store(), at its end
#endif

// HP (HBM_PLANE): maps whose flag plane is too large for LDS keep it in HBM (sf_core.hpp).  BM (BITMAPS): the cell
// bitmaps fit in LDS (every LDS-plane map, and HBM-plane maps up to 128 x 128).  Variants built: (HP 0, BM 1),
// (HP 1, BM 1), (HP 1, BM 0).  ZL (large pools): zombie / exit tables of more than 64 slots in LDS; built for NB = 4 only.
template <int NB, bool HP, bool BM, bool ZL>
__global__ __launch_bounds__(64) void k_reset(Params p, const uint64_t *tb, const uint64_t *serial) {
  extern __shared__ __attribute__((aligned(2048))) uint8_t lds[];  // the RNG power table comes first (W::pow_pair)
  Core<WaveGfx950, NB, HP, BM, ZL>::reset_body(lds, p, (int)blockIdx.x, tb, serial);
}

// sf_reset_arenas: k_reset for the arenas `sel` chooses (sf_core.hpp reset_sel_body), built for the variants k_reset is built
// for.  One wavefront per arena; a wavefront whose arena is not chosen ends behind four loads and its bytes of sel.selected.
template <int NB, bool HP, bool BM, bool ZL>
__global__ __launch_bounds__(64) void k_reset_sel(Params p, ResetSel sel) {
  extern __shared__ __attribute__((aligned(2048))) uint8_t lds[];  // the RNG power table comes first (W::pow_pair)
  Core<WaveGfx950, NB, HP, BM, ZL>::reset_sel_body(lds, p, (int)blockIdx.x, sel);
}

// LOG: the instance launched while the episode log is on (sf_core.hpp latch_results<LOG>); with the log off the kernel is
// the one without log code
template <int NB, bool HP, bool BM, bool ZL, bool LOG>
__global__ __launch_bounds__(64) void k_step(Params p, const uint8_t *cmds, int k) {
  extern __shared__ __attribute__((aligned(2048))) uint8_t lds[];  // the RNG power table comes first (W::pow_pair)
  const int a = p.perm ? (int)gptr(p.perm)[blockIdx.x] : (int)blockIdx.x;
#ifdef SF_DIAG_STAMPS
  if (threadIdx.x == 0) sf_diag_times[4 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
#endif
  Core<WaveGfx950, NB, HP, BM, ZL>::template step_body_t<LOG>(lds, p, a, cmds, k);
#ifdef SF_DIAG_STAMPS
  __builtin_amdgcn_s_waitcnt(0);  // (the stores have left)
  if (threadIdx.x == 0) sf_diag_times[4 * blockIdx.x + 3] = __builtin_amdgcn_s_memrealtime();
#endif
}

// The throughput kernel of one fixed shape (sf_types.hpp FixedShapes): k_step<SH::NB, false, true, false, false> with the shape's
// configuration fields as compile-time constants instead of Params reads.  Same source, same results; launched only for
// an environment whose configuration equals the shape field by field (sf_host.hpp Env::create), with the episode log off.
template <class SH>
__global__ __launch_bounds__(64) void k_step_fixed(Params p, const uint8_t *cmds, int k) {
  extern __shared__ __attribute__((aligned(2048))) uint8_t lds[];  // the RNG power table comes first (W::pow_pair)
  const int a = p.perm ? (int)gptr(p.perm)[blockIdx.x] : (int)blockIdx.x;
#ifdef SF_DIAG_STAMPS
  if (threadIdx.x == 0) sf_diag_times[4 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
#endif
  Core<WaveGfx950, SH::NB, false, true, false, SH>::template step_body_t<false>(lds, p, a, cmds, k);
#ifdef SF_DIAG_STAMPS
  __builtin_amdgcn_s_waitcnt(0);  // (the stores have left)
  if (threadIdx.x == 0) sf_diag_times[4 * blockIdx.x + 3] = __builtin_amdgcn_s_memrealtime();
#endif
}

// Launch order for k_step: arenas by population (live zombies + live humans as the last store() recorded them, SC_LOAD),
// in SNAKE order — blocks of 1024 alternately descending and ascending.  A step's cost grows with the arena's population
// and a launch ends with its slowest wavefront; the chip has 1024 SIMDs and the dispatcher hands consecutive workgroups
// to different ones, so with this order the arenas that share a SIMD are one of each load class with about equal sums
// per SIMD, the busiest arenas start first, and a busy arena's neighbours finish early and leave it the SIMD.  Measured
// on configs[2] (same-call A/B, tools/r03_balance_ab.sh): 186.7 -> 204.8 M env-steps/s, 20-step launches 172 -> 189 M;
// configs[1] (all arenas at the zombie cap: nothing to order) unchanged; keyed by the arena's measured cycles per step
// instead: +1.6 % only (an arena's time depends on its neighbours, so that key chases itself).  Other arena counts and
// the HBM-plane maps: profiles/r04_rank_sweep.txt.
// One workgroup, any number of arenas (each thread walks arenas t, t + 1024, ...); a counting sort over 65 classes, ties
// in any order: arenas are independent, the order never shows in any result.  A last block of fewer than 1024 arenas
// keeps the direction of a full one (its lightest arenas meet the SIMDs that got the busiest of the block before).
__global__ __launch_bounds__(1024) void k_rank(Params p, uint32_t *perm) {
  __shared__ uint32_t hist[72];
  const int t = (int)threadIdx.x;
  if (t < 72) hist[t] = 0u;
  __syncthreads();
  auto cls_of = [&](int a) {
    const uint32_t n = (uint32_t)gptr(p.scal)[(size_t)a * SC_WORDS + SC_LOAD];
    return 64u - (n > 64u ? 64u : n);  // class 0 = the busiest
  };
  for (int a = t; a < p.A; a += 1024) atomicAdd(&hist[cls_of(a)], 1u);
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0;
    for (int c = 0; c < 65; ++c) {
      const uint32_t n = hist[c];
      hist[c] = run;
      run += n;
    }
  }
  __syncthreads();
  for (int a = t; a < p.A; a += 1024) {
    uint32_t pos = atomicAdd(&hist[cls_of(a)], 1u);  // rank, busiest first
    if ((pos >> 10) & 1u) {  // every second block of 1024 backwards
      const uint32_t base = pos & ~1023u, len = (uint32_t)p.A - base < 1024u ? (uint32_t)p.A - base : 1024u;
      pos = base + (len - 1u - (pos - base));
    }
    gptr(perm)[pos] = (uint32_t)a;
  }
}

// sf_step_begin / sf_step_end: one half of one iteration (sf_core.hpp step<1> / step<2>)
template <int NB, bool HP, bool BM, bool ZL>
__global__ __launch_bounds__(64) void k_step_half(Params p, const uint8_t *cmds, int phase) {
  extern __shared__ __attribute__((aligned(2048))) uint8_t lds[];
  Core<WaveGfx950, NB, HP, BM, ZL>::step_half_body(lds, p, (int)blockIdx.x, cmds, phase);
}

// Human::active_agent of every commanded human (sf_agent_alive): alive and still driven through sf_step
__global__ void k_agent_alive(Params p, uint8_t *out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= p.A * p.n_agents) return;
  const int a = i / p.n_agents, g = i % p.n_agents;
  const uint32_t fl = gptr(p.hum)[((size_t)HW_FLAGS * (size_t)p.A + (size_t)a) * (size_t)p.H + (size_t)g];
  gptr(out)[i] = (uint8_t)((fl & (HF_ALIVE | HF_CTRL)) == (HF_ALIVE | HF_CTRL));
}

// check_end()'s verdict per (arena, agent) on the device (sf_done_device)
__global__ void k_done(Params p, uint8_t *out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= p.A * p.n_agents) return;
  const SF_GLOBAL int32_t *sc = gptr(p.scal) + (size_t)(i / p.n_agents) * SC_WORDS;
  gptr(out)[i] = (uint8_t)(p.auto_reset ? sc[SC_ENDED] : sc[SC_DONE]);
}

// The episode-log record of an episode that k_reset's first loop top or the second half of a split step ended (at most one
// per arena and launch), written behind that launch from the state it stored (sf_core.hpp ep_log_late): those two kernels
// carry no log code of their own.  One wavefront per arena and workgroup (WaveGfx950::lane() is threadIdx.x).
__global__ __launch_bounds__(64) void k_ep_late(Params p, int after_reset) {
  Core<WaveGfx950, 1>::ep_log_late(p, (int)blockIdx.x, after_reset != 0);
}

// sf_replay_step's two small launches around the halves of an iteration (sf_core.hpp replay_fetch): mode 0 the loop-top
// check and the line of `ind`, mode 1 the lines of the other commanded humans.  One wavefront per arena and workgroup.
__global__ __launch_bounds__(64) void k_replay_fetch(Params p, Replay r, int mode) {
  Core<WaveGfx950, 1>::replay_fetch(p, r, (int)blockIdx.x, mode);
}

// Episode log collection (sf_episodes_device): two launches, no host round trip, so that the pair can sit in a captured
// graph behind the step launches.
// k_ep_plan: one 1024-thread workgroup, thread t owns a contiguous run of arenas.  Per arena pending = episodes - cursor,
// kept = min(pending, depth) (the ring holds the newest `depth`), lost = pending - kept.  The exclusive prefix sum of
// kept over arenas (a wave64 scan of the per-thread sums, then the totals of the waves before) is the arena's first
// output record; output order is arena ascending, episode ascending.  An arena that meets max_records delivers part or
// nothing and keeps the rest pending.  Writes the plan [3][A] (first output record, records delivered, first episode
// delivered), advances each cursor by delivered + lost, and counts = [written, lost, still pending].
__global__ __launch_bounds__(1024) void k_ep_plan(const int32_t *scal, int32_t *cursor, int A, int depth, int max_records,
                                                  int32_t *plan, int32_t *counts) {
  __shared__ int wsum[16];
  __shared__ int lost_sum;
  const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  const int chunk = (A + 1023) / 1024;
  const int a0 = min(t * chunk, A), a1 = min(a0 + chunk, A);
  int kept = 0, lost = 0;
#pragma unroll 4
  for (int a = a0; a < a1; ++a) {
    const int pend = max(gptr(scal)[(size_t)a * SC_WORDS + SC_EPISODES] - gptr(cursor)[a], 0);
    kept += min(pend, depth), lost += pend - min(pend, depth);
  }
  const int x = wave_scan_incl(kept, lane);
#pragma unroll
  for (int d = 32; d; d >>= 1) lost += __shfl_xor(lost, d, 64);
  if (t == 0) lost_sum = 0;
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  if (lane == 0) atomicAdd(&lost_sum, lost);
  int off = x - kept, total = 0;
  for (int v = 0; v < 16; ++v) {
    if (v < w) off += wsum[v];
    total += wsum[v];
  }
#pragma unroll 4
  for (int a = a0; a < a1; ++a) {
    const int e = gptr(scal)[(size_t)a * SC_WORDS + SC_EPISODES], c = gptr(cursor)[a];
    const int pend = max(e - c, 0), k = min(pend, depth);
    const int give = min(max(max_records - off, 0), k);
    gptr(plan)[a] = off, gptr(plan)[A + a] = give, gptr(plan)[2 * A + a] = e - k;
    gptr(cursor)[a] = c + (pend - k) + give;
    off += k;
  }
  __syncthreads();
  if (t == 0) {
    const int written = min(total, max_records);
    gptr(counts)[0] = written, gptr(counts)[1] = lost_sum, gptr(counts)[2] = total - written;
  }
}

// k_ep_copy: one wavefront per arena (four per workgroup) copies the records the plan gives it out of the ring, the
// lanes along the record words: each pass stores 64 consecutive dwords of the dense output
__global__ __launch_bounds__(256) void k_ep_copy(const uint32_t *ring, int A, int depth, int rw, const int32_t *plan,
                                                 uint32_t *out) {
  const int a = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (a >= A) return;
  const uint32_t n = (uint32_t)gptr(plan)[A + a];
  if (n == 0u) return;
  const uint32_t off = (uint32_t)gptr(plan)[a], first = (uint32_t)gptr(plan)[2 * A + a], w = (uint32_t)rw;
  const SF_GLOBAL uint32_t *src = gptr(ring) + (size_t)a * (size_t)depth * w;
  SF_GLOBAL uint32_t *dst = gptr(out) + (size_t)off * w;
  for (uint32_t i = threadIdx.x & 63u; i < n * w; i += 64u) {
    const uint32_t r = i / w, j = i - r * w;
    dst[i] = src[(size_t)((first + r) & (uint32_t)(depth - 1)) * w + j];
  }
}


// sf_snapshot_save / sf_snapshot_load (sf_snapshot.hpp): what the copy body needs beyond the core's backend — 16 bytes per
// lane at a byte offset from a wave-uniform base, 16-bit stores, and the count of a skipped arena.  Nothing here is used
// by any other kernel.
struct SnapGfx950 : WaveGfx950 {
  using V4 = u32x4;
  static SF_DEV V4 gload16(const uint8_t *base, V byte_off, P pred) {
    return pred ? *reinterpret_cast<const SF_GLOBAL u32x4 *>(gptr(base) + byte_off) : (u32x4)(0u);
  }
  static SF_DEV void gstore16(uint8_t *base, V byte_off, V4 val, P pred) {
    if (pred) *reinterpret_cast<SF_GLOBAL u32x4 *>(gptr(base) + byte_off) = val;
  }
  static SF_DEV void gstore_u16(uint16_t *base, V idx, V val, P pred) {
    if (pred) gptr(base)[idx] = (uint16_t)val;
  }
  static SF_DEV void ucount(uint32_t *counter) {  // one vector atomic per skipped arena: the rare path
    if (lane() == 0u) (void)__hip_atomic_fetch_add(gptr(counter), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};
// One instance per direction for every configuration: the sizes travel in the piece table.  Grid (arenas, parts), one
// wavefront per workgroup (WaveGfx950::lane() is threadIdx.x).
template <bool SAVE>
__global__ __launch_bounds__(64) void k_snapshot(Snap s) {
  SnapCore<SnapGfx950, SAVE>::body(s, (int)blockIdx.x, (int)blockIdx.y);
}

// sf_signals_step (sf_signals.hpp): one lane per (arena, agent), like k_agent_alive and k_done, whose rows it reads.
__global__ __launch_bounds__(256) void k_signals(Signals s) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= s.A * s.n_agents) return;
  signals_agent(s, i);
}

// sf_action_mask_device (sf_action_mask.hpp): one wavefront per arena and workgroup, as the step kernels have it; lanes
// over (commanded human, direction) and over the slots of the entity tables.
__global__ __launch_bounds__(64) void k_action_mask(ActionMask k) { ActionMaskCore<WaveGfx950>::body(k, (int)blockIdx.x); }

// sf_state_device (sf_state_records.hpp): grid (rows, parts), one wavefront per workgroup as in k_snapshot; k_state_init
// zeroes the count and digest rows the wavefronts of one row add into, in front of it on the same stream.
__global__ __launch_bounds__(256) void k_state_init(sf_state_io io) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < io.rows) state_init_body(io, i);
}
__global__ __launch_bounds__(64) void k_state_records(StateRec s) {
  state_records_body(s, (int)blockIdx.x, (int)blockIdx.y);
}

// sf_state_put_device (sf_state_put.hpp): k_put_init zeroes the rows' verdicts, k_put_check — grid (rows, parts),
// one wavefront per workgroup — ORs the reason bits and takes counts and extents, k_put_write — grid (arenas, parts) —
// reads the verdict of the arena's row first and packs the records of rows that passed.
__global__ __launch_bounds__(256) void k_put_init(StatePut s) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < s.io.rows) put_init_body(s, i);
}
__global__ __launch_bounds__(64) void k_put_check(StatePut s) {
  state_put_check_body(s, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y);
}
__global__ __launch_bounds__(64) void k_put_write(StatePut s) {
  state_put_write_body(s, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y);
}

// sf_record_step / sf_record_flush (sf_record.hpp): one wavefront per arena and workgroup, lane g = commanded human g.
// mode 0 the loop top, mode 1 between the halves, mode 2 behind the second half, mode 3 the flush.  Modes 0, 2 and 3 are
// lane 0's alone.  Mode 1: one flag-word load, the ballot, the lane's rank in it, one byte store; the cursor by lane 0.
__global__ __launch_bounds__(64) void k_record(Record k, int mode) {
  const int a = (int)blockIdx.x, g = (int)threadIdx.x;
  if (mode == 1) {
    const bool takes = record_mid_takes(k, a, g);
    const uint64_t bal = __ballot(takes);
    if (!bal) return;
    const bool sub = takes && record_mid_store(k, a, g, bal);
    const uint64_t subs = __ballot(sub);
    if (g == 0) record_mid_finish(k, a, __popcll(bal), __popcll(subs));
    return;
  }
  if (g != 0) return;
  if (mode == 0) record_top(k, a);
  else if (mode == 2) record_end(k, a);
  else record_flush(k, a);
}

// sf_record_collect_device, two launches as the episode log's collection (k_ep_plan / k_ep_copy).
// k_record_plan: one 1024-thread workgroup, thread t owns a contiguous run of arenas.  The exclusive prefix sums of closed
// games and closed bytes over arenas (per-thread sums, a scan of the 1024 sums in LDS) say for every game what lies in
// front of it in the output order; record_plan_arena decides from that alone what its arena delivers.
__global__ __launch_bounds__(1024) void k_record_plan(Record k, long long max_games, long long max_bytes, long long *counts) {
  __shared__ long long sg[1024], sb[1024];
  __shared__ unsigned long long tot[4];
  const int t = (int)threadIdx.x;
  const int chunk = (k.A + 1023) / 1024;
  const int a0 = min(t * chunk, k.A), a1 = min(a0 + chunk, k.A);
  int64_t g = 0, b = 0;
  for (int a = a0; a < a1; ++a) {
    int64_t ga, ba;
    record_arena_totals(k, a, ga, ba);
    g += ga, b += ba;
  }
  sg[t] = g, sb[t] = b;
  if (t < 4) tot[t] = 0ull;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const long long ug = t >= d ? sg[t - d] : 0, ub = t >= d ? sb[t - d] : 0;
    __syncthreads();
    sg[t] += ug, sb[t] += ub;
    __syncthreads();
  }
  int64_t gpre = sg[t] - g, bpre = sb[t] - b;
  const long long all_g = sg[1023], all_b = sb[1023];
  int64_t tg = 0, tb = 0, lost = 0, subst = 0;
  for (int a = a0; a < a1; ++a) {
    int64_t ga, ba;
    record_arena_totals(k, a, ga, ba);
    record_plan_arena(k, a, gpre, bpre, max_games, max_bytes, tg, tb, lost, subst);
    gpre += ga, bpre += ba;
  }
  if (tg) atomicAdd(&tot[0], (unsigned long long)tg);
  if (tb) atomicAdd(&tot[1], (unsigned long long)tb);
  if (lost) atomicAdd(&tot[2], (unsigned long long)lost);
  if (subst) atomicAdd(&tot[3], (unsigned long long)subst);
  __syncthreads();
  if (t == 0) {
    SF_GLOBAL long long *c = gptr(counts);
    c[0] = (long long)tot[0], c[1] = (long long)tot[1], c[2] = all_g - (long long)tot[0], c[3] = all_b - (long long)tot[1];
    c[4] = (long long)tot[2], c[5] = (long long)tot[3];
  }
}

// k_record_copy: one wavefront per arena (four per workgroup).  Each pass stores 64 consecutive dwords of the dense game
// list, then 64 consecutive bytes of the dense streams; then what stays moves to the front of the region and the index.
__global__ __launch_bounds__(256) void k_record_copy(Record k, uint8_t *d_bytes, int32_t *d_games) {
  const int a = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
  if (a >= k.A) return;
  const RecordCopy c = record_copy_load(k, a);
  if (c.ntake == 0) return;
  for (int32_t i = lane; i < c.ntake * RG_WORDS; i += 64) record_copy_game_word(k, c, a, i, d_games);
  for (int32_t i = lane; i < c.tbytes; i += 64) record_copy_byte(k, c, a, i, d_bytes);
  const int32_t rem_w = (c.ngames - c.ntake) * RG_WORDS, rem_b = c.used - c.tbytes;
  for (int32_t i = lane; i < rem_w; i += 64) {
    const int32_t v = record_compact_word_load(k, c, a, i);
    record_compact_word_store(k, a, i, v);
  }
  if (c.tbytes)
    for (int32_t i = lane; i < rem_b; i += 64) {
      const uint8_t v = record_compact_byte_load(k, c, a, i);
      record_compact_byte_store(k, a, i, v);
    }
  if (lane == 0) record_copy_finish(k, c, a);
}

#define SF_HIP(call)                                                                       \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess) return fail(SF_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

struct HipRT {
  hipStream_t stream = nullptr;
  int device = 0;
  size_t lds_limit = 64 * 1024;
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;  // one pair per timed step launch
  size_t used_events = 0;

  int init(int dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
      return fail(SF_ERR_DEVICE, "no HIP device: strikeforce_amd has no CPU path");
    if (dev < 0 || dev >= n) return fail(SF_ERR_DEVICE, "device ordinal out of range");
    device = dev;
    SF_HIP(hipSetDevice(dev));
    hipDeviceProp_t prop;
    SF_HIP(hipGetDeviceProperties(&prop, dev));
    lds_limit = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : prop.sharedMemPerBlock;
    return SF_OK;
  }
  void shutdown() {
    for (auto &ev : events) (void)hipEventDestroy(ev.first), (void)hipEventDestroy(ev.second);
    events.clear();
  }
  size_t max_lds() const { return lds_limit; }
  void *alloc(size_t n) {
    void *p = nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    if (hipMalloc(&p, n ? n : 1) != hipSuccess) return nullptr;
    return p;
  }
  void free(void *p) { (void)hipFree(p); }
  void h2d(void *d, const void *s, size_t n) { note(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, stream)); }
  void d2h(void *d, const void *s, size_t n) { note(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, stream)); }
  void d2d(void *d, const void *s, size_t n) { note(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, stream)); }
  void zero(void *d, size_t n) { note(hipMemsetAsync(d, 0, n, stream)); }
  // copies report through sync(): the first failure is kept and returned there
  hipError_t pending = hipSuccess;
  void note(hipError_t e) {
    if (e != hipSuccess && pending == hipSuccess) pending = e;
  }
  int sync() {
    if (pending != hipSuccess) {
      hipError_t e = pending;
      pending = hipSuccess;
      return fail(SF_ERR_DEVICE, std::string("async copy: ") + hipGetErrorString(e));
    }
    SF_HIP(hipStreamSynchronize(stream));
    return SF_OK;
  }

  int launch_reset(const Params &p, int NB, const uint64_t *tb, const uint64_t *serial) {
    SF_HIP(hipSetDevice(device));
    return launch_arenas(p, NB, [](auto v) { return &k_reset<v.NB, v.HP, v.BM, v.ZL>; }, tb, serial);
  }
  // `bytes` bytes at q: device memory of this runtime's device, aligned, wholly inside its allocation (as
  // sf_policy_load_weights checks its sources).  A host pointer is answered here and never reaches a kernel.
  int check_device_range(const void *q, size_t bytes, size_t align, const char *name, const char *who = "sf_reset_arenas") const {
    const std::string n = std::string(who) + ": " + name;
    if (reinterpret_cast<uintptr_t>(q) & (align - 1)) return fail(SF_ERR_ARG, n + " is not " + std::to_string(align) + "-byte aligned");
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, q) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != device) {
      (void)hipGetLastError();  // (a host pointer is an error of the query: it is answered here, not left behind)
      return fail(SF_ERR_ARG, n + " is not device memory of the environment's device");
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(q)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(SF_ERR_ARG, n + ": its allocation is unknown to the runtime");
    }
    const uintptr_t lo = reinterpret_cast<uintptr_t>(base), addr = reinterpret_cast<uintptr_t>(q);
    if (addr < lo || addr - lo > size || bytes > size - (addr - lo)) return fail(SF_ERR_ARG, n + " reaches past the end of its allocation");
    return SF_OK;
  }
  // one launch, the struct in the kernel arguments; nothing is allocated, copied or waited for
  int launch_reset_sel(const Params &p, int NB, const ResetSel &sel) {
    SF_HIP(hipSetDevice(device));
    const size_t A = (size_t)p.A;
    int rc;
    if (sel.mask && (rc = check_device_range(sel.mask, (A - 1) * (size_t)sel.mask_stride + 1, 1, "d_mask"))) return rc;
    if (sel.tb && (rc = check_device_range(sel.tb, A * sizeof(uint64_t), 8, "d_tb"))) return rc;
    if (sel.serial && (rc = check_device_range(sel.serial, A * sizeof(uint64_t), 8, "d_serial"))) return rc;
    if (sel.selected && (rc = check_device_range(sel.selected, A * (size_t)p.n_agents, 1, "d_selected"))) return rc;
    return launch_arenas(p, NB, [](auto v) { return &k_reset_sel<v.NB, v.HP, v.BM, v.ZL>; }, sel);
  }
  // sf_snapshot_save / sf_snapshot_load: one launch, the piece table in the kernel arguments
  int launch_snapshot(const Snap &k, int parts, bool save) {
    SF_HIP(hipSetDevice(device));
    if (int rc = check_device_range(k.slot_of_arena, (size_t)k.A * sizeof(int32_t), 4, "d_slot_of_arena", save ? "sf_snapshot_save" : "sf_snapshot_load"))
      return rc;
    const dim3 grid((unsigned)k.A, (unsigned)parts);
    return save ? launch(k_snapshot<true>, grid, dim3(64), 0, k) : launch(k_snapshot<false>, grid, dim3(64), 0, k);
  }
  // sf_signals_step: one launch; the optional pointers are checked as sf_reset_arenas checks its own
  int launch_signals(const Signals &k) {
    SF_HIP(hipSetDevice(device));
    const size_t n = (size_t)k.A * (size_t)k.n_agents;
    int rc;
    if (k.vitals && (rc = check_device_range(k.vitals, n * SF_VITALS_WORDS * sizeof(int32_t), 4, "d_vitals", "sf_signals_step"))) return rc;
    if (k.delta && (rc = check_device_range(k.delta, n * SF_DELTA_WORDS * sizeof(int32_t), 4, "d_delta", "sf_signals_step"))) return rc;
    if (k.reward && (rc = check_device_range(k.reward, n * sizeof(float), 4, "d_reward", "sf_signals_step"))) return rc;
    if (k.rebase && (rc = check_device_range(k.rebase, n, 1, "d_rebase", "sf_signals_step"))) return rc;
    return launch(k_signals, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, k);
  }
  // sf_action_mask_device: one launch; the outputs are checked as sf_reset_arenas checks its own
  int launch_action_mask(const ActionMask &k) {
    SF_HIP(hipSetDevice(device));
    const size_t bytes = (size_t)k.A * (size_t)k.n_agents * sizeof(uint32_t);
    int rc;
    if (k.commands && (rc = check_device_range(k.commands, bytes, 4, "d_commands", "sf_action_mask_device"))) return rc;
    if (k.actions && (rc = check_device_range(k.actions, bytes, 4, "d_actions", "sf_action_mask_device"))) return rc;
    return launch(k_action_mask, dim3((unsigned)k.A), dim3(64), 0, k);
  }
  // sf_state_device: the id list and every requested output checked as sf_signals_step checks its own, then k_state_init
  // (only with d_counts or d_digest) and k_state_records.  bytes: what each of the ten outputs must hold (Env::state_fill)
  int launch_state_records(const StateRec &k, const int64_t *bytes) {
    SF_HIP(hipSetDevice(device));
    const sf_state_io &io = k.io;
    const char *who = "sf_state_device";
    int rc;
    if (io.d_arena_ids && (rc = check_device_range(io.d_arena_ids, (size_t)io.rows * sizeof(int32_t), 4, "d_arena_ids", who))) return rc;
    const struct { const void *q; size_t align; const char *name; } outs[10] = {
        {io.d_hdr, 8, "d_hdr"}, {io.d_humans, 4, "d_humans"}, {io.d_zombies, 4, "d_zombies"}, {io.d_bullets, 4, "d_bullets"},
        {io.d_portals, 4, "d_portals"}, {io.d_cell_flags, 1, "d_cell_flags"}, {io.d_cell_dmg, 4, "d_cell_dmg"},
        {io.d_cell_portal, 4, "d_cell_portal"}, {io.d_counts, 4, "d_counts"}, {io.d_digest, 8, "d_digest"}};
    bool any = false;
    for (int j = 0; j < 10; ++j) {
      if (!outs[j].q) continue;
      any = true;
      if ((rc = check_device_range(outs[j].q, (size_t)bytes[j], outs[j].align, outs[j].name, who))) return rc;
    }
    if (!any) return SF_OK;
    if (io.d_counts || io.d_digest)
      if ((rc = launch(k_state_init, dim3((unsigned)((io.rows + 255) / 256)), dim3(256), 0, io))) return rc;
    return launch(k_state_records, dim3((unsigned)io.rows, (unsigned)k.parts), dim3(64), 0, k);
  }
  // sf_state_put_device: the row map, every part given and the two outputs checked as sf_state_device checks its own.
  // bytes: what each of the eleven buffers must hold (Env::put_fill).  Nothing is launched here
  int check_state_put(const StatePut &k, const int64_t *bytes) {
    SF_HIP(hipSetDevice(device));
    const sf_state_put_io &io = k.io;
    const struct { const void *q; size_t align; const char *name; } bufs[11] = {
        {io.d_row_of_arena, 4, "d_row_of_arena"}, {io.d_hdr, 8, "d_hdr"}, {io.d_humans, 4, "d_humans"}, {io.d_zombies, 4, "d_zombies"},
        {io.d_bullets, 4, "d_bullets"}, {io.d_portals, 4, "d_portals"}, {io.d_cell_flags, 1, "d_cell_flags"}, {io.d_cell_dmg, 4, "d_cell_dmg"},
        {io.d_cell_portal, 4, "d_cell_portal"}, {io.d_status, 4, "d_status"}, {io.d_selected, 1, "d_selected"}};
    for (int j = 0; j < 11; ++j) {
      if (!bufs[j].q || bytes[j] == 0) continue;  // (a table cut to 0 slots is never read)
      if (int rc = check_device_range(bufs[j].q, (size_t)bytes[j], bufs[j].align, bufs[j].name, "sf_state_put_device")) return rc;
    }
    return SF_OK;
  }
  // the init, the check over the rows, the write over the arenas
  int launch_state_put(const StatePut &k, const int64_t *) {
    SF_HIP(hipSetDevice(device));
    const int units = put_units(k).total();
    int rc;
    if ((rc = launch(k_put_init, dim3((unsigned)((k.io.rows + 255) / 256)), dim3(256), 0, k))) return rc;
    if ((rc = launch(k_put_check, dim3((unsigned)k.io.rows, (unsigned)state_parts_for(units, k.io.rows)), dim3(64), 0, k))) return rc;
    return launch(k_put_write, dim3((unsigned)k.A, (unsigned)state_parts_for(units, k.A)), dim3(64), 0, k);
  }
  // sf_record_step / sf_record_flush: one of the record launches (k_record's mode)
  int launch_record(const Record &k, int mode) {
    SF_HIP(hipSetDevice(device));
    return launch(k_record, dim3((unsigned)k.A), dim3(64), 0, k, mode);
  }
  // sf_record_collect_device: the outputs checked as sf_signals_step checks its own, then plan and copy
  int launch_record_collect(const Record &k, uint8_t *d_bytes, int64_t max_bytes, int32_t *d_games, int32_t max_games, int64_t *d_counts) {
    SF_HIP(hipSetDevice(device));
    const char *who = "sf_record_collect_device";
    int rc;
    if ((rc = check_device_range(d_bytes, (size_t)max_bytes, 1, "d_bytes", who)) ||
        (rc = check_device_range(d_games, (size_t)max_games * SF_RECORD_GAME_WORDS * sizeof(int32_t), 4, "d_games", who)) ||
        (rc = check_device_range(d_counts, SF_RECORD_COUNT_WORDS * sizeof(int64_t), 8, "d_counts", who)))
      return rc;
    if ((rc = launch(k_record_plan, dim3(1), dim3(1024), 0, k, (long long)max_games, (long long)max_bytes, reinterpret_cast<long long *>(d_counts))))
      return rc;
    return launch(k_record_copy, dim3((unsigned)((k.A + 3) / 4)), dim3(256), 0, k, d_bytes, d_games);
  }
  bool can_rank() const { return true; }
  // k_rank runs right in front of the k_step launch it orders, inside that launch's pair of timing events: what
  // sf_kernel_time reports (and bench.py's roofline prices) includes it
  uint32_t *rank_pending = nullptr;
  int launch_rank(const Params &, uint32_t *perm) {
    rank_pending = perm;
    return SF_OK;
  }
  // set by the host side while the episode log is on (sf_host.hpp Env::episode_log): k_step's LOG instance is launched
  bool ep_log_on = false;
  // the fixed shape of the environment's configuration (index in sf_types.hpp FixedShapes; Env::create), -1: none, or
  // SF_STEP_GENERIC=1.  last_step_shape: what the last step launch ran (sf_step_kernel), -1 = a generic k_step instance
  int fixed_shape = -1, last_step_shape = -1;
  int launch_step(const Params &p, int NB, const uint8_t *cmds, int k) {
    SF_HIP(hipSetDevice(device));
    std::pair<hipEvent_t, hipEvent_t> *ev = nullptr;
    if (timing) {
      if (used_events == events.size()) {
        hipEvent_t a, b;
        SF_HIP(hipEventCreate(&a));
        SF_HIP(hipEventCreate(&b));
        events.emplace_back(a, b);
      }
      ev = &events[used_events++];
      SF_HIP(hipEventRecord(ev->first, stream));
    }
    if (rank_pending) {
      uint32_t *perm = rank_pending;
      rank_pending = nullptr;
      if (int rc = launch(k_rank, dim3(1), dim3(1024), 0, p, perm)) return rc;
    }
    const bool log = ep_log_on;
    last_step_shape = log ? -1 : fixed_shape;
    if (last_step_shape >= 0) {
      const size_t lds = lds_bytes_for(p.cells_pad, p.lds_tab, p.Z, p.P);  // (an LDS-plane shape: at most 12 KiB of plane, below the 48 KiB default)
      if (int rc = with_fixed_shape(last_step_shape, FixedShapes{}, SF_ERR_STATE, [&](auto sh) {
            return launch(&k_step_fixed<decltype(sh)>, dim3((unsigned)p.A), dim3(64), lds, p, cmds, k);
          }))
        return rc;
    } else {
      auto kernel_of = [log](auto v) { return log ? &k_step<v.NB, v.HP, v.BM, v.ZL, true> : &k_step<v.NB, v.HP, v.BM, v.ZL, false>; };
      if (int rc = launch_arenas(p, NB, kernel_of, cmds, k)) return rc;
    }
    if (ev) SF_HIP(hipEventRecord(ev->second, stream));
    return SF_OK;
  }
  int launch_step_half(const Params &p, int NB, const uint8_t *cmds, int phase) {
    SF_HIP(hipSetDevice(device));
    return launch_arenas(p, NB, [](auto v) { return &k_step_half<v.NB, v.HP, v.BM, v.ZL>; }, cmds, phase);
  }
  int launch_agent_alive(const Params &p, uint8_t *d_out) {
    SF_HIP(hipSetDevice(device));
    return launch(k_agent_alive, dim3((unsigned)((p.A * p.n_agents + 255) / 256)), dim3(256), 0, p, d_out);
  }
  int launch_done(const Params &p, uint8_t *d_out) {
    SF_HIP(hipSetDevice(device));
    return launch(k_done, dim3((unsigned)((p.A * p.n_agents + 255) / 256)), dim3(256), 0, p, d_out);
  }
  int launch_ep_late(const Params &p, bool after_reset) {
    SF_HIP(hipSetDevice(device));
    return launch(k_ep_late, dim3((unsigned)p.A), dim3(64), 0, p, after_reset ? 1 : 0);
  }
  int launch_replay_fetch(const Params &p, const Replay &r, int mode) {
    SF_HIP(hipSetDevice(device));
    return launch(k_replay_fetch, dim3((unsigned)p.A), dim3(64), 0, p, r, mode);
  }
  int launch_episodes(const Params &p, const uint32_t *ring, int depth, int32_t *cursor, int32_t *plan, int32_t *out,
                      int max_records, int32_t *counts) {
    SF_HIP(hipSetDevice(device));
    if (int rc = launch(k_ep_plan, dim3(1), dim3(1024), 0, p.scal, cursor, p.A, depth, max_records, plan, counts)) return rc;
    return launch(k_ep_copy, dim3((unsigned)((p.A + 3) / 4)), dim3(256), 0, ring, p.A, depth, ep_record_words(p.n_agents), plan,
                  reinterpret_cast<uint32_t *>(out));
  }
  int launch_observe(const Params &p, int, float *out, uint32_t *nzprev, int mode) {
    SF_HIP(hipSetDevice(device));
    return launch(k_observe, dim3((unsigned)(p.A * p.n_agents)), dim3(OBS_THREADS), obs_lds_bytes(p), p, out, nzprev, mode, ObsSparse{});
  }
  int launch_observe_sparse(const Params &p, uint32_t *keys, float *vals, uint32_t *counts, float *pov, int cap) {
    SF_HIP(hipSetDevice(device));
    static const bool old_form = getenv("SF_OBS_LIST_BLOCK") != nullptr;  // (A/B: the list as mode 3 of the dense kernel, round 3's form)
    const dim3 grid((unsigned)(p.A * p.n_agents));
    const ObsSparse sp{keys, vals, counts, pov, cap};
    if (!old_form) return launch(k_observe_list, grid, dim3(64), 0, p, sp);
    return launch(k_observe, grid, dim3(OBS_THREADS), obs_lds_bytes(p), p, (float *)nullptr, (uint32_t *)nullptr, 3, sp);
  }
  int launch_observe_overflow(const Params &p, const uint32_t *counts, int cap, float *dense, float *pov) {
    SF_HIP(hipSetDevice(device));
    const int n = p.A * p.n_agents;
    return launch(k_observe_redo, dim3((unsigned)(n < 512 ? n : 512)), dim3(OBS_THREADS), obs_lds_bytes(p), p, dense,
                  ObsSparse{nullptr, nullptr, const_cast<uint32_t *>(counts), pov, cap});
  }

  int kernel_time(int enable, float *ms, int *launches) {
    SF_HIP(hipStreamSynchronize(stream));
    float total = 0.f;
    for (size_t i = 0; i < used_events; ++i) {
      float t = 0.f;
      SF_HIP(hipEventElapsedTime(&t, events[i].first, events[i].second));
      total += t;
    }
    if (ms) *ms = total;
    if (launches) *launches = (int)used_events;
    used_events = 0;
    timing = enable != 0;
    return SF_OK;
  }

 private:
  // The per-arena kernels (k_reset, k_step, k_step_half): one wavefront per arena, the instance with_variant picks
  // (kernel_of: KernelVariant -> that instance's address), the arena's LDS as the dynamic allocation
  template <class KernelOf, class... Args>
  int launch_arenas(const Params &p, int NB, KernelOf kernel_of, const Args &...args) {
    const size_t lds = lds_bytes_for(p.cells_pad, p.lds_tab, p.Z, p.P);
    return with_variant(p, NB, [&](auto v) {
      auto kernel = kernel_of(v);
      if (lds > 48 * 1024)
        SF_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      return launch(kernel, dim3((unsigned)p.A), dim3(64), lds, p, args...);
    });
  }
  template <class K, class... Args>
  int launch(K kernel, dim3 grid, dim3 block, size_t lds, const Args &...args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    SF_HIP(hipGetLastError());
    return SF_OK;
  }
};

// The one exchange step of the multi-GPU path: an RCCL all-gather of the end-of-episode result
// records, issued on a stream of the library's own so that it runs beside the next launch.  RCCL is loaded on first
// use (dlopen; single-GPU users never map it) and the communicator is the library's own: the caller only carries
// the 128-byte unique id from rank 0 to the other ranks (torch.distributed, MPI, a file: anything).
struct ncclUniqueIdBytes {  // ncclUniqueId of rccl.h: 128 opaque bytes, passed by value
  char internal[SF_COMM_ID_BYTES];
};
// One double-buffered snapshot + gather (Comm::gather): two staging buffers of `words` dwords used in turn, each with the
// event that says its snapshot is complete (ready) and the one that says the gather that read it has finished (done)
struct GatherChannel {
  hipEvent_t ready[2] = {nullptr, nullptr}, done[2] = {nullptr, nullptr};
  int32_t *staging[2] = {nullptr, nullptr};
  size_t words = 0;
  bool used[2] = {false, false};
  unsigned issued = 0;

  void release() {
    for (int j = 0; j < 2; ++j) {
      if (ready[j]) (void)hipEventDestroy(ready[j]), ready[j] = nullptr;
      if (done[j]) (void)hipEventDestroy(done[j]), done[j] = nullptr;
      if (staging[j]) (void)hipFree(staging[j]), staging[j] = nullptr;
      used[j] = false;
    }
    words = 0, issued = 0;
  }
  // staging for snapshots of n dwords; a channel of another size is rebuilt once the gathers still reading its old
  // snapshots on `side` are through.  `who`: the entry point, for the message of a failed allocation (nothing is left)
  int prepare(size_t n, hipStream_t side, const char *who) {
    if (words == n) return SF_OK;
    if (words) SF_HIP(hipStreamSynchronize(side));
    release();
    bool ok = true;
    for (int j = 0; j < 2 && ok; ++j)
      ok = hipEventCreateWithFlags(&ready[j], hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(&done[j], hipEventDisableTiming) == hipSuccess &&
           hipMalloc((void **)&staging[j], n * sizeof(int32_t)) == hipSuccess;
    if (!ok) {
      release();
      return fail(SF_ERR_DEVICE, std::string(who) + ": event / staging allocation failed");
    }
    words = n;
    return SF_OK;
  }
};
struct Comm {
  typedef int (*get_id_t)(void *);
  typedef int (*init_rank_t)(void **, int, ncclUniqueIdBytes, int);
  typedef int (*all_gather_t)(const void *, void *, size_t, int, void *, hipStream_t);
  typedef int (*destroy_t)(void *);
  typedef const char *(*err_t)(int);
  typedef int (*count_t)(void *, int *);
  count_t count_fn = nullptr;
  void *dl = nullptr;
  get_id_t get_id = nullptr;
  init_rank_t init_rank = nullptr;
  all_gather_t all_gather = nullptr;
  destroy_t destroy_fn = nullptr;
  err_t err = nullptr;
  void *comm = nullptr;
  int world = 0, rank = 0;
  hipStream_t side = nullptr;
  // the result records (sf_results_allgather; sized once, by sf_comm_init) and the raw episode-log ring
  // (sf_episodes_allgather; sized on each call: sf_episode_log may have changed the ring's depth since the last gather)
  GatherChannel results, episodes;

  int load() {
    if (dl) return SF_OK;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char *n : names)
      if ((dl = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (!dl) return fail(SF_ERR_DEVICE, std::string("RCCL not found: ") + dlerror());
    get_id = (get_id_t)dlsym(dl, "ncclGetUniqueId");
    init_rank = (init_rank_t)dlsym(dl, "ncclCommInitRank");
    all_gather = (all_gather_t)dlsym(dl, "ncclAllGather");
    destroy_fn = (destroy_t)dlsym(dl, "ncclCommDestroy");
    err = (err_t)dlsym(dl, "ncclGetErrorString");
    count_fn = (count_t)dlsym(dl, "ncclCommCount");
    if (!get_id || !init_rank || !all_gather || !destroy_fn || !err) return fail(SF_ERR_DEVICE, "RCCL lacks a symbol");
    return SF_OK;
  }
  int nccl(int rc, const char *what) { return rc == 0 ? SF_OK : fail(SF_ERR_DEVICE, std::string(what) + ": " + err(rc)); }
  void shutdown() {
    if (comm) (void)destroy_fn(comm), comm = nullptr;
    for (GatherChannel *ch : {&results, &episodes}) ch->release();
    if (side) (void)hipStreamDestroy(side), side = nullptr;
  }
  // `count` dwords at src are snapshotted on the simulation stream `sim` (later launches write new ones), the gather of the
  // snapshot into d_out runs on the side stream; a snapshot buffer is reused only after the gather that read it has finished
  int gather(GatherChannel &ch, const int32_t *src, size_t count, int32_t *d_out, hipStream_t sim) {
    const int j = (int)(ch.issued++ & 1u);
    if (ch.used[j]) SF_HIP(hipStreamWaitEvent(sim, ch.done[j], 0));
    SF_HIP(hipMemcpyAsync(ch.staging[j], src, count * sizeof(int32_t), hipMemcpyDeviceToDevice, sim));
    SF_HIP(hipEventRecord(ch.ready[j], sim));
    SF_HIP(hipStreamWaitEvent(side, ch.ready[j], 0));
    int rc = nccl(all_gather(ch.staging[j], d_out, count, 2 /* ncclInt32 */, comm, side), "ncclAllGather");
    if (rc) return rc;
    SF_HIP(hipEventRecord(ch.done[j], side));
    ch.used[j] = true;
    return SF_OK;
  }
};

}  // namespace sf

struct sf_env {
  sf::Env<sf::HipRT> e;
  sf::Comm comm;
};
struct sf_snapshot {
  sf::Env<sf::HipRT>::Snapshot *s;
};
struct sf_signals {
  sf::Env<sf::HipRT>::SignalsObj *s;
};
struct sf_recorder {
  sf::Env<sf::HipRT>::Recorder *r;
};

using sf::fail;  // SF_HIP in the entry points below

extern "C" {

int sf_abi_version(void) { return SF_ABI_VERSION; }
const char *sf_last_error(void) { return sf::last_error().c_str(); }
void sf_config_defaults(sf_config *cfg) {
  if (cfg) sf::config_defaults(cfg);
}

int sf_create(const sf_config *cfg, sf_env **out) {
  if (!out) return sf::fail(SF_ERR_ARG, "null output handle");
  *out = nullptr;
  sf_env *env = new (std::nothrow) sf_env();
  if (!env) return sf::fail(SF_ERR_MEMORY, "host allocation failed");
  int rc = env->e.create(cfg);
  if (rc != SF_OK) {
    env->e.destroy();
    delete env;
    return rc;
  }
  *out = env;
  return SF_OK;
}
int sf_destroy(sf_env *env) {
  if (!env) return SF_OK;
  env->comm.shutdown();
  env->e.destroy();
  delete env;
  return SF_OK;
}
#define SF_ENV(env) \
  if (!(env)) return sf::fail(SF_ERR_ARG, "null environment")

int sf_reset(sf_env *env, const uint64_t *tb, const uint64_t *serial) {
  SF_ENV(env);
  return env->e.reset(tb, serial);
}
int sf_reset_arenas(sf_env *env, const sf_reset_sel *sel) {
  SF_ENV(env);
  return env->e.reset_arenas(sel);
}
int sf_snapshot_create(sf_env *env, int32_t slots, sf_snapshot **out) {
  if (!out) return sf::fail(SF_ERR_ARG, "sf_snapshot_create: null output handle");
  *out = nullptr;
  SF_ENV(env);
  sf_snapshot *h = new (std::nothrow) sf_snapshot{nullptr};
  if (!h) return sf::fail(SF_ERR_MEMORY, "host allocation failed");
  if (int rc = env->e.snapshot_create(slots, &h->s)) {
    delete h;
    return rc;
  }
  *out = h;
  return SF_OK;
}
int sf_snapshot_destroy(sf_snapshot *s) {
  if (!s) return SF_OK;
  const int rc = s->s->owner->snapshot_destroy(s->s);
  delete s;
  return rc;
}
int sf_snapshot_slot_bytes(sf_env *env, int64_t *device_bytes, int64_t *blob_bytes) {
  SF_ENV(env);
  return env->e.snapshot_slot_bytes(device_bytes, blob_bytes);
}
int sf_snapshot_save(sf_env *env, sf_snapshot *s, const int32_t *d_slot_of_arena) {
  SF_ENV(env);
  return env->e.snapshot_copy(s ? s->s : nullptr, d_slot_of_arena, true);
}
int sf_snapshot_load(sf_env *env, sf_snapshot *s, const int32_t *d_slot_of_arena) {
  SF_ENV(env);
  return env->e.snapshot_copy(s ? s->s : nullptr, d_slot_of_arena, false);
}
#define SF_SNAP(s) \
  if (!(s)) return sf::fail(SF_ERR_ARG, "null snapshot")
int sf_snapshot_status(sf_snapshot *s, int32_t out_host[4]) {
  SF_SNAP(s);
  return s->s->owner->snapshot_status(s->s, out_host);
}
int sf_snapshot_export(sf_snapshot *s, int32_t slot, void *blob_host, int64_t bytes) {
  SF_SNAP(s);
  return s->s->owner->snapshot_export(s->s, slot, blob_host, bytes);
}
int sf_snapshot_import(sf_snapshot *s, int32_t slot, const void *blob_host, int64_t bytes) {
  SF_SNAP(s);
  return s->s->owner->snapshot_import(s->s, slot, blob_host, bytes);
}
int sf_signals_create(sf_env *env, sf_signals **out) {
  if (!out) return sf::fail(SF_ERR_ARG, "sf_signals_create: null output handle");
  *out = nullptr;
  SF_ENV(env);
  sf_signals *h = new (std::nothrow) sf_signals{nullptr};
  if (!h) return sf::fail(SF_ERR_MEMORY, "host allocation failed");
  if (int rc = env->e.signals_create(&h->s)) {
    delete h;
    return rc;
  }
  *out = h;
  return SF_OK;
}
int sf_signals_destroy(sf_signals *s) {
  if (!s) return SF_OK;
  const int rc = s->s->owner->signals_destroy(s->s);
  delete s;
  return rc;
}
int sf_signals_step(sf_env *env, sf_signals *s, const sf_signals_io *io) {
  SF_ENV(env);
  return env->e.signals_step(s ? s->s : nullptr, io);
}
int sf_signals_status(sf_signals *s, int64_t out_host[4]) {
  if (!s) return sf::fail(SF_ERR_ARG, "null signals object");
  return s->s->owner->signals_status(s->s, out_host);
}
int sf_action_mask_device(sf_env *env, const sf_action_mask_io *io) {
  SF_ENV(env);
  return env->e.action_mask_device(io);
}
int sf_action_mask(sf_env *env, uint32_t *out_host) {
  SF_ENV(env);
  return env->e.action_mask_host(out_host);
}
int sf_record_create(sf_env *env, int64_t bytes_per_arena, int32_t games_per_arena, sf_recorder **out) {
  if (!out) return sf::fail(SF_ERR_ARG, "sf_record_create: null output handle");
  *out = nullptr;
  SF_ENV(env);
  sf_recorder *h = new (std::nothrow) sf_recorder{nullptr};
  if (!h) return sf::fail(SF_ERR_MEMORY, "host allocation failed");
  if (int rc = env->e.record_create(bytes_per_arena, games_per_arena, &h->r)) {
    delete h;
    return rc;
  }
  *out = h;
  return SF_OK;
}
int sf_record_destroy(sf_recorder *r) {
  if (!r) return SF_OK;
  const int rc = r->r->owner->record_destroy(r->r);
  delete r;
  return rc;
}
int sf_record_step(sf_env *env, sf_recorder *r, const uint8_t *d_cmd) {
  SF_ENV(env);
  return env->e.record_step(r ? r->r : nullptr, d_cmd);
}
int sf_record_flush(sf_env *env, sf_recorder *r) {
  SF_ENV(env);
  return env->e.record_flush(r ? r->r : nullptr);
}
int sf_record_collect_device(sf_recorder *r, uint8_t *d_bytes, int64_t max_bytes, int32_t *d_games, int32_t max_games,
                             int64_t *d_counts) {
  if (!r) return sf::fail(SF_ERR_ARG, "null recorder");
  return r->r->owner->record_collect_device(r->r, d_bytes, max_bytes, d_games, max_games, d_counts);
}
int sf_record_collect(sf_recorder *r, uint8_t *bytes_host, int64_t max_bytes, int32_t *games_host, int32_t max_games,
                      int64_t *counts_host) {
  if (!r) return sf::fail(SF_ERR_ARG, "null recorder");
  return r->r->owner->record_collect_host(r->r, bytes_host, max_bytes, games_host, max_games, counts_host);
}
int sf_step(sf_env *env, const uint8_t *cmd) {
  SF_ENV(env);
  return env->e.step_host(cmd);
}
int sf_step_device(sf_env *env, const uint8_t *d_cmd, int32_t k) {
  SF_ENV(env);
  return env->e.step_device(d_cmd, k);
}
int sf_observe(sf_env *env, float *out_host) {
  SF_ENV(env);
  return env->e.observe_host(out_host);
}
int sf_observe_device_delta(sf_env *env, float *d_out) {
  SF_ENV(env);
  return env->e.observe_device_delta(d_out);
}
int sf_observe_device(sf_env *env, float *d_out) {
  SF_ENV(env);
  return env->e.observe_device(d_out);
}
int sf_observe_overflow_device(sf_env *env, const uint32_t *d_counts, int32_t cap, float *d_dense, float *d_pov) {
  SF_ENV(env);
  return env->e.observe_overflow_device(d_counts, cap, d_dense, d_pov);
}
int sf_observe_sparse_device(sf_env *env, uint32_t *d_keys, float *d_vals, uint32_t *d_counts, float *d_pov, int32_t cap) {
  SF_ENV(env);
  return env->e.observe_sparse_device(d_keys, d_vals, d_counts, d_pov, cap);
}
int sf_results(sf_env *env, int32_t *out_host) {
  SF_ENV(env);
  return env->e.results_host(out_host);
}
int sf_results_device(sf_env *env, int32_t *d_out) {
  SF_ENV(env);
  return env->e.results_device(d_out);
}
int sf_episode_log(sf_env *env, int32_t depth) {
  SF_ENV(env);
  return env->e.episode_log(depth);
}
int sf_episodes(sf_env *env, int32_t *out_host, int32_t max_records, int32_t *counts_host) {
  SF_ENV(env);
  return env->e.episodes_host(out_host, max_records, counts_host);
}
int sf_episodes_device(sf_env *env, int32_t *d_out, int32_t max_records, int32_t *d_counts) {
  SF_ENV(env);
  return env->e.episodes_device(d_out, max_records, d_counts);
}
int sf_episode_ring(sf_env *env, int32_t *out_host) {
  SF_ENV(env);
  return env->e.episode_ring_host(out_host);
}
int sf_replay_load(sf_env *env, const uint8_t *streams, const int64_t *offsets) {
  SF_ENV(env);
  return env->e.replay_load(streams, offsets);
}
int sf_replay_step(sf_env *env) {
  SF_ENV(env);
  return env->e.replay_step();
}
int sf_replay_status(sf_env *env, int32_t *out_host) {
  SF_ENV(env);
  return env->e.replay_status_host(out_host);
}
int sf_replay_status_device(sf_env *env, int32_t *d_out) {
  SF_ENV(env);
  return env->e.replay_status_device(d_out);
}
int sf_replay_commands_device(sf_env *env, uint8_t *d_out) {
  SF_ENV(env);
  return env->e.replay_commands_device(d_out);
}
int sf_done_device(sf_env *env, uint8_t *d_out) {
  SF_ENV(env);
  return env->e.done_device(d_out);
}
int sf_done_view_device(sf_env *env, const int32_t **d_words, int32_t *stride_words, int32_t *agents_per_arena) {
  SF_ENV(env);
  return env->e.done_view_device(d_words, stride_words, agents_per_arena);
}
int sf_done(sf_env *env, uint8_t *out_host) {
  SF_ENV(env);
  return env->e.done_host(out_host);
}
int sf_phase_draws(sf_env *env, int32_t *out_host) {
  SF_ENV(env);
  return env->e.phase_draws_host(out_host);
}
int sf_step_begin(sf_env *env) {
  SF_ENV(env);
  return env->e.step_begin();
}
int sf_step_end(sf_env *env, const uint8_t *cmd) {
  SF_ENV(env);
  return env->e.step_end_host(cmd);
}
int sf_step_end_device(sf_env *env, const uint8_t *d_cmd) {
  SF_ENV(env);
  return env->e.step_end_device(d_cmd);
}
int sf_agent_alive(sf_env *env, uint8_t *out_host) {
  SF_ENV(env);
  return env->e.agent_alive_host(out_host);
}
int sf_agent_alive_device(sf_env *env, uint8_t *d_out) {
  SF_ENV(env);
  return env->e.agent_alive_device(d_out);
}
int sf_state_digest(sf_env *env, uint64_t *out_host) {
  SF_ENV(env);
  return env->e.state_digest(out_host);
}
int sf_dump_arena(sf_env *env, int32_t arena, sf_arena_hdr *hdr, sf_human_rec *humans, sf_zombie_rec *zombies,
                  sf_bullet_rec *bullets, sf_portal_rec *portals, uint8_t *cell_flags, int32_t *cell_dmg,
                  int32_t *cell_portal) {
  SF_ENV(env);
  return env->e.dump_arena(arena, hdr, humans, zombies, bullets, portals, cell_flags, cell_dmg, cell_portal);
}
int sf_state_device(sf_env *env, const sf_state_io *io) {
  SF_ENV(env);
  return env->e.state_device(io);
}
int sf_state_put_device(sf_env *env, const sf_state_put_io *io) {
  if (!env) return fail(SF_ERR_ARG, "sf_state_put_device: null env");
  return env->e.state_put_device(io);
}
int sf_state_put_status(sf_env *env, int64_t out_host[4]) {
  if (!env) return fail(SF_ERR_ARG, "sf_state_put_status: null env");
  return env->e.state_put_status(out_host);
}
int sf_load_arena(sf_env *env, int32_t arena, const sf_arena_hdr *hdr, const sf_human_rec *humans, const sf_zombie_rec *zombies,
                  const sf_bullet_rec *bullets, const sf_portal_rec *portals, const uint8_t *cell_flags, const int32_t *cell_dmg,
                  const int32_t *cell_portal) {
  if (!env) return fail(SF_ERR_ARG, "sf_load_arena: null env");
  return env->e.load_arena(arena, hdr, humans, zombies, bullets, portals, cell_flags, cell_dmg, cell_portal);
}
int sf_state_bytes(sf_env *env, const sf_state_io *io, int64_t bytes_out[10]) {
  SF_ENV(env);
  return env->e.state_bytes(io, bytes_out);
}
int sf_set_stream(sf_env *env, void *hip_stream) {
  SF_ENV(env);
  env->e.rt.stream = reinterpret_cast<hipStream_t>(hip_stream);
  return SF_OK;
}
int sf_synchronize(sf_env *env) {
  SF_ENV(env);
  return env->e.rt.sync();
}
int sf_comm_unique_id(uint8_t *id) {
  if (!id) return sf::fail(SF_ERR_ARG, "null id buffer");
  sf::Comm c;
  int rc = c.load();
  if (rc) return rc;
  return c.nccl(c.get_id(id), "ncclGetUniqueId");  // (the handle of a loaded library is reference-counted by dlopen)
}
int sf_comm_init(sf_env *env, const uint8_t *id, int32_t rank, int32_t world) {
  SF_ENV(env);
  sf::Comm &c = env->comm;
  if (!id || world < 1 || rank < 0 || rank >= world) return sf::fail(SF_ERR_ARG, "bad communicator arguments");
  if (c.comm) return sf::fail(SF_ERR_ARG, "communicator already initialised");
  int rc = c.load();
  if (rc) return rc;
  SF_HIP(hipSetDevice(env->e.rt.device));
  sf::ncclUniqueIdBytes uid;
  memcpy(uid.internal, id, sizeof uid.internal);
  rc = c.nccl(c.init_rank(&c.comm, world, uid, rank), "ncclCommInitRank");
  if (rc) return rc;
  c.world = world, c.rank = rank;
  // a failure from here on leaves no half-built communicator behind: a retry starts from scratch
  const size_t words = (size_t)env->e.p.A * env->e.p.n_agents * 8;
  if (hipStreamCreateWithFlags(&c.side, hipStreamNonBlocking) != hipSuccess || c.results.prepare(words, c.side, "sf_comm_init")) {
    c.shutdown();
    return sf::fail(SF_ERR_DEVICE, "sf_comm_init: stream / event / staging allocation failed");
  }
  return SF_OK;
}
int sf_comm_ranks(sf_env *env, int32_t *ranks) {
  SF_ENV(env);
  sf::Comm &c = env->comm;
  if (!ranks) return sf::fail(SF_ERR_ARG, "null output");
  if (!c.comm) return sf::fail(SF_ERR_ARG, "sf_comm_init has not been called");
  if (!c.count_fn) return sf::fail(SF_ERR_DEVICE, "RCCL lacks ncclCommCount");
  int n = 0;
  int rc = c.nccl(c.count_fn(c.comm, &n), "ncclCommCount");
  if (rc) return rc;
  *ranks = n;
  return SF_OK;
}
int sf_results_allgather(sf_env *env, int32_t *d_out) {
  SF_ENV(env);
  sf::Comm &c = env->comm;
  if (!c.comm) return sf::fail(SF_ERR_ARG, "sf_comm_init has not been called");
  if (!d_out) return sf::fail(SF_ERR_ARG, "null gather buffer");
  if (!env->e.was_reset) return sf::fail(SF_ERR_ARG, "sf_reset has not been called");
  if (int rc0 = env->e.not_mid_step("sf_results_allgather")) return rc0;
  SF_HIP(hipSetDevice(env->e.rt.device));
  return c.gather(c.results, env->e.p.results, (size_t)env->e.p.A * env->e.p.n_agents * 8, d_out, env->e.rt.stream);
}
int sf_episodes_allgather(sf_env *env, int32_t *d_out) {
  SF_ENV(env);
  sf::Comm &c = env->comm;
  if (!c.comm) return sf::fail(SF_ERR_ARG, "sf_comm_init has not been called");
  if (!d_out) return sf::fail(SF_ERR_ARG, "null gather buffer");
  if (int rc0 = env->e.episode_log_state("sf_episodes_allgather")) return rc0;
  SF_HIP(hipSetDevice(env->e.rt.device));
  const size_t count = env->e.ep_ring_words();
  if (int rc0 = c.episodes.prepare(count, c.side, "sf_episodes_allgather")) return rc0;
  const int32_t *ring = reinterpret_cast<const int32_t *>(env->e.tab.ep_ring);  // (read only: the cursors are not touched)
  return c.gather(c.episodes, ring, count, d_out, env->e.rt.stream);
}
int sf_comm_wait(sf_env *env, int32_t host_too) {
  SF_ENV(env);
  sf::Comm &c = env->comm;
  if (!c.comm) return sf::fail(SF_ERR_ARG, "sf_comm_init has not been called");
  SF_HIP(hipSetDevice(env->e.rt.device));
  for (int j = 0; j < 2; ++j)
    for (sf::GatherChannel *ch : {&c.results, &c.episodes})
      if (ch->used[j]) SF_HIP(hipStreamWaitEvent(env->e.rt.stream, ch->done[j], 0));
  if (host_too) SF_HIP(hipStreamSynchronize(c.side));
  return SF_OK;
}
#ifdef SF_DIAG_OBS
int sf_diag_obs_read(sf_env *env, uint32_t *out, int32_t waves) {  // diagnostic build only: [waves][8] cycles of the last launch
  SF_ENV(env);
  if (env->e.rt.sync() != SF_OK) return SF_ERR_DEVICE;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(sf::sf_diag_obs), (size_t)waves * 8 * sizeof(uint32_t)) == hipSuccess ? SF_OK : SF_ERR_DEVICE;
}
#endif
#ifdef SF_DIAG_STAMPS
int sf_diag_times_read(sf_env *env, unsigned long long *out_host, int32_t workgroups) {  // diagnostic build only (tools/r04_k1_times.py)
  SF_ENV(env);
  if (env->e.rt.sync() != SF_OK) return SF_ERR_DEVICE;
  return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(sf::sf_diag_times), (size_t)workgroups * 4 * sizeof(unsigned long long)) == hipSuccess
             ? SF_OK : SF_ERR_DEVICE;
}
int sf_diag_read(sf_env *env, uint32_t *out_host, int32_t arenas) {  // diagnostic build only (tools/diag_stamps.sh)
  SF_ENV(env);
  if (env->e.rt.sync() != SF_OK) return SF_ERR_DEVICE;
  return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(sf::sf_diag_buffer), (size_t)arenas * 16 * sizeof(uint32_t)) == hipSuccess
             ? SF_OK : SF_ERR_DEVICE;
}
#endif
int sf_step_kernel(sf_env *env, int32_t *fixed_shape) {
  SF_ENV(env);
  if (!fixed_shape) return sf::fail(SF_ERR_ARG, "null output");
  *fixed_shape = env->e.rt.last_step_shape;
  return SF_OK;
}
int sf_kernel_time(sf_env *env, int32_t enable, float *ms, int32_t *launches) {
  SF_ENV(env);
  return env->e.rt.kernel_time(enable, ms, launches);
}

}  // extern "C"
