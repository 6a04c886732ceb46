// sf_obs_kernels.hpp — the gfx950 observation kernels of libstrikeforce_amd.so (HIP only; sf_api.hip includes it and
// launches them; the per-cell encoder they share with the CPU test build is sf_obs.hpp):
//   k_observe       one 256-thread workgroup per (arena, agent): the dense 32 x 31 x 31 float observation (modes 0-2),
//                   or its non-zero floats as a list (mode 3)
//   k_observe_redo  the dense rows of the agents whose list did not fit (mode 4)
//   k_observe_list  the list form, one wavefront per (arena, agent)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "wave_gfx950.hpp"
// clang-format off
#include "sf_core.hpp"
#include "sf_obs.hpp"
// clang-format on

namespace sf {

constexpr int OBS_W2 = SF_OBS_WINDOW * SF_OBS_WINDOW;  // 961
constexpr int OBS_THREADS = 256;

// workgroup barrier that orders LDS traffic only: global stores issued before it stay in flight
static __device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// inclusive prefix sum of x over the wavefront's 64 lanes (lane: the caller's)
template <class T>
static __device__ __forceinline__ T wave_scan_incl(T x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T up = (T)__shfl_up((int)x, d, 64);
    if (lane >= d) x += up;
  }
  return x;
}
// window cell of the network's pov cell q: (-1,0) (0,-1) (0,0) (0,1) (1,0) around the centre (Modules.hpp:114-121)
constexpr __host__ __device__ int pov_cell(int q) {
  return (SF_OBS_WINDOW / 2 + (q == 0 ? -1 : q == 4 ? 1 : 0)) * SF_OBS_WINDOW + (SF_OBS_WINDOW / 2 + (q == 1 ? -1 : q == 3 ? 1 : 0));
}

constexpr int OBS_Z_STAGE = 256;    // zombie tables up to this many slots are staged in LDS with the other entities
static inline size_t obs_lds_bytes(const Params &p) {
  return (size_t)(HW_WORDS * p.H + (p.Z <= OBS_Z_STAGE ? ZW_WORDS * p.Z : 0) + BW_WORDS * p.B) * sizeof(uint32_t) + sizeof(int32_t) * 12 +
         sizeof(Derived) * (size_t)(p.npc_block + 1);
}
// The observation kernels' limits can be set from the compiler's command line (-DSF_OBS_REC_MAX=24 ...): a test build with
// small limits makes ordinary worlds take every fallback below (tests/obs_flavour.py).  The defaults are the product's.
#ifndef SF_OBS_REC_MAX
#define SF_OBS_REC_MAX 72
#endif
#ifndef SF_OBS_LIST_MAX
#define SF_OBS_LIST_MAX 256
#endif
#ifndef SF_OBS_STAGED
#define SF_OBS_STAGED (2 * OBS_W2)
#endif
#ifndef SF_OL_REC
#define SF_OL_REC 48
#endif
#ifndef SF_OL_POWQ
#define SF_OL_POWQ 384
#endif
#ifndef SF_OL_CELLS
#define SF_OL_CELLS 640
#endif
constexpr int OBS_CLASS_RECS = 8;   // shared records of plain static cells: '#', '^', 'v', 'O', chest types 0-3
constexpr int OBS_REC_MAX = SF_OBS_REC_MAX;     // + cells with an entity or a player-built object on them (own record each)
constexpr int OBS_LIST_MAX = SF_OBS_LIST_MAX;  // (a) values that need a real pow, (b) overflow cells' outputs
constexpr uint32_t OBS_NOREC = 255u;
static_assert(OBS_REC_MAX > OBS_CLASS_RECS && OBS_REC_MAX <= (int)OBS_NOREC && OBS_LIST_MAX >= 1, "a record slot is one byte, 255 = none");

// One workgroup per (arena, agent).  The 123 KB observation is written exactly once, with 16-B-per-lane stores
// that cover whole 128-B lines (scattered 4-byte stores of the few non-zero values cost more HBM time than the
// whole zero stream), so everything is first assembled in LDS:
//   prologue  all HBM reads: the arena's entity tables -> LDS (coalesced), the window's flag bytes / damage
//   pass 2    every entity scatters itself into the window's occupant words (LDS atomics)
//   pass 3    one thread per non-empty window cell builds that cell's 32-float record in LDS; values come from
//             the host-built constant table, the rest (a few per entity) are queued for a real x^(1/5)
//   pass 3b   the queued double-precision pows run densely, one per lane, and land in the records
//   pass 4    stream the output: each lane produces 4 consecutive floats by looking up cell -> record
// record shared by every window cell with this flag byte and nothing on it, or -1
static __device__ __forceinline__ int obs_class_of(uint32_t fl) {
  // (a chain of selects: as a `switch` this became a tree of divergent branches, ~200 scalar mask instructions per use —
  // most of k_observe_list's classify phase)
  int c = -1;
  c = fl == SF_CELL_WALL ? 0 : c;
  c = fl == SF_CELL_PIN_UP ? 1 : c;
  c = fl == SF_CELL_PIN_DN ? 2 : c;
  c = fl == SF_CELL_POUT ? 3 : c;
  c = fl == (SF_CELL_CHEST | (0u << SF_CELL_CONS_SHIFT)) ? 4 : c;
  c = fl == (SF_CELL_CHEST | (1u << SF_CELL_CONS_SHIFT)) ? 5 : c;
  c = fl == (SF_CELL_CHEST | (2u << SF_CELL_CONS_SHIFT)) ? 6 : c;
  c = fl == (SF_CELL_CHEST | (3u << SF_CELL_CONS_SHIFT)) ? 7 : c;
  return c;
}
// mode 0: plain.  mode 1: plain + record which floats are non-zero in nzprev.  mode 2 (sf_observe_device_delta): the
// buffer still holds what the previous call left, nzprev says which floats of it are non-zero: only 16-byte pieces
// with an old or a new non-zero are written.
// mode 3 (sf_observe_sparse_device): no dense buffer at all — the non-zero floats leave as a list in the dense buffer's
// scan order (key = channel * 9 | y << 9 | x << 14: the form k_conv0_sparse's list has, value), `cap` entries per agent at
// most (counts[] says how many there were: more than cap, or 0xffffffff for a window too crowded for the records, tells the
// caller to take the dense path), plus the 160 values around the window's centre that the network reads directly.
struct ObsSparse {
  uint32_t *keys;
  float *vals;
  uint32_t *counts;
  float *pov;
  int cap;
};
// one agent's window (workgroup `bid` of the plain launch)
static __device__ __forceinline__ void observe_agent(const Params &p, float *out, uint32_t *nzprev, int mode, const ObsSparse &sp, const unsigned bid) {
  extern __shared__ __attribute__((aligned(16))) uint32_t ent[];  // [13][H] humans, [3][Z] zombies, [4][B] bullets
  __shared__ float rec[OBS_REC_MAX][SF_OBS_CHANNELS];
  __shared__ uint32_t occ[OBS_W2];
  __shared__ int32_t wdmg[OBS_W2];
  __shared__ uint8_t wfl[OBS_W2 + 3];
  __shared__ uint8_t slot[OBS_W2 + 3];
  __shared__ uint32_t list_idx[OBS_LIST_MAX];
  __shared__ float list_val[OBS_LIST_MAX];
  __shared__ uint32_t nzmap[OBS_W2];  // one bit per output float: non-zero (30752 bits)
  uint32_t *ormap = reinterpret_cast<uint32_t *>(wdmg);  // delta mode, pass 4: the previous call's map (wdmg is dead
                                                          // by then unless a spill follows, and a spill disables delta)
  __shared__ uint32_t cmask[OBS_CLASS_RECS];  // non-zero channels of each class record
  __shared__ uint16_t work[OBS_REC_MAX];      // window cell of record r (r >= OBS_CLASS_RECS)
  __shared__ float t_in[16], t_out[16];       // Tables::obs_in / obs_out (obs_in[0] == 1.0)
  // the leading part of Tables that obs_cell_emit reads through ObsView::tab (cons_items, then the used blocks of
  // der[]): an LDS copy (behind the entity tables in the dynamic allocation), so that the one lane describing a human
  // cell does not walk four dependent L2 loads in get_damage_effect
  const int TAB_WORDS = (int)((sizeof(int32_t) * 12 + sizeof(Derived) * (size_t)(p.npc_block + 1)) / 4);
  static_assert(offsetof(Tables, cons_items) == 0 && offsetof(Tables, der) == sizeof(int32_t) * 12,
                "obs_cell_emit's tables must lead Tables");
  __shared__ uint32_t list_n, rec_n, spill_n;
  const int a = (int)bid / p.n_agents, g = (int)bid % p.n_agents;
  const int tid = (int)threadIdx.x;
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  SF_GLOBAL float *o = gptr(out) + (size_t)bid * SF_OBS_FLOATS;
  SF_GLOBAL f32x4 *o4 = reinterpret_cast<SF_GLOBAL f32x4 *>(o);  // 30752 floats = 7688 x 16 B, 16-B aligned
  // ---- prologue --------------------------------------------------------------------------------------------
  const uint32_t hf = gptr(p.hum)[((size_t)HW_FLAGS * p.A + a) * p.H + g];
  const uint32_t center = gptr(p.hum)[((size_t)HW_POS * p.A + a) * p.H + g];
  SF_GLOBAL uint32_t *old = nzprev ? gptr(nzprev) + (size_t)bid * OBS_W2 : nullptr;
  const bool redo = mode == 4;
  if (mode == 4) {  // sf_observe_overflow_device: the plain dense write, but only for the agents whose list did not fit
    const uint32_t c = gptr(sp.counts)[bid];
    if (!(c == 0xffffffffu || c > (uint32_t)sp.cap)) return;  // (uniform over the workgroup)
    mode = 0;
  }
  if (mode == 3 && (hf & (HF_ALIVE | HF_CTRL)) != (HF_ALIVE | HF_CTRL)) {  // no observer: an empty list
    if (tid == 0) gptr(sp.counts)[bid] = 0u;
    if (tid < 5 * SF_OBS_CHANNELS) gptr(sp.pov)[(size_t)bid * (5 * SF_OBS_CHANNELS) + tid] = 0.f;
    return;
  }
  if ((hf & (HF_ALIVE | HF_CTRL)) != (HF_ALIVE | HF_CTRL)) {  // no observer: all zero (uniform over the workgroup)
    for (int i = tid; i < SF_OBS_FLOATS / 4; i += OBS_THREADS)
      if (mode != 2 || ((old[(4u * (uint32_t)i) >> 5] >> ((4u * (uint32_t)i) & 31u)) & 15u))
        __builtin_nontemporal_store((f32x4)(0.f), &o4[i]);
    if (mode) {
      __syncthreads();  // every old word has been read
      for (int w = tid; w < OBS_W2; w += OBS_THREADS) old[w] = 0u;
    }
    return;
  }
  const bool zstage = p.Z <= OBS_Z_STAGE;  // a larger zombie table is read where it lies (flat loads through ObsView)
  const int nh = HW_WORDS * p.H, nz = zstage ? ZW_WORDS * p.Z : 0, nb = BW_WORDS * p.B;
  uint32_t *tab_lds = ent + nh + nz + nb;
  // Every global load of the prologue is issued before the first LDS store waits for one: the first 256 words of each
  // table and the window's four flag bytes per thread go to registers first.  (Loop by loop, each with its store behind
  // the load, this was a dozen round trips in a row — most of what a workgroup does before it starts to write.)
  auto hum_w = [&](int i) { return gptr(p.hum)[((size_t)(i / p.H) * p.A + a) * p.H + i % p.H]; };
  auto zom_w = [&](int i) { return gptr(p.zom)[((size_t)(i / p.Z) * p.A + a) * p.Z + i % p.Z]; };
  auto bul_w = [&](int i) { return gptr(p.bul)[((size_t)(i / p.B) * p.A + a) * p.B + i % p.B]; };
  auto tab_w = [&](int i) { return reinterpret_cast<const SF_GLOBAL uint32_t *>(gptr(p.tab))[i]; };
  const uint32_t rh = tid < nh ? hum_w(tid) : 0u, rz = tid < nz ? zom_w(tid) : 0u, rb = tid < nb ? bul_w(tid) : 0u;
  const uint32_t rt = tid < TAB_WORDS ? tab_w(tid) : 0u;
  const float r_in = tid < 16 ? gptr(p.tab)->obs_in[tid] : 0.f, r_out = tid < 16 ? gptr(p.tab)->obs_out[tid] : 0.f;
  const int t_n = gptr(p.tab)->obs_n;
  const int pteam = (int)((hf >> HF_TEAM_SH) & 255u);
  const int r0 = pos_r(center) - SF_OBS_WINDOW / 2, c0 = pos_c(center) - SF_OBS_WINDOW / 2, f0 = pos_f(center);
  constexpr int CELL_IT = (OBS_W2 + OBS_THREADS - 1) / OBS_THREADS;  // 4
  uint32_t rfl[CELL_IT];
#pragma unroll
  for (int q = 0; q < CELL_IT; ++q) {
    const int w = tid + q * OBS_THREADS;
    const int i = r0 + w / SF_OBS_WINDOW, j = c0 + w % SF_OBS_WINDOW;
    rfl[q] = (w < OBS_W2 && i >= 0 && j >= 0 && i < p.N && j < p.M) ? (uint32_t)gptr(p.flags)[(size_t)a * p.cells_pad + (size_t)(f0 * p.N + i) * p.M + j] : 0u;
  }
  if (tid < nh) ent[tid] = rh;
  if (tid < nz) ent[nh + tid] = rz;
  if (tid < nb) ent[nh + nz + tid] = rb;
  if (tid < TAB_WORDS) tab_lds[tid] = rt;
  if (tid < 16) t_in[tid] = r_in, t_out[tid] = r_out;
  if (tid == 0) list_n = 0u, rec_n = (uint32_t)OBS_CLASS_RECS, spill_n = 0u;
  for (int i = tid + OBS_THREADS; i < nh; i += OBS_THREADS) ent[i] = hum_w(i);  // (tables of more than 256 words)
  for (int i = tid + OBS_THREADS; i < nz; i += OBS_THREADS) ent[nh + i] = zom_w(i);
  for (int i = tid + OBS_THREADS; i < nb; i += OBS_THREADS) ent[nh + nz + i] = bul_w(i);
  for (int i = tid + OBS_THREADS; i < TAB_WORDS; i += OBS_THREADS) tab_lds[i] = tab_w(i);
#pragma unroll
  for (int q = 0; q < CELL_IT; ++q) {
    const int w = tid + q * OBS_THREADS;
    if (w >= OBS_W2) continue;
    const uint32_t fl = rfl[q];
    int32_t cdmg = 0;
    if (fl & SF_CELL_TEMP) {  // (a player-built object: on the map by construction)
      const int i = r0 + w / SF_OBS_WINDOW, j = c0 + w % SF_OBS_WINDOW;
      cdmg = gptr(p.aux_dmg)[(size_t)a * p.cells + (size_t)(f0 * p.N + i) * p.M + j];
    }
    occ[w] = 0u, wfl[w] = (uint8_t)fl, wdmg[w] = cdmg, slot[w] = (uint8_t)OBS_NOREC, nzmap[w] = 0u;
  }
  lds_barrier();
  // ---- pass 2 ----------------------------------------------------------------------------------------------
  ObsView v(p, 0);  // the LDS copy: one arena, [field][slot]
  v.hum_ = ent, v.bul_ = ent + nh + nz, v.A = 1;
  if (zstage)
    v.zom_ = ent + nh, v.zA = 1, v.za = 0;
  else
    v.zom_ = p.zom, v.zA = p.A, v.za = a;
  v.tab = reinterpret_cast<const Tables *>(tab_lds);
  for (int e = tid; e < p.H + p.Z + p.B; e += OBS_THREADS) {
    int s = -1;
    uint32_t bits = 0;
    if (e < p.H) {
      if (v.hum(HW_FLAGS, e) & HF_OCC) s = obs_window_slot(v.hum(HW_POS, e), center), bits = (uint32_t)(e + 1);
    } else if (e < p.H + p.Z) {
      const int z = e - p.H;
      const uint32_t zp = v.zom(ZW_POS, z);
      if (zp & ZF_ALIVE) s = obs_window_slot(zp & POS_MASK, center), bits = (uint32_t)(z + 1) << OCC_Z_SH;
    } else {
      const int b = e - p.H - p.Z;
      const uint32_t ba = v.bul(BW_A, b);
      if (ba & BA_REF) s = obs_window_slot(ba & POS_MASK, center), bits = (uint32_t)(b + 1) << OCC_B_SH;
    }
    if (s >= 0) atomicOr(&occ[s], bits);
  }
  lds_barrier();
  // ---- pass 3 ----------------------------------------------------------------------------------------------
  // items 0..7 are the shared class records (a pseudo-cell with that class's flag byte and nothing on it), items
  // 8.. are the window cells; one instantiation of obs_cell_emit serves both
  const Tables &tab = *p.tab;
  // 3a: every window cell is classified (empty / plain static cell -> shared class record / needs its own record);
  // the few cells that need a record are queued, so that the heavy feature code below runs once, densely, on
  // consecutive threads instead of once per wavefront per sweep of the window
  for (int w = tid; w < OBS_W2; w += OBS_THREADS) {
    const uint32_t fl = (uint32_t)wfl[w], oc = occ[w];
    if (fl == 0u && oc == 0u) continue;  // '.' with nothing on it
    const int cls = oc == 0u ? obs_class_of(fl) : -1;
    if (cls >= 0) {  // plain static cell: shared record, its non-zero bits are set after the barrier
      slot[w] = (uint8_t)cls;
      continue;
    }
    const uint32_t r = atomicAdd(&rec_n, 1u);
    if (r >= (uint32_t)OBS_REC_MAX) {
      atomicAdd(&spill_n, 1u);  // more non-empty cells than records: written after the stream, see below
      continue;
    }
    slot[w] = (uint8_t)r;
    work[r] = (uint16_t)w;
  }
  lds_barrier();
  // 3b: records 0..7 are the shared class records, finished on the host (Tables::class_rec); records 8.. belong to
  // the queued window cells and are built here
  rec[tid >> 5][tid & 31] = gptr(p.tab)->class_rec[tid >> 5][tid & 31];  // 8 x 32 = OBS_THREADS values
  if (tid < OBS_CLASS_RECS) cmask[tid] = gptr(p.tab)->class_mask[tid];
  const int n_items = (int)(rec_n < (uint32_t)OBS_REC_MAX ? rec_n : (uint32_t)OBS_REC_MAX);
  for (int item = OBS_CLASS_RECS + tid; item < n_items; item += OBS_THREADS) {
    const int w = (int)work[item];
    const uint32_t fl = (uint32_t)wfl[w], oc = occ[w];
    const uint32_t r = (uint32_t)item;
#pragma unroll
    for (int k = 0; k < SF_OBS_CHANNELS; ++k) rec[r][k] = 0.f;
    float ti[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) ti[i] = i < t_n ? t_in[i] : __builtin_nanf("");
    uint32_t mask = 0u;
    obs_cell_emit(v, fl, wdmg[w], oc, pteam, [&](int k, float x) {
      // obs_map_fast() on the LDS copy of the constant table; 1.0 (a set flag) is most of what is emitted
      float y = 0.f;
      bool fast = x == 0.f;
      if (x == 1.f) {
        y = t_out[0], fast = true;
      } else if (!fast) {
        int hit = -1;  // the table's inputs are in registers (ti): a value that is not in it costs 15 compares, no LDS trip
#pragma unroll
        for (int i = 1; i < 16; ++i)
          if (x == ti[i]) hit = i;
        if (hit >= 0) y = t_out[hit], fast = true;
      }
      if (fast && y == 0.f) return;
      mask |= 1u << k;
      if (fast) {
        rec[r][k] = y;
      } else {
        const uint32_t q = atomicAdd(&list_n, 1u);
        if (q < (uint32_t)OBS_LIST_MAX)
          list_idx[q] = r * SF_OBS_CHANNELS + (uint32_t)k, list_val[q] = x;
        else
          rec[r][k] = obs_map(x);
      }
    });
    for (uint32_t m = mask; m; m &= m - 1u) {
      const uint32_t bit = (uint32_t)__builtin_ctz(m) * OBS_W2 + (uint32_t)w;
      atomicOr(&nzmap[bit >> 5], 1u << (bit & 31u));
    }
  }
  lds_barrier();
  for (int w = tid; w < OBS_W2; w += OBS_THREADS) {  // plain static cells: the class's non-zero channels
    const uint32_t sl = slot[w];
    if (sl >= (uint32_t)OBS_CLASS_RECS) continue;
    for (uint32_t m = cmask[sl]; m; m &= m - 1u) {
      const uint32_t bit = (uint32_t)__builtin_ctz(m) * OBS_W2 + (uint32_t)w;
      atomicOr(&nzmap[bit >> 5], 1u << (bit & 31u));
    }
  }
  // ---- pass 3b (same barrier interval: both only consume pass 3's results) -------------------------------------
  {
    const uint32_t n = list_n < (uint32_t)OBS_LIST_MAX ? list_n : (uint32_t)OBS_LIST_MAX;
    for (uint32_t i = (uint32_t)tid; i < n; i += OBS_THREADS) (&rec[0][0])[list_idx[i]] = obs_map(list_val[i]);
  }
  lds_barrier();
  // ---- pass 4, sparse form -----------------------------------------------------------------------------------
  if (mode == 3) {
    __shared__ uint32_t wave_tot[OBS_THREADS / 64];
    // thread t owns bitmap words 4 t .. 4 t + 3 (bits = dense indices in ascending order); an exclusive scan of the
    // threads' non-zero counts gives every entry its place in scan order
    uint32_t wv[4], cnt = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int w = 4 * tid + j;
      wv[j] = w < OBS_W2 ? nzmap[w] : 0u;
      cnt += (uint32_t)__builtin_popcount(wv[j]);
    }
    const uint32_t incl = wave_scan_incl(cnt, tid & 63);
    if ((tid & 63) == 63) wave_tot[tid >> 6] = incl;
    lds_barrier();
    uint32_t pos = incl - cnt, total = 0;
#pragma unroll
    for (int q = 0; q < OBS_THREADS / 64; ++q) {
      if (q < (tid >> 6)) pos += wave_tot[q];
      total += wave_tot[q];
    }
    SF_GLOBAL uint32_t *kd = gptr(sp.keys) + (size_t)bid * (size_t)sp.cap;
    SF_GLOBAL float *vd = gptr(sp.vals) + (size_t)bid * (size_t)sp.cap;
    auto emit = [&](uint32_t e, uint32_t idx) {  // entry e of the list: dense index -> key, value
      const uint32_t k = idx / (uint32_t)OBS_W2, w = idx - k * (uint32_t)OBS_W2;
      const uint32_t y = w / (uint32_t)SF_OBS_WINDOW, x = w - y * (uint32_t)SF_OBS_WINDOW;
      if (e < (uint32_t)sp.cap) kd[e] = (k * 9u) | (y << 9) | (x << 14), vd[e] = rec[slot[w]][k];
    };
    // The non-zeros cluster (a channel that marks every wall cell fills whole bitmap words), so a thread that turned its
    // own bits into entries would make the others wait for the fullest words (13 k of the kernel's 42 k cycles).  The
    // threads only drop their bits' dense indices into an LDS list (occ[] and wdmg[] are dead by now), and the entries
    // are then built and stored round-robin: equal work, coalesced stores.
    constexpr uint32_t STAGED = (uint32_t)(SF_OBS_STAGED);
    static_assert(STAGED <= 2u * (uint32_t)OBS_W2, "the staging area is occ[] and wdmg[]");
    if (total <= STAGED) {
      uint32_t *stage0 = occ, *stage1 = reinterpret_cast<uint32_t *>(wdmg);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        for (uint32_t m = wv[j]; m; m &= m - 1u) {
          const uint32_t idx = 32u * (uint32_t)(4 * tid + j) + (uint32_t)__builtin_ctz(m);
          (pos < (uint32_t)OBS_W2 ? stage0[pos] : stage1[pos - (uint32_t)OBS_W2]) = idx;
          ++pos;
        }
      lds_barrier();
      for (uint32_t e = (uint32_t)tid; e < total; e += OBS_THREADS)
        emit(e, e < (uint32_t)OBS_W2 ? stage0[e] : stage1[e - (uint32_t)OBS_W2]);
    } else {  // more non-zeros than the staging area holds (never an observation of the BASELINE configurations)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        for (uint32_t m = wv[j]; m; m &= m - 1u) {
          emit(pos, 32u * (uint32_t)(4 * tid + j) + (uint32_t)__builtin_ctz(m));
          ++pos;
        }
    }
    if (tid == 0) gptr(sp.counts)[bid] = spill_n ? 0xffffffffu : total;
    if (tid < 5 * SF_OBS_CHANNELS) {  // the network's pov: cells (-1,0) (0,-1) (0,0) (0,1) (1,0) around the centre, Modules.hpp:114-121
      const int cell = tid >> 5, ch = tid & 31;
      const uint32_t w = (uint32_t)pov_cell(cell);
      const uint32_t bit = (uint32_t)ch * (uint32_t)OBS_W2 + w;
      gptr(sp.pov)[(size_t)bid * (5 * SF_OBS_CHANNELS) + tid] = ((nzmap[bit >> 5] >> (bit & 31u)) & 1u) ? rec[slot[w]][ch] : 0.f;
    }
    return;
  }
  // ---- pass 4 ----------------------------------------------------------------------------------------------
  const bool delta = mode == 2 && spill_n == 0u;  // (a window crowded beyond the records is written in full)
  if (delta) {  // the old map next to the new one in LDS (over wdmg): one coalesced read instead of one per piece
    for (int w = tid; w < OBS_W2; w += OBS_THREADS) ormap[w] = old[w];
    lds_barrier();
  }
#pragma unroll 2
  for (int i = tid; i < SF_OBS_FLOATS / 4; i += OBS_THREADS) {
    const uint32_t idx = 4u * (uint32_t)i;
    const uint32_t nib = (nzmap[idx >> 5] >> (idx & 31u)) & 15u;  // idx is a multiple of 4: a nibble never straddles
    if (delta && !(nib | ((ormap[idx >> 5] >> (idx & 31u)) & 15u))) continue;  // was zero, stays zero: not written
    f32x4 val = (f32x4)(0.f);
    if (nib) {  // ~5 % of the 16-B chunks
      uint32_t k = idx / (uint32_t)OBS_W2, w = idx - k * (uint32_t)OBS_W2;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if ((nib >> j) & 1u) val[j] = rec[slot[w]][k];
        if (++w == (uint32_t)OBS_W2) w = 0u, ++k;
      }
    }
    __builtin_nontemporal_store(val, &o4[i]);  // streamed once, never re-read by this kernel
  }
  if (mode)  // what this buffer now holds; after a spill, "anything": the next delta call rewrites it all
    for (int w = tid; w < OBS_W2; w += OBS_THREADS) old[w] = spill_n ? 0xffffffffu : nzmap[w];
  if (spill_n) {  // a window crowded beyond OBS_REC_MAX cells (never in the BASELINE configs): direct, slower
    __syncthreads();  // the streamed zeros of those cells are complete before they are overwritten
    for (int w = tid; w < OBS_W2; w += OBS_THREADS) {
      const uint32_t fl = wfl[w], oc = occ[w];
      if ((fl == 0u && oc == 0u) || slot[w] != OBS_NOREC) continue;
      obs_cell_emit(v, fl, wdmg[w], oc, pteam, [&](int k, float x) {
        float y;
        if (!obs_map_fast(tab, x, y)) y = obs_map(x);
        if (y != 0.f) o[k * OBS_W2 + w] = y;
      });
    }
  }
  if (redo) {  // and the 160 centre values of such an agent, from the dense row just written (a crowded window's records
               // do not cover every cell): cell = t >> 5 of (-1,0) (0,-1) (0,0) (0,1) (1,0), channel = t & 31
    __syncthreads();  // (the workgroup's stores to the row are complete; this CU has not read the row before)
    if (tid < 5 * SF_OBS_CHANNELS) {
      const int cell = tid >> 5, ch = tid & 31;
      const int w = pov_cell(cell);
      gptr(sp.pov)[(size_t)bid * (5 * SF_OBS_CHANNELS) + tid] = o[ch * OBS_W2 + w];
    }
  }
}

__global__ __launch_bounds__(OBS_THREADS, 6) void k_observe(Params p, float *out, uint32_t *nzprev, int mode, ObsSparse sp) {
  observe_agent(p, out, nzprev, mode, sp, blockIdx.x);
}
// sf_observe_overflow_device: a few workgroups walk the agents and redo (mode 4) those whose list did not fit — none, normally,
// and then the launch is one load per thread (as one workgroup per agent the idle launch cost 4 us of a 230 us loop).  A kernel
// of its own: two copies of the window code in one kernel spilled registers.
__global__ __launch_bounds__(OBS_THREADS) void k_observe_redo(Params p, float *out, ObsSparse sp) {
  const unsigned n = (unsigned)(p.A * p.n_agents);
  auto over = [&](unsigned b) {
    const uint32_t c = gptr(sp.counts)[b];
    return c == 0xffffffffu || c > (uint32_t)sp.cap;
  };
  bool mine = false;
  for (unsigned b = blockIdx.x + threadIdx.x * gridDim.x; b < n; b += OBS_THREADS * gridDim.x) mine = mine || over(b);
  if (!__syncthreads_or(mine)) return;
  for (unsigned b = blockIdx.x; b < n; b += gridDim.x) {
    if (!over(b)) continue;  // (uniform over the workgroup)
    observe_agent(p, out, nullptr, 4, sp, b);
    __syncthreads();  // the next agent takes over the workgroup's LDS
  }
}

// ---- sf_observe_sparse_device: the observation as the list of its non-zero floats, one WAVEFRONT per (arena, agent) ----
// The dense kernel above is built around streaming 123 KB per agent; for the list form that stream does not exist and
// what is left — 16 384 wavefronts for 4096 agents, five workgroup barriers around a few hundred useful operations per
// thread — takes 0.075 ms (round 3).  Here one 64-lane wavefront does
// the whole window, without workgroup barriers:
//   0  the window's 961 flag bytes are requested first, all sixteen loads of a lane in flight at once
//   1  every entity of the arena scatters itself into the window's occupant words (LDS atomics)
//   2a the window cells are classified, 64 per pass: empty / plain static cell (one of 8 shared records, finished on the
//      host) / needs a record of its own (an entity or a player-built object on it: ~20 cells) — those are queued
//   2b the queued cells' records are built, one lane each, by the same describe() code as everywhere else; values that
//      need a real x^(1/5) are queued once more and evaluated densely, one per lane (a human cell has ten of them)
//   3  the list leaves in the dense buffer's scan order — channel, then row, then column — which is the order
//      k_feat_list's partial sums are defined over: for every channel, the passes that hold a cell with that channel
//      set (a 16-bit set per channel, from one OR per pass) emit their entries at base + rank-below-me (ballot + mbcnt)
// Same values, same order, same counts as mode 3 of the dense kernel (tests/test_gpu_sparse_obs.py compares the list
// with the dense observation float by float).  A window with more than OL_REC own records is "crowded" (count
// 0xffffffff: the caller takes the dense call for that agent, as before; the dense kernel's own limit is 64).
// LDS: 9.7 KB per wavefront, so that the 16 wavefronts a CU gets of a 4096-agent launch are resident together.
constexpr int OL_REC = SF_OL_REC;                            // own records per window
constexpr int OL_STRIDE = SF_OBS_CHANNELS + 1;        // (odd stride: the lanes of pass 2b write different banks)
constexpr int OL_PASSES = (OBS_W2 + 63) / 64;         // 16
constexpr int OL_POWQ = SF_OL_POWQ;                          // queued x^(1/5) evaluations per window; more are done in place
constexpr int OL_CELLS = SF_OL_CELLS;                         // non-empty cells per window (walls included); more: "crowded"
static_assert(OL_REC + OBS_CLASS_RECS <= 64 && OBS_W2 <= 1024, "a compact cell entry is window cell | slot << 10 in 16 bits");
static_assert(OL_CELLS % 64 == 0 && OL_CELLS >= 64 && OL_POWQ >= 1, "the compact cells leave in whole passes of 64");
// LDS of one window, carved out of a caller-provided region (the stand-alone kernel's own, or k_step's dynamic region
// once the step has stored its state): 16-byte aligned, OL_LDS_BYTES long
struct ObsListLds {
  uint32_t occ_rec[OL_REC * OL_STRIDE];  // the occupant words (961) while cells are classified, then the records
  float crec[OBS_CLASS_RECS][SF_OBS_CHANNELS];
  uint32_t cmask[OBS_CLASS_RECS], recmask[OL_REC], work_oc[OL_REC], powq_n;
  uint16_t cell[OL_CELLS];               // the non-empty cells in window order: window cell | slot << 10
  uint16_t work_w[OL_REC], powq[OL_POWQ];
  uint8_t work_fl[OL_REC];
};
static_assert(OL_REC * OL_STRIDE >= OBS_W2 + 3, "the occupant words fit the record area");
constexpr size_t OL_LDS_BYTES = (sizeof(ObsListLds) + 15) & ~(size_t)15;
static_assert(OL_LDS_BYTES <= 10 * 1024, "16 wavefronts per CU");

#ifdef SF_DIAG_OBS  // diagnostic build only (tools/r04_obs_stamps.py): wave cycles per phase of the list observation
__device__ uint32_t sf_diag_obs[65536 * 8];  // [wave][phase]: the last launch's cycles (no atomics: they would be the measurement)
#define OL_STAMP(ph)                                                                                      \
  do {                                                                                                    \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();                                           \
    if (threadIdx.x == 0 && blockIdx.x < 65536u) sf_diag_obs[blockIdx.x * 8u + (ph)] = (uint32_t)(t_ - ol_last_); \
    ol_last_ = t_;                                                                                        \
  } while (0)
#else
#define OL_STAMP(ph)
#endif

// bitwise OR over the wavefront's 64 lanes, as a wave-uniform value (DPP row steps, then the four row totals)
static __device__ __forceinline__ uint32_t wave_or(uint32_t x) {
  int v = (int)x;
  v |= __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
  v |= __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
  v |= __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true);  // row_half_mirror
  v |= __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true);  // row_mirror: every lane holds its row's OR
  return (uint32_t)(__builtin_amdgcn_readlane(v, 0) | __builtin_amdgcn_readlane(v, 16) | __builtin_amdgcn_readlane(v, 32) |
                    __builtin_amdgcn_readlane(v, 48));
}
static __device__ __forceinline__ uint32_t rank_below(uint64_t bal) {  // set bits of `bal` below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
}

// The list observation of agent `agent` (= arena * n_agents + g) by the calling wavefront; L: OL_LDS_BYTES of LDS.
static __device__ __forceinline__ void observe_list_wave(const Params &p, const ObsSparse &sp, int agent, ObsListLds &L) {
#ifdef SF_DIAG_OBS
  unsigned long long ol_last_ = __builtin_amdgcn_s_memtime();
#endif
  uint32_t *occ = L.occ_rec;
  float *rec = reinterpret_cast<float *>(L.occ_rec);
  const int l = (int)threadIdx.x;
  const int a = agent / p.n_agents, g = agent % p.n_agents;
  const uint32_t hf = gptr(p.hum)[((size_t)HW_FLAGS * p.A + a) * p.H + g];
  const uint32_t center = gptr(p.hum)[((size_t)HW_POS * p.A + a) * p.H + g];
  SF_GLOBAL float *pov = gptr(sp.pov) + (size_t)agent * (5 * SF_OBS_CHANNELS);
  if ((hf & (HF_ALIVE | HF_CTRL)) != (HF_ALIVE | HF_CTRL)) {  // no observer: an empty list (uniform over the wave)
    if (l == 0) gptr(sp.counts)[agent] = 0u;
    for (int t = l; t < 5 * SF_OBS_CHANNELS; t += 64) pov[t] = 0.f;
    return;
  }
  auto crowded = [&]() {  // the caller takes the dense call for this agent
    if (l == 0) gptr(sp.counts)[agent] = 0xffffffffu;
    for (int t = l; t < 5 * SF_OBS_CHANNELS; t += 64) pov[t] = 0.f;  // (sf_observe_overflow_device rewrites it from the dense row)
  };
  // ---- 0: the window's flag bytes --------------------------------------------------------------------------------
  const int pteam = (int)((hf >> HF_TEAM_SH) & 255u);
  const int r0 = pos_r(center) - SF_OBS_WINDOW / 2, c0 = pos_c(center) - SF_OBS_WINDOW / 2, f0 = pos_f(center);
  const SF_GLOBAL uint8_t *plane = gptr(p.flags) + (size_t)a * p.cells_pad + (size_t)f0 * p.N * p.M;
  uint32_t flv[OL_PASSES];
#pragma unroll
  for (int it = 0; it < OL_PASSES; ++it) {
    const int w = it * 64 + l;
    const int i = r0 + w / SF_OBS_WINDOW, j = c0 + w % SF_OBS_WINDOW;
    flv[it] = (w < OBS_W2 && i >= 0 && j >= 0 && i < p.N && j < p.M) ? (uint32_t)plane[i * p.M + j] : 0u;
  }
  OL_STAMP(0);
  // ---- 1: occupant words -------------------------------------------------------------------------------------
  // (every global load of this phase first, into registers: class records, the constant table, the first 64 slots of each
  // entity table — written one by one, each with its LDS store or atomic behind it, they were ten round trips in a row)
  const ObsView v(p, a);  // entity tables where they lie: a window holds ~20 of them
  const uint32_t cm_ld = l < OBS_CLASS_RECS ? gptr(p.tab)->class_mask[l] : 0u;
  float cr_ld[OBS_CLASS_RECS * SF_OBS_CHANNELS / 64];
#pragma unroll
  for (int q = 0; q < OBS_CLASS_RECS * SF_OBS_CHANNELS / 64; ++q) {
    const int t = l + 64 * q;
    cr_ld[q] = gptr(p.tab)->class_rec[t >> 5][t & 31];
  }
  // the host-built constant table (the reference's libm): obs_map_fast.  One entry per lane, read by v_readlane below
  const float t_in = l < 16 ? gptr(p.tab)->obs_in[l] : 0.f, t_out = l < 16 ? gptr(p.tab)->obs_out[l] : 0.f;
  const int t_n = gptr(p.tab)->obs_n;
  // (large pools: only the words of the zombie table that are in use, sf_core.hpp ZL)
  int zlim = p.Z;
  if (large_pools(p.Z, p.P)) {
    const int used = 64 * (int)gptr(p.scal)[(size_t)a * SC_WORDS + SC_ZWN];
    zlim = used < p.Z ? used : p.Z;
  }
  const uint32_t h_fl = l < p.H ? v.hum(HW_FLAGS, l) : 0u, h_pos = l < p.H ? v.hum(HW_POS, l) : 0u;
  const uint32_t z_first = l < zlim ? v.zom(ZW_POS, l) : 0u, b_first = l < p.B ? v.bul(BW_A, l) : 0u;
  for (int w4 = l; w4 < (OBS_W2 + 3) / 4; w4 += 64) reinterpret_cast<u32x4 *>(occ)[w4] = (u32x4)(0u);
  if (l < OBS_CLASS_RECS) L.cmask[l] = cm_ld;
  if (l == 0) L.powq_n = 0u;
#pragma unroll
  for (int q = 0; q < OBS_CLASS_RECS * SF_OBS_CHANNELS / 64; ++q) {
    const int t = l + 64 * q;
    L.crec[t >> 5][t & 31] = cr_ld[q];
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (h_fl & HF_OCC) {
    const int s = obs_window_slot(h_pos, center);
    if (s >= 0) atomicOr(&occ[s], (uint32_t)(l + 1));
  }
  for (int z = l; z < zlim; z += 64) {
    const uint32_t zp = z < 64 ? z_first : v.zom(ZW_POS, z);
    if (zp & ZF_ALIVE) {
      const int s = obs_window_slot(zp & POS_MASK, center);
      if (s >= 0) atomicOr(&occ[s], (uint32_t)(z + 1) << OCC_Z_SH);
    }
  }
  for (int b = l; b < p.B; b += 64) {
    const uint32_t ba = b < 64 ? b_first : v.bul(BW_A, b);
    if (ba & BA_REF) {
      const int s = obs_window_slot(ba & POS_MASK, center);
      if (s >= 0) atomicOr(&occ[s], (uint32_t)(b + 1) << OCC_B_SH);
    }
  }
  __syncthreads();
  OL_STAMP(1);
  // ---- 2a: classify; the non-empty cells are compacted, in window order ----------------------------------------
  uint32_t nrec = 0u, ncell = 0u;  // wave-uniform
#pragma unroll
  for (int it = 0; it < OL_PASSES; ++it) {
    const int w = it * 64 + l;
    const uint32_t fl = flv[it], oc = w < OBS_W2 ? occ[w] : 0u;
    const int cls = oc == 0u ? obs_class_of(fl) : -1;
    const bool some = fl != 0u || oc != 0u, own = some && cls < 0;
    const uint64_t bal = __builtin_amdgcn_ballot_w64(some), balo = __builtin_amdgcn_ballot_w64(own);
    if (some) {
      uint32_t s = (uint32_t)cls;
      if (own) {
        const uint32_t r = nrec + rank_below(balo);
        s = (uint32_t)OBS_CLASS_RECS + (r < (uint32_t)OL_REC ? r : 0u);
        if (r < (uint32_t)OL_REC) L.work_w[r] = (uint16_t)w, L.work_oc[r] = oc, L.work_fl[r] = (uint8_t)fl;
      }
      const uint32_t c = ncell + rank_below(bal);
      if (c < (uint32_t)OL_CELLS) L.cell[c] = (uint16_t)((uint32_t)w | (s << 10));
    }
    nrec += (uint32_t)__builtin_popcountll(balo), ncell += (uint32_t)__builtin_popcountll(bal);
  }
  if (nrec > (uint32_t)OL_REC || ncell > (uint32_t)OL_CELLS) return crowded();
  __syncthreads();  // every occupant word has been read: the records may overwrite them
  OL_STAMP(2);
  // ---- 2b: the queued cells' records, one lane each ------------------------------------------------------------
  const float t_out0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t_out), 0));  // of 1.0: a set flag
  if ((uint32_t)l < nrec) {
    const int w = (int)L.work_w[l];
    const uint32_t fl = L.work_fl[l];
    int32_t cdmg = 0;
    if (fl & SF_CELL_TEMP) {  // (a player-built object: on the map by construction)
      const int i = r0 + w / SF_OBS_WINDOW, j = c0 + w % SF_OBS_WINDOW;
      cdmg = gptr(p.aux_dmg)[(size_t)a * p.cells + (size_t)(f0 * p.N + i) * p.M + j];
    }
    uint32_t m = 0u;
    obs_cell_emit(v, fl, cdmg, L.work_oc[l], pteam, [&](int k, float x) {
      if (x == 0.f) return;
      m |= 1u << k;
      if (x == 1.f) {  // (Tables::obs_in[0] == 1.0: most of what a cell emits)
        rec[l * OL_STRIDE + k] = t_out0;
        return;
      }
      // raw value now; the table / x^(1/5) pass below maps every queued one densely
      rec[l * OL_STRIDE + k] = x;
      const uint32_t q = atomicAdd(&L.powq_n, 1u);
      if (q < (uint32_t)OL_POWQ)
        L.powq[q] = (uint16_t)(l * OL_STRIDE + k);
      else
        rec[l * OL_STRIDE + k] = obs_map(x);  // (obs_map of a table entry is the table's value up to the host's libm; no game reaches this
                                              // at 384, the small-limits test build does and gets the dense kernel's bits, tests/test_gpu_obs_edges.py)
    });
    L.recmask[l] = m;
  }
  __syncthreads();
  OL_STAMP(3);
  {
    const uint32_t nq = L.powq_n < (uint32_t)OL_POWQ ? L.powq_n : (uint32_t)OL_POWQ;
    for (uint32_t q = (uint32_t)l; q < nq; q += 64u) {
      const uint32_t idx = L.powq[q];
      const float x = rec[idx];
      float y = 0.f;
      bool fast = false;
      for (int t = 1; t < t_n; ++t) {
        const float ti = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t_in), t));
        const float to = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t_out), t));
        if (x == ti) y = to, fast = true;
      }
      rec[idx] = fast ? y : obs_map(x);
    }
  }
  __syncthreads();
  OL_STAMP(4);
  // ---- 3: the list, in scan order: channel, then window cell ------------------------------------------------------
  auto mask_of = [&](uint32_t s) { return s < (uint32_t)OBS_CLASS_RECS ? L.cmask[s] : L.recmask[s - OBS_CLASS_RECS]; };
  auto value_of = [&](uint32_t s, uint32_t k) { return s < (uint32_t)OBS_CLASS_RECS ? L.crec[s][k] : rec[(s - OBS_CLASS_RECS) * OL_STRIDE + k]; };
  // the compact cells, 64 per pass: what a lane needs of its cell in each pass stays in registers for the whole channel
  // loop (record, channel mask, the key's position bits), and which channels a pass holds at all
  constexpr int CP_MAX = OL_CELLS / 64;  // 10
  const int npass = (int)((ncell + 63u) / 64u);
  uint32_t cpm = 0u;  // lane i < npass: the OR of pass i's channel masks
  uint32_t pm[CP_MAX], ps[CP_MAX], pkey[CP_MAX];
#pragma unroll
  for (int cp = 0; cp < CP_MAX; ++cp) {
    pm[cp] = 0u, ps[cp] = 0u, pkey[cp] = 0u;
    if (cp >= npass) continue;  // (uniform)
    const uint32_t c = (uint32_t)cp * 64u + (uint32_t)l;
    if (c < ncell) {
      const uint32_t ent = (uint32_t)L.cell[c], w = ent & 1023u;
      const uint32_t y = w / (uint32_t)SF_OBS_WINDOW, x = w - y * (uint32_t)SF_OBS_WINDOW;
      ps[cp] = ent >> 10, pm[cp] = mask_of(ps[cp]), pkey[cp] = (y << 9) | (x << 14);
    }
    const uint32_t o = wave_or(pm[cp]);
    cpm = l == cp ? o : cpm;
  }
  OL_STAMP(5);
  SF_GLOBAL uint32_t *kd = gptr(sp.keys) + (size_t)agent * (size_t)sp.cap;
  SF_GLOBAL float *vd = gptr(sp.vals) + (size_t)agent * (size_t)sp.cap;
  uint32_t base = 0u;
  for (uint32_t chans = wave_or(cpm); chans; chans &= chans - 1u) {  // the channels the window holds at all, ascending
    const uint32_t k = (uint32_t)__builtin_ctz(chans);
    const uint32_t passes = (uint32_t)__builtin_amdgcn_ballot_w64(((cpm >> k) & 1u) != 0u);  // which passes hold channel k
#pragma unroll
    for (int cp = 0; cp < CP_MAX; ++cp) {
      if (!((passes >> cp) & 1u)) continue;  // (uniform)
      const bool has = ((pm[cp] >> k) & 1u) != 0u;
      const uint64_t bal = __builtin_amdgcn_ballot_w64(has);
      if (has) {
        const uint32_t e = base + rank_below(bal);
        if (e < (uint32_t)sp.cap) kd[e] = (k * 9u) | pkey[cp], vd[e] = value_of(ps[cp], k);
      }
      base += (uint32_t)__builtin_popcountll(bal);
    }
  }
  OL_STAMP(6);
  if (l == 0) gptr(sp.counts)[agent] = base;
  // the network's pov: cells (-1,0) (0,-1) (0,0) (0,1) (1,0) around the centre, channel fastest (Modules.hpp:114-121).
  // Their compact entries first (wave-uniform, by ballot over the passes), then 160 lanes' worth of values
  uint32_t pent[5] = {0xffffu, 0xffffu, 0xffffu, 0xffffu, 0xffffu};
  for (int cp = 0; cp < npass; ++cp) {
    const uint32_t c = (uint32_t)cp * 64u + (uint32_t)l;
    const uint32_t ent = c < ncell ? (uint32_t)L.cell[c] : 0xffffu;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      const uint32_t w = (uint32_t)pov_cell(q);
      const uint64_t hit = __builtin_amdgcn_ballot_w64(c < ncell && (ent & 1023u) == w);
      if (hit) pent[q] = (uint32_t)__builtin_amdgcn_readlane((int)ent, __builtin_ctzll(hit));
    }
  }
  for (int t = l; t < 5 * SF_OBS_CHANNELS; t += 64) {
    const int q = t >> 5, ch = t & 31;
    const uint32_t ent = q == 0 ? pent[0] : q == 1 ? pent[1] : q == 2 ? pent[2] : q == 3 ? pent[3] : pent[4];
    const uint32_t s = ent >> 10;
    pov[t] = (ent != 0xffffu && ((mask_of(s) >> ch) & 1u)) ? value_of(s, (uint32_t)ch) : 0.f;
  }
  OL_STAMP(7);
}

__global__ __launch_bounds__(64) void k_observe_list(Params p, ObsSparse sp) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[OL_LDS_BYTES];
  observe_list_wave(p, sp, (int)blockIdx.x, *reinterpret_cast<ObsListLds *>(lds));
}

}  // namespace sf
