// sf_emu.cpp — TEST INFRASTRUCTURE: the device core (strikeforce_amd/csrc/sf_core.hpp, sf_snapshot.hpp, sf_signals.hpp)
// and the host API (sf_host.hpp) compiled for the CPU against a 64-lane wave emulator.  Exports the C-ABI of
// include/strikeforce.h with an `sfe_` prefix, plus observers of what the runtime launched.  Loaded only by tests/ (CPU
// parity of the kernel logic against the oracle, ASan/UBSan runs); never part of, or a fallback for, the product library.
//
// CpuRT has every launch of the product's runtime whose kernel body lives in a shared header: each runs that body for
// every arena (arena and part, agent) in turn, and device pointers are host memory.  Not emulated: k_ep_late (the split
// step's episode records and the rings emptied by sf_reset on the device: sf_host.hpp has_ep_late; sf_reset empties the
// rings with a host-side fill here), k_rank, the sparse / overflow observation kernels and sf_episodes' kernels (sf_api.hip).
#include <stdlib.h>

#include <vector>

#include "wave_emu.hpp"
// clang-format off
#include "../../strikeforce_amd/csrc/sf_core.hpp"
#include "../../strikeforce_amd/csrc/sf_obs.hpp"
#include "../../strikeforce_amd/csrc/sf_host.hpp"
#include "../../strikeforce_amd/csrc/sf_snapshot.hpp"
// clang-format on

namespace sf {

// the template arguments <NB, HP, BM, ZL> of the last launch of each kernel (sfe_last_variant): what the suite's own
// restatement of the choice (tests/variant_cases.py expected_variant) is checked against
enum { LV_RESET = 0, LV_STEP, LV_STEP_HALF, LV_RESET_SEL, LV_KINDS };
struct Variant {
  int32_t nb = 0, hp = 0, bm = 0, zl = 0;
};

// One emulated launch of a per-arena kernel.  The instance is the one the product's own selector picks (sf_types.hpp
// with_variant; big flag planes stay in "HBM", here the host arrays); noted in `last`, then fn(lds, arena) for every arena.
template <class V>
using EmuCore = Core<WaveEmu, V::NB, V::HP, V::BM, V::ZL>;
template <class V, class F>
static int each_arena(const Params &p, Variant &last, V, F fn) {
  last = {V::NB, V::HP, V::BM, V::ZL};
  std::vector<uint8_t> lds(lds_bytes_for(p.cells_pad, p.lds_tab, p.Z, p.P));
  for (int a = 0; a < p.A; ++a) fn(lds.data(), a);
  return SF_OK;
}

static void run_observe(const Params &p, float *out) {
  const int W2 = SF_OBS_WINDOW * SF_OBS_WINDOW;
  std::vector<uint32_t> occ(W2);
  for (int a = 0; a < p.A; ++a)
    for (int g = 0; g < p.n_agents; ++g) {
      float *o = out + ((size_t)a * p.n_agents + g) * SF_OBS_FLOATS;
      ObsView v(p, a);
      const uint32_t hf = v.hum(HW_FLAGS, g);
      if ((hf & (HF_ALIVE | HF_CTRL)) != (HF_ALIVE | HF_CTRL)) {
        for (int i = 0; i < SF_OBS_FLOATS; ++i) o[i] = 0.f;
        continue;
      }
      const uint32_t center = v.hum(HW_POS, g);
      const int pteam = (int)((hf >> HF_TEAM_SH) & 255u);
      for (int w = 0; w < W2; ++w) occ[w] = 0;
      for (int h = 0; h < p.H; ++h)
        if (v.hum(HW_FLAGS, h) & HF_OCC) {
          int s = obs_window_slot(v.hum(HW_POS, h), center);
          if (s >= 0) occ[s] |= (uint32_t)(h + 1);
        }
      for (int z = 0; z < p.Z; ++z)
        if (v.zom(ZW_POS, z) & ZF_ALIVE) {
          int s = obs_window_slot(v.zom(ZW_POS, z) & POS_MASK, center);
          if (s >= 0) occ[s] |= (uint32_t)(z + 1) << OCC_Z_SH;
        }
      for (int b = 0; b < p.B; ++b)
        if (v.bul(BW_A, b) & BA_REF) {
          int s = obs_window_slot(v.bul(BW_A, b) & POS_MASK, center);
          if (s >= 0) occ[s] |= (uint32_t)(b + 1) << OCC_B_SH;
        }
      for (int w = 0; w < W2; ++w) {
        const int i = pos_r(center) - SF_OBS_WINDOW / 2 + w / SF_OBS_WINDOW;
        const int j = pos_c(center) - SF_OBS_WINDOW / 2 + w % SF_OBS_WINDOW;
        uint32_t fl = 0;
        int32_t cdmg = 0;
        if (i >= 0 && j >= 0 && i < p.N && j < p.M) {
          const size_t ci = (size_t)(pos_f(center) * p.N + i) * p.M + j;
          fl = p.flags[(size_t)a * p.cells_pad + ci];
          if (fl & SF_CELL_TEMP) cdmg = p.aux_dmg[(size_t)a * p.cells + ci];
        }
        for (int k = 0; k < SF_OBS_CHANNELS; ++k) o[k * W2 + w] = 0.f;
        obs_cell_emit(v, fl, cdmg, occ[w], pteam, [&](int k, float x) {
          float y;
          if (!obs_map_fast(*p.tab, x, y)) y = obs_map(x);
          o[k * W2 + w] = y;
        });
      }
    }
}

struct CpuRT {
  Variant last[LV_KINDS];
  // the fixed-shape step path (k_step_fixed) is the product's, and opt-in here (sfe_fixed_shapes): a handle that has not
  // opted in runs the generic instance for every configuration, so `last[LV_STEP]` and the op profile name one code path
  int fixed_shape = -1;  // Env::create's choice (sf_types.hpp FixedShapes; -1 under SF_STEP_GENERIC=1 or off every shape)
  bool use_fixed_shapes = false;
  int last_step_shape = -1;  // what the last step launch ran: an index in FixedShapes, -1 a generic instance
  int last_parts = 0;        // the grid's second dimension of the last snapshot launch
  int signals_launches = 0;
  int init(int) { return SF_OK; }
  void shutdown() {}
  size_t max_lds() const { return 160 * 1024; }
  void *alloc(size_t n) { return calloc(n ? n : 1, 1); }
  void free(void *p) { ::free(p); }
  void h2d(void *d, const void *s, size_t n) { memcpy(d, s, n); }
  void d2h(void *d, const void *s, size_t n) { memcpy(d, s, n); }
  void d2d(void *d, const void *s, size_t n) { memcpy(d, s, n); }
  void zero(void *d, size_t n) { memset(d, 0, n); }
  int sync() { return SF_OK; }
  int launch_reset(const Params &p, int NB, const uint64_t *tb, const uint64_t *serial) {
    return with_variant(p, NB, [&](auto v) {
      return each_arena(p, last[LV_RESET], v, [&](uint8_t *lds, int a) { EmuCore<decltype(v)>::reset_body(lds, p, a, tb, serial); });
    });
  }
  int launch_reset_sel(const Params &p, int NB, const ResetSel &sel) {
    return with_variant(p, NB, [&](auto v) {
      return each_arena(p, last[LV_RESET_SEL], v, [&](uint8_t *lds, int a) { EmuCore<decltype(v)>::reset_sel_body(lds, p, a, sel); });
    });
  }
  int launch_step(const Params &p, int NB, const uint8_t *cmds, int k) {
    last_step_shape = use_fixed_shapes && !p.tab->ep_ring ? fixed_shape : -1;  // (the log's records are written by the generic LOG instance)
    if (last_step_shape >= 0)  // (last[LV_STEP] keeps the last GENERIC launch: a fixed one shows in last_step_shape only)
      return with_fixed_shape(last_step_shape, FixedShapes{}, SF_ERR_STATE, [&](auto sh) {
        using SH = decltype(sh);
        std::vector<uint8_t> lds(lds_bytes_for(p.cells_pad, p.lds_tab, p.Z, p.P));
        for (int a = 0; a < p.A; ++a) Core<WaveEmu, SH::NB, false, true, false, SH>::template step_body_t<false>(lds.data(), p, a, cmds, k);
        return (int)SF_OK;
      });
    return with_variant(p, NB, [&](auto v) {
      return each_arena(p, last[LV_STEP], v, [&](uint8_t *lds, int a) { EmuCore<decltype(v)>::step_body(lds, p, a, cmds, k); });
    });
  }
  bool can_rank() const { return false; }  // (a launch order only matters where arenas run side by side)
  int launch_rank(const Params &, uint32_t *) { return SF_OK; }
  int launch_step_half(const Params &p, int NB, const uint8_t *cmds, int phase) {
    return with_variant(p, NB, [&](auto v) {
      return each_arena(p, last[LV_STEP_HALF], v, [&](uint8_t *lds, int a) { EmuCore<decltype(v)>::step_half_body(lds, p, a, cmds, phase); });
    });
  }
  int launch_replay_fetch(const Params &p, const Replay &r, int mode) {
    for (int a = 0; a < p.A; ++a) Core<WaveEmu, 1>::replay_fetch(p, r, a, mode);
    return SF_OK;
  }
  int launch_snapshot(const Snap &k, int parts, bool save) {
    last_parts = parts;
    for (int a = 0; a < k.A; ++a)
      for (int part = 0; part < parts; ++part) {
        if (save)
          SnapCore<WaveEmu, true>::body(k, a, part);
        else
          SnapCore<WaveEmu, false>::body(k, a, part);
      }
    return SF_OK;
  }
  int launch_signals(const Signals &k) {
    ++signals_launches;
    for (int i = 0; i < k.A * k.n_agents; ++i) signals_agent(k, i);
    return SF_OK;
  }
  int launch_agent_alive(const Params &p, uint8_t *out) {
    for (int i = 0; i < p.A * p.n_agents; ++i) {
      const int a = i / p.n_agents, g = i % p.n_agents;
      const uint32_t fl = p.hum[((size_t)HW_FLAGS * (size_t)p.A + (size_t)a) * (size_t)p.H + (size_t)g];
      out[i] = (uint8_t)((fl & (HF_ALIVE | HF_CTRL)) == (HF_ALIVE | HF_CTRL));
    }
    return SF_OK;
  }
  int launch_done(const Params &p, uint8_t *out) {
    for (int i = 0; i < p.A * p.n_agents; ++i) {
      const int32_t *sc = p.scal + (size_t)(i / p.n_agents) * SC_WORDS;
      out[i] = (uint8_t)(p.auto_reset ? sc[SC_ENDED] : sc[SC_DONE]);
    }
    return SF_OK;
  }
  int launch_observe_overflow(const Params &, const uint32_t *, int, float *, float *) { return SF_ERR_DEVICE; }  // device-only form
  int launch_observe_sparse(const Params &, uint32_t *, float *, uint32_t *, float *, int) { return SF_ERR_DEVICE; }
  int launch_observe(const Params &p, int, float *out, uint32_t *, int) {  // (delta mode: same final buffer content)
    run_observe(p, out);
    return SF_OK;
  }
};

}  // namespace sf

struct sfe_env {
  sf::Env<sf::CpuRT> e;
};
typedef sf::Env<sf::CpuRT>::Snapshot sfe_snapshot;
typedef sf::Env<sf::CpuRT>::SignalsObj sfe_signals;

extern "C" {
// op profile of the device source: out[0] = all vector ops, out[1 + ph] = vector ops in phase ph, out[1 + PH_COUNT + ph]
// = wave-uniform accesses (readlane / ballot / setlane / uniform LDS) in phase ph; clears the counters (out: 32 words)
int sfe_profile(uint64_t *out) {
  sf::EmuProf &q = sf::emu_prof();
  q.by[q.phase] += q.ops - q.mark, q.mark = q.ops;
  out[0] = q.ops;
  q.sby[q.phase] += q.sops - q.smark, q.smark = q.sops;
  for (int i = 0; i < sf::PH_COUNT; ++i) out[1 + i] = q.by[i], q.by[i] = 0;
  for (int i = 0; i < sf::PH_COUNT; ++i) out[1 + sf::PH_COUNT + i] = q.sby[i], q.sby[i] = 0;
  q.ops = q.mark = 0, q.sops = q.smark = 0;
  return sf::PH_COUNT;
}
// SF_COUNT(k) path counters of the device source; clears them (out: 8 words)
void sfe_counts(uint64_t *out) {
  sf::EmuProf &q = sf::emu_prof();
  for (int i = 0; i < 8; ++i) out[i] = q.counts[i], q.counts[i] = 0;
}
sfe_env *sfe_create(const sf_config *cfg) {
  sfe_env *env = new sfe_env();
  if (env->e.create(cfg) != SF_OK) {
    env->e.destroy();
    delete env;
    return nullptr;
  }
  return env;
}
int sfe_destroy(sfe_env *env) {
  if (env) {
    env->e.destroy();
    delete env;
  }
  return SF_OK;
}
int sfe_reset(sfe_env *env, const uint64_t *tb, const uint64_t *serial) { return env->e.reset(tb, serial); }
int sfe_reset_arenas(sfe_env *env, const sf_reset_sel *sel) { return env->e.reset_arenas(sel); }
int sfe_step(sfe_env *env, const uint8_t *cmd) { return env->e.step_host(cmd); }
int sfe_step_many(sfe_env *env, const uint8_t *cmds, int32_t k) { return env->e.step_device(cmds, k); }
int sfe_step_begin(sfe_env *env) { return env->e.step_begin(); }
int sfe_step_end(sfe_env *env, const uint8_t *cmd) { return env->e.step_end_host(cmd); }
int sfe_agent_alive(sfe_env *env, uint8_t *out) { return env->e.agent_alive_host(out); }
int sfe_observe(sfe_env *env, float *out) { return env->e.observe_host(out); }
int sfe_results(sfe_env *env, int32_t *out) { return env->e.results_host(out); }
int sfe_done(sfe_env *env, uint8_t *out) { return env->e.done_host(out); }
int sfe_phase_draws(sfe_env *env, int32_t *out) { return env->e.phase_draws_host(out); }
int sfe_state_digest(sfe_env *env, uint64_t *out) { return env->e.state_digest(out); }
int sfe_dump_arena(sfe_env *env, int32_t a, sf_arena_hdr *hdr, sf_human_rec *hs, sf_zombie_rec *zs, sf_bullet_rec *bs,
                   sf_portal_rec *ps, uint8_t *cf, int32_t *cd, int32_t *cp) {
  return env->e.dump_arena(a, hdr, hs, zs, bs, ps, cf, cd, cp);
}
const char *sfe_last_error(void) { return sf::last_error().c_str(); }
int sfe_episode_log(sfe_env *env, int32_t depth) { return env->e.episode_log(depth); }
int sfe_episode_ring(sfe_env *env, int32_t *out) { return env->e.episode_ring_host(out); }
int sfe_replay_load(sfe_env *env, const uint8_t *streams, const int64_t *offsets) { return env->e.replay_load(streams, offsets); }
int sfe_replay_step(sfe_env *env) { return env->e.replay_step(); }
int sfe_replay_status(sfe_env *env, int32_t *out) { return env->e.replay_status_host(out); }
int sfe_replay_commands(sfe_env *env, uint8_t *out) { return env->e.replay_commands_device(out); }  // (one memory here)
int sfe_snapshot_create(sfe_env *env, int32_t slots, sfe_snapshot **out) { return env->e.snapshot_create(slots, out); }
int sfe_snapshot_destroy(sfe_snapshot *s) { return s ? s->owner->snapshot_destroy(s) : SF_OK; }
int sfe_snapshot_slot_bytes(sfe_env *env, int64_t *d, int64_t *b) { return env->e.snapshot_slot_bytes(d, b); }
int sfe_snapshot_save(sfe_env *env, sfe_snapshot *s, const int32_t *slot_of_arena) { return env->e.snapshot_copy(s, slot_of_arena, true); }
int sfe_snapshot_load(sfe_env *env, sfe_snapshot *s, const int32_t *slot_of_arena) { return env->e.snapshot_copy(s, slot_of_arena, false); }
int sfe_snapshot_status(sfe_snapshot *s, int32_t out[4]) { return s->owner->snapshot_status(s, out); }
int sfe_snapshot_export(sfe_snapshot *s, int32_t slot, void *blob, int64_t bytes) { return s->owner->snapshot_export(s, slot, blob, bytes); }
int sfe_snapshot_import(sfe_snapshot *s, int32_t slot, const void *blob, int64_t bytes) { return s->owner->snapshot_import(s, slot, blob, bytes); }
int sfe_signals_create(sfe_env *env, sfe_signals **out) { return env->e.signals_create(out); }
int sfe_signals_destroy(sfe_signals *s) { return s ? s->owner->signals_destroy(s) : SF_OK; }
int sfe_signals_step(sfe_env *env, sfe_signals *s, const sf_signals_io *io) { return env->e.signals_step(s, io); }
int sfe_signals_status(sfe_signals *s, int64_t out[4]) { return s ? s->owner->signals_status(s, out) : SF_ERR_ARG; }

// Observers and switches of the emulated runtime (no counterpart in strikeforce.h).
// out[4] = NB, HP, BM, ZL of the last launch of kernel `kind` (0 reset, 1 step, 2 half step, 3 reset_sel) by a generic
// instance; all 0 before the first
int sfe_last_variant(sfe_env *env, int32_t kind, int32_t *out) {
  if (kind < 0 || kind >= sf::LV_KINDS) return SF_ERR_ARG;
  const sf::Variant &v = env->e.rt.last[kind];
  out[0] = v.nb, out[1] = v.hp, out[2] = v.bm, out[3] = v.zl;
  return SF_OK;
}
// whether this handle's step launches take the fixed-shape path where Env::create found a shape; a new handle does not
int sfe_fixed_shapes(sfe_env *env, int32_t on) {
  env->e.rt.use_fixed_shapes = on != 0;
  return SF_OK;
}
// the fixed shape the last step launch ran (index in sf_types.hpp FixedShapes), -1: a generic instance
int sfe_step_kernel(sfe_env *env) { return env->e.rt.last_step_shape; }
// the grid's second dimension of the last snapshot launch (how many wavefronts shared one arena); 0 before the first
int sfe_last_parts(sfe_env *env) { return env->e.rt.last_parts; }
// launches of the signals kernel since create: a refused call must not add one
int sfe_signals_launches(sfe_env *env) { return env->e.rt.signals_launches; }
// raw words of one arena's scalar block, int32 [24]: what a dump does not show (SC_WARM, SC_ENDED, the pool word counts)
int sfe_scal(sfe_env *env, int32_t a, int32_t *out) {
  memcpy(out, env->e.p.scal + (size_t)a * sf::SC_WORDS, sf::SC_WORDS * sizeof(int32_t));
  return SF_OK;
}
// what k_signals reads of the environment, raw: hum [HW_WORDS][A][H], scal [A][SC_WORDS], results [A][n_agents][8]
int sfe_raw_state(sfe_env *env, uint32_t *hum, int32_t *scal, int32_t *results) {
  const sf::Params &p = env->e.p;
  memcpy(hum, p.hum, (size_t)sf::HW_WORDS * p.A * p.H * 4u);
  memcpy(scal, p.scal, (size_t)p.A * sf::SC_WORDS * 4u);
  memcpy(results, p.results, (size_t)p.A * p.n_agents * 8u * 4u);
  return SF_OK;
}
}
