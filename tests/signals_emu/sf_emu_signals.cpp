// TEST INFRASTRUCTURE ONLY: the wave-emulator build of tests/emu (the device core and the host API on the CPU) with a
// runtime that has the launch sf_signals_step needs — k_signals' body, signals_agent (strikeforce_amd/csrc/sf_signals.hpp),
// for every (arena, agent) of the launch in turn — and the launches of everything the signals' cases put between two calls:
// sf_reset_arenas (k_reset_sel's body), sf_snapshot_save / load (k_snapshot's body) and sf_replay_step (k_replay_fetch's
// body), each as tests/reset_sel_emu, tests/snapshot_emu and tests/replay_emu run them.  The host side is the product's
// Env::signals_*, so its refusals are covered too; the pointer checks belong to the HIP runtime and are covered on the
// device (tests/test_gpu_signals.py).  Exports the entry points with an `sfg_` prefix.  Never part of the product library.
#include "../emu/sf_emu.cpp"
#include "../../strikeforce_amd/csrc/sf_snapshot.hpp"

namespace sf {
struct EmuV4 {
  uint8_t b[64][16];
};
struct WaveEmuSig : WaveEmu {
  using V4 = EmuV4;
  static void gstore_u8(uint8_t *base, const V &idx, const V &val, P pred) {
    for (int i = 0; i < 64; ++i)
      if ((pred.m >> i) & 1ull) base[idx.v[i]] = (uint8_t)val.v[i];
  }
  static V rank_below(uint64_t bal) {
    EMU_OP();
    V r;
    for (int i = 0; i < 64; ++i) r.v[i] = (uint32_t)__builtin_popcountll(bal & ((1ull << i) - 1ull));
    return r;
  }
  static V4 gload16(const uint8_t *base, const V &off, P pred) {
    V4 r;
    for (int i = 0; i < 64; ++i)
      if ((pred.m >> i) & 1ull)
        memcpy(r.b[i], base + off.v[i], 16);
      else
        memset(r.b[i], 0, 16);
    return r;
  }
  static void gstore16(uint8_t *base, const V &off, const V4 &val, P pred) {
    for (int i = 0; i < 64; ++i)
      if ((pred.m >> i) & 1ull) memcpy(base + off.v[i], val.b[i], 16);
  }
  static void gstore_u16(uint16_t *base, const V &idx, const V &val, P pred) {
    for (int i = 0; i < 64; ++i)
      if ((pred.m >> i) & 1ull) base[idx.v[i]] = (uint16_t)val.v[i];
  }
  static void ucount(uint32_t *counter) { ++*counter; }
};
struct CpuRTSig : CpuRT {
  Variant last_sel;
  int signals_launches = 0;
  int launch_signals(const Signals &k) {
    ++signals_launches;
    for (int i = 0; i < k.A * k.n_agents; ++i) signals_agent(k, i);
    return SF_OK;
  }
  int launch_reset_sel(const Params &p, int NB, const ResetSel &sel) {
    return with_variant(p, NB, [&](auto v) {
      using VT = decltype(v);
      return each_arena(p, last_sel, v, [&](uint8_t *lds, int a) {
        Core<WaveEmuSig, VT::NB, VT::HP, VT::BM, VT::ZL>::reset_sel_body(lds, p, a, sel);
      });
    });
  }
  int launch_snapshot(const Snap &k, int parts, bool save) {
    for (int a = 0; a < k.A; ++a)
      for (int part = 0; part < parts; ++part) {
        if (save)
          SnapCore<WaveEmuSig, true>::body(k, a, part);
        else
          SnapCore<WaveEmuSig, false>::body(k, a, part);
      }
    return SF_OK;
  }
  int launch_replay_fetch(const Params &p, const Replay &r, int mode) {
    for (int a = 0; a < p.A; ++a) Core<WaveEmuSig, 1>::replay_fetch(p, r, a, mode);
    return SF_OK;
  }
};
}  // namespace sf

struct sfg_env {
  sf::Env<sf::CpuRTSig> e;
};
typedef sf::Env<sf::CpuRTSig>::Snapshot sfg_snapshot;
typedef sf::Env<sf::CpuRTSig>::SignalsObj sfg_signals;

extern "C" {
sfg_env *sfg_create(const sf_config *cfg) {
  sfg_env *env = new sfg_env();
  if (env->e.create(cfg) != SF_OK) {
    env->e.destroy();
    delete env;
    return nullptr;
  }
  return env;
}
int sfg_destroy(sfg_env *env) {
  if (env) {
    env->e.destroy();
    delete env;
  }
  return SF_OK;
}
int sfg_reset(sfg_env *env, const uint64_t *tb, const uint64_t *serial) { return env->e.reset(tb, serial); }
int sfg_reset_arenas(sfg_env *env, const sf_reset_sel *sel) { return env->e.reset_arenas(sel); }
int sfg_step(sfg_env *env, const uint8_t *cmd) { return env->e.step_host(cmd); }
int sfg_step_many(sfg_env *env, const uint8_t *cmds, int32_t k) { return env->e.step_device(cmds, k); }
int sfg_step_begin(sfg_env *env) { return env->e.step_begin(); }
int sfg_step_end(sfg_env *env, const uint8_t *cmd) { return env->e.step_end_host(cmd); }
int sfg_agent_alive(sfg_env *env, uint8_t *out) { return env->e.agent_alive_host(out); }
int sfg_observe(sfg_env *env, float *out) { return env->e.observe_host(out); }
int sfg_results(sfg_env *env, int32_t *out) { return env->e.results_host(out); }
int sfg_done(sfg_env *env, uint8_t *out) { return env->e.done_host(out); }
int sfg_phase_draws(sfg_env *env, int32_t *out) { return env->e.phase_draws_host(out); }
int sfg_state_digest(sfg_env *env, uint64_t *out) { return env->e.state_digest(out); }
int sfg_dump_arena(sfg_env *env, int32_t a, sf_arena_hdr *hdr, sf_human_rec *hs, sf_zombie_rec *zs, sf_bullet_rec *bs,
                   sf_portal_rec *ps, uint8_t *cf, int32_t *cd, int32_t *cp) {
  return env->e.dump_arena(a, hdr, hs, zs, bs, ps, cf, cd, cp);
}
const char *sfg_last_error(void) { return sf::last_error().c_str(); }
int sfg_replay_load(sfg_env *env, const uint8_t *streams, const int64_t *offsets) { return env->e.replay_load(streams, offsets); }
int sfg_replay_step(sfg_env *env) { return env->e.replay_step(); }
int sfg_snapshot_create(sfg_env *env, int32_t slots, sfg_snapshot **out) { return env->e.snapshot_create(slots, out); }
int sfg_snapshot_destroy(sfg_snapshot *s) { return s ? s->owner->snapshot_destroy(s) : SF_OK; }
int sfg_snapshot_slot_bytes(sfg_env *env, int64_t *d, int64_t *b) { return env->e.snapshot_slot_bytes(d, b); }
int sfg_snapshot_save(sfg_env *env, sfg_snapshot *s, const int32_t *slot_of_arena) { return env->e.snapshot_copy(s, slot_of_arena, true); }
int sfg_snapshot_load(sfg_env *env, sfg_snapshot *s, const int32_t *slot_of_arena) { return env->e.snapshot_copy(s, slot_of_arena, false); }
int sfg_snapshot_status(sfg_snapshot *s, int32_t out[4]) { return s->owner->snapshot_status(s, out); }
int sfg_snapshot_export(sfg_snapshot *s, int32_t slot, void *blob, int64_t bytes) { return s->owner->snapshot_export(s, slot, blob, bytes); }
int sfg_snapshot_import(sfg_snapshot *s, int32_t slot, const void *blob, int64_t bytes) { return s->owner->snapshot_import(s, slot, blob, bytes); }
int sfg_signals_create(sfg_env *env, sfg_signals **out) { return env->e.signals_create(out); }
int sfg_signals_destroy(sfg_signals *s) { return s ? s->owner->signals_destroy(s) : SF_OK; }
int sfg_signals_step(sfg_env *env, sfg_signals *s, const sf_signals_io *io) { return env->e.signals_step(s, io); }
int sfg_signals_status(sfg_signals *s, int64_t out[4]) { return s ? s->owner->signals_status(s, out) : SF_ERR_ARG; }
// what k_signals reads of the environment, raw: hum [HW_WORDS][A][H], scal [A][SC_WORDS], results [A][n_agents][8]
int sfg_raw_state(sfg_env *env, uint32_t *hum, int32_t *scal, int32_t *results) {
  const sf::Params &p = env->e.p;
  memcpy(hum, p.hum, (size_t)sf::HW_WORDS * p.A * p.H * 4u);
  memcpy(scal, p.scal, (size_t)p.A * sf::SC_WORDS * 4u);
  memcpy(results, p.results, (size_t)p.A * p.n_agents * 8u * 4u);
  return SF_OK;
}
// launches of the signals kernel since create: a refused call must not add one
int sfg_signals_launches(sfg_env *env) { return env->e.rt.signals_launches; }
}
