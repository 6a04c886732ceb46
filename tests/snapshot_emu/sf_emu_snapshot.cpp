// TEST INFRASTRUCTURE ONLY: the wave-emulator build of tests/emu (the device core and the host API on the CPU) with a
// runtime that has the launch sf_snapshot_save / sf_snapshot_load need: k_snapshot's body, SnapCore<W, SAVE>::body
// (strikeforce_amd/csrc/sf_snapshot.hpp), for every (arena, part) of the launch's grid in turn.  The host side is the
// product's Env::snapshot_*, so layout, refusals, blob code and fingerprint are covered too; the pointer checks belong to
// the HIP runtime and are covered on the device (tests/test_gpu_snapshot.py).  Exports the entry points with an `sfn_`
// prefix beside tests/emu's `sfe_` ones.  Never part of the product library.
#include "../emu/sf_emu.cpp"
#include "../../strikeforce_amd/csrc/sf_snapshot.hpp"

namespace sf {
// the wave operations the copy body uses that tests/emu's emulator lacks
struct EmuV4 {
  uint8_t b[64][16];
};
struct WaveEmuSnap : WaveEmu {
  using V4 = EmuV4;
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
struct CpuRTSnap : CpuRT {
  int last_parts = 0;
  int launch_snapshot(const Snap &k, int parts, bool save) {
    last_parts = parts;
    for (int a = 0; a < k.A; ++a)
      for (int part = 0; part < parts; ++part) {
        if (save)
          SnapCore<WaveEmuSnap, true>::body(k, a, part);
        else
          SnapCore<WaveEmuSnap, false>::body(k, a, part);
      }
    return SF_OK;
  }
};
}  // namespace sf

struct sfn_env {
  sf::Env<sf::CpuRTSnap> e;
};
typedef sf::Env<sf::CpuRTSnap>::Snapshot sfn_snapshot;

extern "C" {
sfn_env *sfn_create(const sf_config *cfg) {
  sfn_env *env = new sfn_env();
  if (env->e.create(cfg) != SF_OK) {
    env->e.destroy();
    delete env;
    return nullptr;
  }
  return env;
}
int sfn_destroy(sfn_env *env) {
  if (env) {
    env->e.destroy();
    delete env;
  }
  return SF_OK;
}
int sfn_reset(sfn_env *env, const uint64_t *tb, const uint64_t *serial) { return env->e.reset(tb, serial); }
int sfn_step(sfn_env *env, const uint8_t *cmd) { return env->e.step_host(cmd); }
int sfn_step_many(sfn_env *env, const uint8_t *cmds, int32_t k) { return env->e.step_device(cmds, k); }
int sfn_step_begin(sfn_env *env) { return env->e.step_begin(); }
int sfn_step_end(sfn_env *env, const uint8_t *cmd) { return env->e.step_end_host(cmd); }
int sfn_agent_alive(sfn_env *env, uint8_t *out) { return env->e.agent_alive_host(out); }
int sfn_observe(sfn_env *env, float *out) { return env->e.observe_host(out); }
int sfn_results(sfn_env *env, int32_t *out) { return env->e.results_host(out); }
int sfn_done(sfn_env *env, uint8_t *out) { return env->e.done_host(out); }
int sfn_phase_draws(sfn_env *env, int32_t *out) { return env->e.phase_draws_host(out); }
int sfn_state_digest(sfn_env *env, uint64_t *out) { return env->e.state_digest(out); }
int sfn_dump_arena(sfn_env *env, int32_t a, sf_arena_hdr *hdr, sf_human_rec *hs, sf_zombie_rec *zs, sf_bullet_rec *bs,
                   sf_portal_rec *ps, uint8_t *cf, int32_t *cd, int32_t *cp) {
  return env->e.dump_arena(a, hdr, hs, zs, bs, ps, cf, cd, cp);
}
int sfn_replay_load(sfn_env *env, const uint8_t *streams, const int64_t *offsets) { return env->e.replay_load(streams, offsets); }
const char *sfn_last_error(void) { return sf::last_error().c_str(); }
int sfn_snapshot_create(sfn_env *env, int32_t slots, sfn_snapshot **out) { return env->e.snapshot_create(slots, out); }
int sfn_snapshot_destroy(sfn_snapshot *s) { return s ? s->owner->snapshot_destroy(s) : SF_OK; }
int sfn_snapshot_slot_bytes(sfn_env *env, int64_t *d, int64_t *b) { return env->e.snapshot_slot_bytes(d, b); }
int sfn_snapshot_save(sfn_env *env, sfn_snapshot *s, const int32_t *slot_of_arena) { return env->e.snapshot_copy(s, slot_of_arena, true); }
int sfn_snapshot_load(sfn_env *env, sfn_snapshot *s, const int32_t *slot_of_arena) { return env->e.snapshot_copy(s, slot_of_arena, false); }
int sfn_snapshot_status(sfn_snapshot *s, int32_t out[4]) { return s->owner->snapshot_status(s, out); }
int sfn_snapshot_export(sfn_snapshot *s, int32_t slot, void *blob, int64_t bytes) { return s->owner->snapshot_export(s, slot, blob, bytes); }
int sfn_snapshot_import(sfn_snapshot *s, int32_t slot, const void *blob, int64_t bytes) { return s->owner->snapshot_import(s, slot, blob, bytes); }
// the grid's second dimension of the last snapshot launch (how many wavefronts shared one arena); 0 before the first
int sfn_last_parts(sfn_env *env) { return env->e.rt.last_parts; }
// raw words of one arena's scalar block, int32 [24]: what a dump does not show (SC_WARM, SC_ENDED, the pool word counts)
int sfn_scal(sfn_env *env, int32_t a, int32_t *out) {
  memcpy(out, env->e.p.scal + (size_t)a * sf::SC_WORDS, sf::SC_WORDS * sizeof(int32_t));
  return SF_OK;
}
}
