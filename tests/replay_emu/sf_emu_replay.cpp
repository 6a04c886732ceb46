// TEST INFRASTRUCTURE ONLY: the wave-emulator build of tests/emu (the device core and the host API on the CPU) plus the
// replay of logged games with the command lines fetched by the DEVICE's own code: sf_core.hpp Core::replay_fetch, the body
// of the gfx950 kernel k_replay_fetch, run here on the emulated wavefront between the emulated halves of the step
// (Env::replay_step: fetch mode 0, step_half 1, fetch mode 1, step_half 2 — the launch sequence of sf_replay_step).  The
// emulator of tests/emu lacks the two wave operations the fetch adds (a byte store and the rank of a lane in a ballot),
// and its runtime the launcher: both are added here, on types derived from it, and the entry points get the prefix
// `sfr_`.  Never part of the product library.
#include "../emu/sf_emu.cpp"

namespace sf {

struct WaveEmuReplay : WaveEmu {
  static void gstore_u8(uint8_t *base, const V &idx, const V &val, P pred) {
    for (int i = 0; i < 64; ++i)
      if ((pred.m >> i) & 1ull) base[idx.v[i]] = (uint8_t)val.v[i];
  }
  static V rank_below(uint64_t bal) {  // v_mbcnt_lo / v_mbcnt_hi
    EMU_OP();
    V r;
    for (int i = 0; i < 64; ++i) r.v[i] = (uint32_t)__builtin_popcountll(bal & ((1ull << i) - 1ull));
    return r;
  }
};

struct CpuRTReplay : CpuRT {
  int launch_replay_fetch(const Params &p, const Replay &r, int mode) {
    for (int a = 0; a < p.A; ++a) Core<WaveEmuReplay, 1>::replay_fetch(p, r, a, mode);
    return SF_OK;
  }
};

}  // namespace sf

struct sfr_env {
  sf::Env<sf::CpuRTReplay> e;
};

extern "C" {
sfr_env *sfr_create(const sf_config *cfg) {
  sfr_env *env = new sfr_env();
  if (env->e.create(cfg) != SF_OK) {
    env->e.destroy();
    delete env;
    return nullptr;
  }
  return env;
}
int sfr_destroy(sfr_env *env) {
  if (env) env->e.destroy(), delete env;
  return SF_OK;
}
int sfr_reset(sfr_env *env, const uint64_t *tb, const uint64_t *serial) { return env->e.reset(tb, serial); }
int sfr_step(sfr_env *env, const uint8_t *cmd) { return env->e.step_host(cmd); }
int sfr_step_begin(sfr_env *env) { return env->e.step_begin(); }
int sfr_step_end(sfr_env *env, const uint8_t *cmd) { return env->e.step_end_host(cmd); }
int sfr_agent_alive(sfr_env *env, uint8_t *out) { return env->e.agent_alive_host(out); }
int sfr_observe(sfr_env *env, float *out) { return env->e.observe_host(out); }
int sfr_results(sfr_env *env, int32_t *out) { return env->e.results_host(out); }
int sfr_done(sfr_env *env, uint8_t *out) { return env->e.done_host(out); }
int sfr_state_digest(sfr_env *env, uint64_t *out) { return env->e.state_digest(out); }
int sfr_dump_arena(sfr_env *env, int32_t a, sf_arena_hdr *hdr, sf_human_rec *hs, sf_zombie_rec *zs, sf_bullet_rec *bs,
                   sf_portal_rec *ps, uint8_t *cf, int32_t *cd, int32_t *cp) {
  return env->e.dump_arena(a, hdr, hs, zs, bs, ps, cf, cd, cp);
}
const char *sfr_last_error(void) { return sf::last_error().c_str(); }
int sfr_replay_load(sfr_env *env, const uint8_t *streams, const int64_t *offsets) { return env->e.replay_load(streams, offsets); }
int sfr_replay_step(sfr_env *env) { return env->e.replay_step(); }
int sfr_replay_status(sfr_env *env, int32_t *out) { return env->e.replay_status_host(out); }
int sfr_replay_commands(sfr_env *env, uint8_t *out) { return env->e.replay_commands_device(out); }  // (one memory here)
}
