// TEST INFRASTRUCTURE ONLY: the wave-emulator build of tests/emu (the device core and the host API on the CPU) with a
// runtime that has the launch sf_reset_arenas needs: k_reset_sel's body, Core<WaveEmu, ..>::reset_sel_body, for every arena
// in turn, the instance picked by the product's own selector (sf_types.hpp with_variant).  The host side is the product's
// Env::reset_arenas, so its refusals are covered too; the pointer checks belong to the HIP runtime and are covered on the
// device (tests/test_gpu_reset_sel.py).  Exports the entry points with an `sfs_` prefix beside tests/emu's `sfe_` ones.
// Never part of the product library.
#include "../emu/sf_emu.cpp"

namespace sf {
// the one wave operation reset_sel_body uses that tests/emu's emulator lacks: the byte store of d_selected
struct WaveEmuSel : WaveEmu {
  static void gstore_u8(uint8_t *base, const V &idx, const V &val, P pred) {
    for (int i = 0; i < 64; ++i)
      if ((pred.m >> i) & 1ull) base[idx.v[i]] = (uint8_t)val.v[i];
  }
};
struct CpuRTSel : CpuRT {
  Variant last_sel;
  int launch_reset_sel(const Params &p, int NB, const ResetSel &sel) {
    return with_variant(p, NB, [&](auto v) {
      using VT = decltype(v);
      return each_arena(p, last_sel, v, [&](uint8_t *lds, int a) {
        Core<WaveEmuSel, VT::NB, VT::HP, VT::BM, VT::ZL>::reset_sel_body(lds, p, a, sel);
      });
    });
  }
};
}  // namespace sf

struct sfs_env {
  sf::Env<sf::CpuRTSel> e;
};

extern "C" {
sfs_env *sfs_create(const sf_config *cfg) {
  sfs_env *env = new sfs_env();
  if (env->e.create(cfg) != SF_OK) {
    env->e.destroy();
    delete env;
    return nullptr;
  }
  return env;
}
int sfs_destroy(sfs_env *env) {
  if (env) {
    env->e.destroy();
    delete env;
  }
  return SF_OK;
}
int sfs_reset(sfs_env *env, const uint64_t *tb, const uint64_t *serial) { return env->e.reset(tb, serial); }
int sfs_reset_arenas(sfs_env *env, const sf_reset_sel *sel) { return env->e.reset_arenas(sel); }
int sfs_step(sfs_env *env, const uint8_t *cmd) { return env->e.step_host(cmd); }
int sfs_step_many(sfs_env *env, const uint8_t *cmds, int32_t k) { return env->e.step_device(cmds, k); }
int sfs_step_begin(sfs_env *env) { return env->e.step_begin(); }
int sfs_step_end(sfs_env *env, const uint8_t *cmd) { return env->e.step_end_host(cmd); }
int sfs_agent_alive(sfs_env *env, uint8_t *out) { return env->e.agent_alive_host(out); }
int sfs_observe(sfs_env *env, float *out) { return env->e.observe_host(out); }
int sfs_results(sfs_env *env, int32_t *out) { return env->e.results_host(out); }
int sfs_done(sfs_env *env, uint8_t *out) { return env->e.done_host(out); }
int sfs_phase_draws(sfs_env *env, int32_t *out) { return env->e.phase_draws_host(out); }
int sfs_state_digest(sfs_env *env, uint64_t *out) { return env->e.state_digest(out); }
int sfs_dump_arena(sfs_env *env, int32_t a, sf_arena_hdr *hdr, sf_human_rec *hs, sf_zombie_rec *zs, sf_bullet_rec *bs,
                   sf_portal_rec *ps, uint8_t *cf, int32_t *cd, int32_t *cp) {
  return env->e.dump_arena(a, hdr, hs, zs, bs, ps, cf, cd, cp);
}
int sfs_episode_log(sfs_env *env, int32_t depth) { return env->e.episode_log(depth); }
int sfs_episode_ring(sfs_env *env, int32_t *out) { return env->e.episode_ring_host(out); }
int sfs_replay_load(sfs_env *env, const uint8_t *streams, const int64_t *offsets) { return env->e.replay_load(streams, offsets); }
const char *sfs_last_error(void) { return sf::last_error().c_str(); }
// out[4] = NB, HP, BM, ZL of the last k_reset_sel launch; all 0 before the first
int sfs_last_variant(sfs_env *env, int32_t, int32_t *out) {
  const sf::Variant &v = env->e.rt.last_sel;
  out[0] = v.nb, out[1] = v.hp, out[2] = v.bm, out[3] = v.zl;
  return SF_OK;
}
}
