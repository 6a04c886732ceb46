// TEST INFRASTRUCTURE ONLY: the wave-emulator build of tests/emu (the device core and the host API on the CPU) with the
// fixed-shape step path of the product: the runtime carries `fixed_shape`, so sf_host.hpp Env::create picks the shape as
// it does for the HIP runtime (sf_types.hpp FixedShapes, SF_STEP_GENERIC), and launch_step runs
// Core<WaveEmu, SH::NB, false, true, false, SH>::step_body_t<false> — the body of the gfx950 kernel k_step_fixed<SH> — for
// an environment that matches a shape, the generic instance for any other.  Entry points get the prefix `sfx_`.  Never part
// of the product library.
#include "../emu/sf_emu.cpp"

namespace sf {

struct CpuRTFixed : CpuRT {
  int fixed_shape = -1, last_step_shape = -1;
  int launch_step(const Params &p, int NB, const uint8_t *cmds, int k) {
    last_step_shape = p.tab->ep_ring ? -1 : fixed_shape;  // (the log's records are written by the generic LOG instance)
    if (last_step_shape < 0) return CpuRT::launch_step(p, NB, cmds, k);
    return with_fixed_shape(last_step_shape, FixedShapes{}, SF_ERR_STATE, [&](auto sh) {
      using SH = decltype(sh);
      std::vector<uint8_t> lds(lds_bytes_for(p.cells_pad, p.lds_tab, p.Z, p.P));
      for (int a = 0; a < p.A; ++a) Core<WaveEmu, SH::NB, false, true, false, SH>::template step_body_t<false>(lds.data(), p, a, cmds, k);
      return (int)SF_OK;
    });
  }
};

}  // namespace sf

struct sfx_env {
  sf::Env<sf::CpuRTFixed> e;
};

extern "C" {
sfx_env *sfx_create(const sf_config *cfg) {
  sfx_env *env = new sfx_env();
  if (env->e.create(cfg) != SF_OK) {
    env->e.destroy();
    delete env;
    return nullptr;
  }
  return env;
}
int sfx_destroy(sfx_env *env) {
  if (env) env->e.destroy(), delete env;
  return SF_OK;
}
int sfx_reset(sfx_env *env, const uint64_t *tb, const uint64_t *serial) { return env->e.reset(tb, serial); }
int sfx_step(sfx_env *env, const uint8_t *cmd) { return env->e.step_host(cmd); }
int sfx_step_many(sfx_env *env, const uint8_t *cmds, int32_t k) { return env->e.step_device(cmds, k); }
int sfx_step_begin(sfx_env *env) { return env->e.step_begin(); }
int sfx_step_end(sfx_env *env, const uint8_t *cmd) { return env->e.step_end_host(cmd); }
int sfx_agent_alive(sfx_env *env, uint8_t *out) { return env->e.agent_alive_host(out); }
int sfx_observe(sfx_env *env, float *out) { return env->e.observe_host(out); }
int sfx_results(sfx_env *env, int32_t *out) { return env->e.results_host(out); }
int sfx_done(sfx_env *env, uint8_t *out) { return env->e.done_host(out); }
int sfx_phase_draws(sfx_env *env, int32_t *out) { return env->e.phase_draws_host(out); }
int sfx_state_digest(sfx_env *env, uint64_t *out) { return env->e.state_digest(out); }
int sfx_dump_arena(sfx_env *env, int32_t a, sf_arena_hdr *hdr, sf_human_rec *hs, sf_zombie_rec *zs, sf_bullet_rec *bs,
                   sf_portal_rec *ps, uint8_t *cf, int32_t *cd, int32_t *cp) {
  return env->e.dump_arena(a, hdr, hs, zs, bs, ps, cf, cd, cp);
}
const char *sfx_last_error(void) { return sf::last_error().c_str(); }
// the fixed shape the last step launch ran (index in sf_types.hpp FixedShapes), -1: a generic instance
int sfx_step_kernel(sfx_env *env) { return env->e.rt.last_step_shape; }
}
