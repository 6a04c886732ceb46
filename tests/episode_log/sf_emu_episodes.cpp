// TEST INFRASTRUCTURE ONLY: the wave-emulator build of tests/emu (the device core and the host API on the CPU) plus the
// episode-log entry points that need no device kernel of their own: sf_episode_log and sf_episode_ring over the same
// Env<CpuRT>, with the `sfe_` prefix of tests/emu.  What it covers is k_step's part of the log: the emulated step body
// runs the LOG form of sf_core.hpp (latch_results<true>) whenever the log is on, exactly the code of the gfx950 k_step
// instance launched then.  The emulator's runtime has no k_ep_late: the split step's records are not written here, and
// sf_reset empties the rings with a host-side fill; those paths are covered by tests/test_gpu_episode_log.py only.
// Never part of the product library.
#include "../emu/sf_emu.cpp"

extern "C" {
int sfe_episode_log(sfe_env *env, int32_t depth) { return env->e.episode_log(depth); }
int sfe_episode_ring(sfe_env *env, int32_t *out) { return env->e.episode_ring_host(out); }
}
