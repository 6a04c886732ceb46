// emu_state.cpp — the wave emulator's runtime (tests/emu/sf_emu.cpp, included as it is) has no state-put launches:
// has_state_put<CpuRT> is false, and sf_state_put_device / sf_load_arena answer SF_ERR_STATE there whatever they are given.
// Built and run by tests/test_state_put_api.py.
#include <cstdio>
#include <cstring>

#include "../emu/sf_emu.cpp"

static_assert(!sf::has_state_put<sf::CpuRT>::value, "the wave emulator has no put");
static_assert(!sf::has_state_records<sf::CpuRT>::value, "... as it has no state-record kernels");

int main() {
  sf_config c;
  sf::config_defaults(&c);
  c.floors = 1, c.rows = 8, c.cols = 8, c.cap_humans = 1, c.cap_zombies = 4, c.cap_bullets = 8, c.cap_portals = 4;
  char map[65];
  std::memset(map, '.', 64);
  map[64] = 0;
  c.map = map;
  sfe_env *env = sfe_create(&c);
  if (!env) return std::printf("emu_state: create failed: %s\n", sfe_last_error()), 1;
  sf_state_put_io io;
  std::memset(&io, 0, sizeof io);
  sf_arena_hdr hdr;
  std::memset(&hdr, 0, sizeof hdr);
  const int a = env->e.state_put_device(&io);
  const bool said = std::strstr(sfe_last_error(), "no state-put kernels") != nullptr;
  const int b = env->e.load_arena(0, &hdr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  sfe_destroy(env);
  if (a != SF_ERR_STATE || b != SF_ERR_STATE || !said) return std::printf("emu_state: %d %d %d\n", a, b, (int)said), 1;
  std::printf("emu_state ok\n");
  return 0;
}
