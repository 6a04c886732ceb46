// sf_host.hpp — host side of the C-ABI (include/strikeforce.h): configuration checks, the derived
// stat tables (Human::build), HBM allocation, launches and the parity tooling (dump / digest).
//
// Template over a runtime RT that owns memory and launches.  The product instantiates it with the HIP
// runtime (sf_api.hip); tests/emu instantiates it with a CPU runtime that runs the same device core on a
// wave emulator.  There is no CPU path in the product: HipRT fails with SF_ERR_DEVICE without a GPU.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/strikeforce.h"
#include "sf_types.hpp"
#include "sf_obs.hpp"
#include "sf_snapshot_blob.hpp"
#include "sf_signals.hpp"
#include "sf_record.hpp"
#include "sf_state_records.hpp"
#include "sf_state_put.hpp"

namespace sf {

inline std::string &last_error() {
  static thread_local std::string e;
  return e;
}
inline int fail(int code, const std::string &msg) {
  last_error() = msg;
  return code;
}

// Character.hpp:29-45 compute_damage (only ever called on per-profile constants, so it runs on the host
// once and the device reads Derived::cd_punch / cd_weapon).  Note the reference's indentation: only
// `tmp /= mid` belongs to the for.
inline int host_compute_damage(int x, int y) {
  int l = 0, r = x + 1, z = 2;
  for (; 1 < y; y >>= 1) ++z;
  while (r - l > 1) {
    const int mid = (l + r) >> 1;
    int tmp = x;
    for (int i = 0; i < z && mid; ++i) tmp /= mid;
    if (tmp)
      l = mid;
    else
      r = mid;
  }
  return l;
}

// The generator's tables (sf_types.hpp LOGT_*, Params::logt / exptab): discrete logs and powers of the generator 3 of
// Z/65537*.  logt[LOGT_ENTRIES] must come in zeroed (the entries of residue 0 stay 0), exptab holds 512 words.  A function
// of its own so that tests/wave_probe checks the very tables the product uploads.
inline void build_rng_tables(uint16_t *logt, uint32_t *exptab) {
  uint32_t v = 1;
  for (uint32_t m = 0; m < 65536; ++m) {
    logt[LOGT_OFF + v] = (uint16_t)m;                                              // t = v
    if (v + (uint32_t)LOGT_OFF >= 65537u) logt[LOGT_OFF + v - 65537u] = (uint16_t)m;  // t = v - 65537 < 0
    if (m < 256) exptab[m] = v;
    if ((m & 255u) == 0) exptab[256 + (m >> 8)] = v;
    v = (uint32_t)(((uint64_t)v * 3u) % 65537u);
  }
}

// Human::build, Character.hpp:650-709: what a freshly built human of this profile carries.
inline void derive_profile(const sf_config &cfg, const sf_profile &pr, Derived &d) {
  int def_blocks = 8, def_portals = 1;  // Character.hpp:78-79
  int md = pr.mindamage_def;
  d.hp = pr.def_hp, d.mindamage = pr.mindamage_def, d.stamina = pr.def_stamina;  // Character.hpp:667
  for (int i = 0; i < 4; ++i) d.cons[i] = pr.cons[i];
  for (int i = 0; i < 4; ++i) {
    const int lvl = pr.throw_lvl_cnt[i][0];
    const int up = lvl - 1 > 0 ? lvl - 1 : 0;  // Character.hpp:674-675
    d.thr_cnt[i] = pr.throw_lvl_cnt[i][1];
    d.thr[i][0] = cfg.items.thr[i][0];
    d.thr[i][1] = cfg.items.thr[i][1] + 50 * up;  // Weapon::upgrade Item.hpp:105-111
    d.thr[i][2] = cfg.items.thr[i][2] - 50 * up;
    d.thr[i][3] = cfg.items.thr[i][3];
  }
  for (int i = 0; i < 8; ++i) {
    const int lvl = pr.weapon_lvl[i] > 0 ? pr.weapon_lvl[i] : 0;  // Character.hpp:680-681
    d.weapon_lvl[i] = pr.weapon_lvl[i];
    d.weapon[i][0] = cfg.items.weapon[i][0];
    d.weapon[i][1] = cfg.items.weapon[i][1] + 50 * lvl;
    d.weapon[i][2] = cfg.items.weapon[i][2] - 50 * lvl;
    d.weapon[i][3] = cfg.items.weapon[i][3];
  }
  const int lv[3] = {pr.level_solo, pr.level_timer, pr.level_squad};  // Character.hpp:689-706
  for (int m = 0; m < 3; ++m)
    for (int level = 2; level <= lv[m]; ++level) {  // level_*_up Character.hpp:765-807
      md += 5;
      if (level % 2 == 1) ++def_blocks, ++def_portals;
    }
  d.mindamage_def = md;
  d.blocks = def_blocks, d.portals = def_portals;  // back_tmp Character.hpp:139-144
}

inline void finish_derived(Derived &d) {
  d.cd_punch = host_compute_damage(d.mindamage_def, 1);
  for (int i = 0; i < 8; ++i) d.cd_weapon[i] = host_compute_damage(d.weapon[i][1], d.weapon[i][3]);
}

// Tables::hatab (sf_types.hpp HT_*): obey()'s key classes (gameplay.hpp:695-821) and the per-profile stats its
// shooting / selection branches read, as one flat table that the step kernel keeps in LDS
inline void fill_hatab(Tables &t, int blocks) {
  memset(t.hatab, 0, sizeof t.hatab);
  uint8_t *cmd = reinterpret_cast<uint8_t *>(t.hatab + HT_CMD);
  auto put = [&](char c, int cls, int prm) { cmd[(unsigned char)c] = (uint8_t)(cls | (prm << 4)); };
  put('_', CL_SUICIDE, 0), put('[', CL_BLOCK, 0), put(']', CL_PORTAL, 0), put('q', CL_TURN, 0), put('e', CL_TURN, 1);
  put('s', CL_MOVE, 0), put('d', CL_MOVE, 1), put('w', CL_MOVE, 2), put('a', CL_MOVE, 3);
  const char *selc = "fghj", *selt = "kl;'", *selw = "cvbnm,./";
  for (int k = 0; k < 4; ++k) put(selc[k], CL_SELC, k), put(selt[k], CL_SELT, k);
  for (int k = 0; k < 8; ++k) put(selw[k], CL_SELW, k);
  put('u', CL_USE, 0), put('z', CL_PUNCH, 0), put('x', CL_FIRE, 0);
  for (int pr = 0; pr < blocks; ++pr) {
    uint32_t *w = t.hatab + HT_PROF + pr * HT_PROF_STRIDE;
    const Derived &d = t.der[pr];
    w[HT_P_CDPUNCH] = (uint32_t)d.cd_punch;
    for (int k = 0; k < 8; ++k) {
      w[HT_P_WLVL + k] = (uint32_t)d.weapon_lvl[k], w[HT_P_CDW + k] = (uint32_t)d.cd_weapon[k];
      for (int j = 0; j < 4; ++j) w[HT_P_WEAPON + 4 * k + j] = (uint32_t)d.weapon[k][j];
    }
    for (int k = 0; k < 4; ++k)
      for (int j = 0; j < 4; ++j) w[HT_P_THR + 4 * k + j] = (uint32_t)d.thr[k][j];
  }
  for (int k = 0; k < 4; ++k)
    for (int j = 0; j < 3; ++j) t.hatab[HT_CONS + 3 * k + j] = (uint32_t)t.cons_items[k][j];
}

inline int validate(const sf_config *c) {
  if (!c) return fail(SF_ERR_ARG, "null config");
  if (c->abi_version != SF_ABI_VERSION) return fail(SF_ERR_ARG, "abi_version mismatch");
  if (!c->map) return fail(SF_ERR_ARG, "config.map is null");
  if (c->arenas < 1) return fail(SF_ERR_ARG, "arenas < 1");
  if (c->floors < 1 || c->floors > 4) return fail(SF_ERR_ARG, "floors must be 1..4");
  if (c->rows < 3 || c->cols < 3 || c->rows > SF_MAX_COORD || c->cols > SF_MAX_COORD)
    return fail(SF_ERR_ARG, "rows/cols must be 3..1024");
  if (c->cap_humans < 1 || c->cap_humans > SF_MAX_HUMANS) return fail(SF_ERR_ARG, "cap_humans must be 1..64");
  if (c->cap_zombies < 1 || c->cap_zombies > SF_MAX_ZOMBIES) return fail(SF_ERR_ARG, "cap_zombies must be 1..9000");
  if (c->cap_bullets < 1 || c->cap_bullets > SF_MAX_BULLETS) return fail(SF_ERR_ARG, "cap_bullets must be 1..256");
  if (c->cap_portals < 1 || c->cap_portals > SF_MAX_PORTALS) return fail(SF_ERR_ARG, "cap_portals must be 1..9000");
  if (c->cap_chests < 0) return fail(SF_ERR_ARG, "cap_chests < 0");
  if (c->reseed_stride < 0) return fail(SF_ERR_ARG, "reseed_stride < 0");
  if (c->ind < 0 || c->ind >= c->n_agents || (c->ind != 0 && c->mode != SF_MODE_BATTLE))
    return fail(SF_ERR_ARG, "ind must be 0, or an agent slot of a Battle match");
  if (c->n_agents < 1 || c->n_agents > SF_MAX_AGENTS || c->n_agents > c->cap_humans)
    return fail(SF_ERR_ARG, "n_agents must be 1..min(16, cap_humans)");
  if (c->level < 1 || c->level > 10) return fail(SF_ERR_ARG, "level must be 1..10");
  if (c->mode < SF_MODE_SOLO || c->mode > SF_MODE_BATTLE) return fail(SF_ERR_ARG, "unknown mode");
  if (c->mode == SF_MODE_SQUAD && (c->cap_humans < 10 || c->rows < 5 || c->cols < 12))
    return fail(SF_ERR_ARG, "Squad needs cap_humans >= 10 and a map of at least 5 x 12");
  if ((c->mode == SF_MODE_SOLO || c->mode == SF_MODE_TIMER) && c->n_agents != 1)
    return fail(SF_ERR_ARG, "Solo/Timer have exactly one agent");
  if (c->n_agent_profiles != 0 && c->n_agent_profiles != c->n_agents)
    return fail(SF_ERR_ARG, "n_agent_profiles must be 0 or n_agents");
  // per-player records are what the players of a lock-step match exchange (gameplay.hpp:120-151): Battle mode only.  In
  // Solo / Timer / Squad every commanded human is built from `player` (Squad team mates from `npc`, gameplay.hpp:1878)
  if (c->n_agent_profiles != 0 && c->mode != SF_MODE_BATTLE)
    return fail(SF_ERR_ARG, "agent_profile[] is for SF_MODE_BATTLE (one record per player of the match)");
  const sf_profile *pr[2 + SF_MAX_AGENTS] = {&c->player, &c->npc};
  for (int i = 0; i < c->n_agent_profiles; ++i) pr[2 + i] = &c->agent_profile[i];
  for (int k = 0; k < 2 + c->n_agent_profiles; ++k) {
    for (int i = 0; i < 4; ++i)
      if (pr[k]->cons[i] < 0 || pr[k]->cons[i] > 65535 || pr[k]->throw_lvl_cnt[i][1] < 0 ||
          pr[k]->throw_lvl_cnt[i][1] > 65535)
        return fail(SF_ERR_ARG, "item counts must be 0..65535");
  }
  for (int i = 0; i < 4; ++i)
    if (c->items.thr[i][3] < 0 || c->items.thr[i][3] > 65535) return fail(SF_ERR_ARG, "item range out of 0..65535");
  for (int i = 0; i < 8; ++i)
    if (c->items.weapon[i][3] < 0 || c->items.weapon[i][3] > 65535) return fail(SF_ERR_ARG, "item range out of 0..65535");
  const int cells = c->floors * c->rows * c->cols;
  for (int i = 0; i < cells; ++i) {
    const char ch = c->map[i];
    if (ch != '#' && ch != '.' && ch != 'O' && ch != '^' && ch != 'v') return fail(SF_ERR_ARG, "map holds a char outside {# . O ^ v}");
    if ((ch == '^' || ch == 'v') && (!c->map_portal || c->map_portal[i] < 0 || c->map_portal[i] >= c->cap_portals))
      return fail(SF_ERR_ARG, "portal entrance without a valid exit number in map_portal");
  }
  return SF_OK;
}

// (mix64 / dg, the digest's hash, and the record decoders are in sf_state_records.hpp: the device compiles them too)

// whether a runtime has the state-record kernels (sf_state_device: k_state_init, k_state_records).  The HIP runtime has
// them; the wave emulator's runtime of tests/emu does not, and sf_state_device answers SF_ERR_STATE there
template <class R, class = void>
struct has_state_records : std::false_type {};
template <class R>
struct has_state_records<R, decltype((void)std::declval<R &>().launch_state_records(std::declval<const StateRec &>(), nullptr))>
    : std::true_type {};

// whether a runtime has the state-put kernels (sf_state_put_device: k_put_init / k_put_check / k_put_write).  The HIP runtime has
// them; the wave emulator's runtime of tests/emu does not, and sf_state_put_device / sf_load_arena answer SF_ERR_STATE there
template <class R, class = void>
struct has_state_put : std::false_type {};
template <class R>
struct has_state_put<R, decltype((void)std::declval<R &>().launch_state_put(std::declval<const StatePut &>(), nullptr))> : std::true_type {};

// whether a runtime has the episode log's own kernels: k_step's LOG instance (chosen through ep_log_on) and k_ep_late (the
// record behind k_reset and the split step's second half).  The HIP runtime has them; the wave emulator's runtime of
// tests/emu has one code path (Core::step_body picks the LOG form itself) and no k_ep_late, so there only k_step's
// records reach the ring
template <class R, class = void>
struct has_ep_late : std::false_type {};
template <class R>
struct has_ep_late<R, decltype((void)std::declval<R &>().launch_ep_late(std::declval<const Params &>(), true))> : std::true_type {};

// whether a runtime has the fixed-shape step kernels (k_step_fixed; sf_types.hpp FixedShapes): it then carries the index
// Env::create picked in `fixed_shape`.  Env::create is instantiated for every runtime, so a runtime without the member (one
// that runs generic instances only) needs this to build at all; the HIP runtime and tests/emu's CpuRT both have it
template <class R, class = void>
struct has_fixed_shapes : std::false_type {};
template <class R>
struct has_fixed_shapes<R, decltype((void)std::declval<R &>().fixed_shape)> : std::true_type {};

template <class RT>
struct Env {
  sf_config cfg;
  Params p;
  Tables tab;
  int NB = 1, cells = 0;
  bool was_reset = false;
  bool mid_step = false;  // between sf_step_begin and sf_step_end
  RT rt;
  // device buffers
  Tables *d_tab = nullptr;
  uint8_t *d_map_flags = nullptr;
  int16_t *d_map_pidx = nullptr;
  uint32_t *d_map_exits = nullptr;
  uint16_t *d_logt = nullptr;
  uint32_t *d_exptab = nullptr;
  uint64_t *d_tb = nullptr, *d_serial = nullptr;
  uint8_t *d_cmd = nullptr;
  uint32_t *d_perm = nullptr;  // k_step's launch order (k_rank): arenas by population, for long launches
  // episode log (sf_episode_log): the ring is tab.ep_ring; per arena the first episode not yet delivered by sf_episodes;
  // the collection's plan [3][A] (first output record, records delivered, first episode delivered); sf_episodes' staging
  int32_t *d_ep_cursor = nullptr, *d_ep_plan = nullptr, *d_ep_out = nullptr, *d_ep_counts = nullptr;
  size_t ep_out_records = 0;
  // command streams of logged games (sf_replay_load): rp.cmd is d_cmd; everything else is allocated by the load and
  // freed by sf_replay_load(NULL, NULL).  Null while nothing is loaded
  Replay rp = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int balance = 1;             // SF_BALANCE=0 switches the ordering off (A/B measurements)
  int rank_k_min = 8;          // launches of fewer steps run in arena order
  int rank_every = 100;        // steps between two orderings (SF_RANK_EVERY; measured: tools/experiments/README.md)
  int steps_since_rank = 1 << 30;  // the order is renewed every >= 100 steps (populations change by one every 20-25 steps)
  float *d_obs = nullptr;
  uint32_t *d_nzprev = nullptr;      // [A * n_agents][961] which floats of the delta-tracked buffer are non-zero
  const float *delta_ptr = nullptr;  // the buffer d_nzprev describes
  // host copies of the static map
  std::vector<uint8_t> map_flags;
  std::vector<int16_t> map_pidx;
  std::vector<uint32_t> map_exits;
  // host snapshot of the dynamic state (dump / digest)
  std::vector<uint32_t> s_hum, s_zom, s_bul, s_por, s_rng;
  std::vector<int32_t> s_scal, s_dmg;
  std::vector<int16_t> s_pidx;
  std::vector<uint8_t> s_flags;

  template <class T>
  int alloc(T *&ptr, size_t n) {
    ptr = (T *)rt.alloc(n * sizeof(T));
    return ptr ? SF_OK : fail(SF_ERR_MEMORY, "device allocation failed");
  }

  int create(const sf_config *c) {
    int rc = validate(c);
    if (rc) return rc;
    cfg = *c;
    rc = rt.init(cfg.device);
    if (rc) return rc;
    memset(&p, 0, sizeof p);
    memset(&tab, 0, sizeof tab);
    cells = cfg.floors * cfg.rows * cfg.cols;
    p.A = cfg.arenas, p.F = cfg.floors, p.N = cfg.rows, p.M = cfg.cols;
    p.cells = cells, p.cells_pad = (cells + 15) & ~15;
    p.bm_words = bm_words_for(p.cells_pad);
    p.H = cfg.cap_humans, p.Z = cfg.cap_zombies, p.B = cfg.cap_bullets, p.P = cfg.cap_portals, p.C = cfg.cap_chests;
    p.mode = cfg.mode, p.level = cfg.level, p.n_agents = cfg.n_agents, p.auto_reset = cfg.auto_reset;
    p.reseed = cfg.reseed_stride > 0 ? cfg.reseed_stride : cfg.arenas;
    p.timer_lim = cfg.level * (cfg.timer_frames_per_level > 0 ? cfg.timer_frames_per_level : 7500);
    p.squad_floor = cfg.floors > 2 ? 2 : cfg.floors - 1;
    p.ind = cfg.ind;
    // large pools (zombie / exit tables in LDS): one kernel instance, built for four bullet words (any B up to 256)
    NB = large_pools(p.Z, p.P) ? 4 : nb_for(p.B);
    {
      const char *e = getenv("SF_BALANCE");  // (A/B measurements: SF_BALANCE=0 switches k_rank's launch order off)
      balance = (e && e[0] == '0') ? 0 : 1;
      const char *r = getenv("SF_RANK_K_MIN");  // (A/B measurements: the shortest launch that is ordered)
      if (r) rank_k_min = atoi(r);
      const char *ev = getenv("SF_RANK_EVERY");
      if (ev && atoi(ev) > 0) rank_every = atoi(ev);
    }
    // the step kernel of a listed configuration (sf_types.hpp FixedShapes), chosen here once: every fixed field of `p`
    // equals the shape's.  SF_STEP_GENERIC=1 keeps the generic instance (A/B measurements, tests); while the episode log
    // is on the runtime launches the generic LOG instance whatever was chosen here
    if constexpr (has_fixed_shapes<RT>::value) {
      const char *g = getenv("SF_STEP_GENERIC");
      rt.fixed_shape = (g && g[0] == '1' && !g[1]) ? -1 : fixed_shape_of(p, FixedShapes{});
    }
    // tables: one shared player record (block 0) + npc (block 1), or one record per commanded human (blocks 0..15,
    // the account blobs of a lock-step match, gameplay.hpp:120-151) + npc (block 16)
    p.npc_block = cfg.n_agent_profiles > 0 ? MAX_PROFILE_BLOCKS - 1 : 1;
    p.ht_bytes = ht_bytes_for(p.npc_block + 1), p.lds_tab = lds_tab_for(p.npc_block + 1);
    if (lds_bytes_for(p.cells_pad, p.lds_tab, p.Z, p.P) > rt.max_lds())
      return fail(SF_ERR_ARG, large_pools(p.Z, p.P) ? "flag plane + zombie / exit tables (12 B per zombie slot, 4 B per exit) do not fit the CU's LDS: lower cap_zombies / cap_portals"
                                                   : "map does not fit the LDS flag plane");
    for (int i = 0; i < p.npc_block; ++i)
      derive_profile(cfg, (cfg.n_agent_profiles > 0 && i < cfg.n_agent_profiles) ? cfg.agent_profile[i] : cfg.player, tab.der[i]);
    derive_profile(cfg, cfg.npc, tab.der[p.npc_block]);
    tab.der[p.npc_block].mindamage_def += 15 * (cfg.level - 1);  // gen_human Character.hpp:882-886
    for (int i = 0; i <= p.npc_block; ++i) finish_derived(tab.der[i]);
    for (int i = 0; i < 4; ++i)
      for (int k = 0; k < 3; ++k) tab.cons_items[i][k] = cfg.items.cons[i][k];
    fill_hatab(tab, p.npc_block + 1);
    for (int i = 0; i < SF_MAX_AGENTS; ++i) {
      if (cfg.agent_team[i] < 0 || cfg.agent_team[i] > 255) return fail(SF_ERR_ARG, "agent_team must be 0..255");
      tab.teams[i] = cfg.agent_team[i];
    }
    {  // observation fast map (sf_obs.hpp obs_map_fast): constants of describe(), Custom.hpp:98,110-111,117-121
      float in[16];
      int n = 0;
      auto add = [&](float x) {
        if (x == 0.f) return;
        for (int i = 0; i < n; ++i)
          if (in[i] == x) return;
        if (n < 16) in[n++] = x;
      };
      add(1.0f), add((float)0.01), add((float)(20 / 1000.0)), add((float)(10 / 1000.0));
      for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 3; ++k) add((float)(cfg.items.cons[i][k] / 1000.0));
      tab.obs_n = n;
      for (int i = 0; i < n; ++i) {
        tab.obs_in[i] = in[i];
        tab.obs_out[i] = (float)pow((double)(fabsf(in[i]) / 10), 0.2);  // Custom.hpp:157, host libm
      }
      // the records of plain static cells, through the same describe() code the kernel runs for occupied cells
      Params hp = p;
      hp.tab = &tab;
      const ObsView hv(hp, 0);
      for (int c = 0; c < 8; ++c) {
        tab.class_mask[c] = 0u;
        for (int k = 0; k < 32; ++k) tab.class_rec[c][k] = 0.f;
        obs_cell_emit(hv, obs_class_flags(c), 0, 0u, 0, [&](int k, float x) {
          float y;
          if (!obs_map_fast(tab, x, y)) y = obs_map(x);
          tab.class_rec[c][k] = y;
          if (y != 0.f) tab.class_mask[c] |= 1u << k;
        });
      }
    }
    // static map: gameplay.hpp:1249-1274
    map_flags.assign((size_t)p.cells_pad, 0);
    map_pidx.assign((size_t)cells, -1);
    map_exits.assign((size_t)p.P, 0u);
    int next_exit = 0;
    for (int ci = 0; ci < cells; ++ci) {
      const char ch = cfg.map[ci];
      if (ch == '#')
        map_flags[ci] = SF_CELL_WALL;
      else if (ch == '^')
        map_flags[ci] = SF_CELL_PIN_UP, map_pidx[ci] = cfg.map_portal[ci];
      else if (ch == 'v')
        map_flags[ci] = SF_CELL_PIN_DN, map_pidx[ci] = cfg.map_portal[ci];
      else if (ch == 'O') {
        map_flags[ci] = SF_CELL_POUT;
        if (next_exit < p.P) {  // p_ind() of an empty table: scan order
          const int f = ci / (p.N * p.M), r = (ci / p.M) % p.N, cc = ci % p.M;
          map_exits[next_exit++] = pos_pack(f, r, cc) | PF_ACTIVE;
        }
      }
    }
    p.pw0 = zw_for(next_exit);
    cfg.map = nullptr, cfg.map_portal = nullptr;  // the caller's buffers are not kept
    // RNG tables: discrete logs / powers of the generator 3 of Z/65537*
    std::vector<uint16_t> logt(LOGT_ENTRIES, 0);
    std::vector<uint32_t> exptab(512);
    build_rng_tables(logt.data(), exptab.data());
    // device state
    const size_t A = (size_t)p.A;
    if ((rc = alloc(d_logt, (size_t)LOGT_ENTRIES)) || (rc = alloc(d_exptab, 512)) || (rc = alloc(d_tab, 1)) || (rc = alloc(d_map_flags, (size_t)p.cells_pad)) || (rc = alloc(d_map_pidx, (size_t)cells)) ||
        (rc = alloc(d_map_exits, (size_t)p.P)) || (rc = alloc(p.hum, HW_WORDS * A * p.H)) ||
        (rc = alloc(p.zom, ZW_WORDS * A * p.Z)) || (rc = alloc(p.bul, BW_WORDS * A * p.B)) ||
        (rc = alloc(p.por, A * p.P)) || (rc = alloc(p.rng, A * RNG_WORDS)) || (rc = alloc(p.rng2, A * RNG_WORDS)) || (rc = alloc(p.scal, A * SC_WORDS)) ||
        (rc = alloc(p.results, A * p.n_agents * 8)) || (rc = alloc(p.flags, A * (size_t)p.cells_pad)) ||
        (rc = alloc(p.aux_dmg, A * (size_t)cells)) || (rc = alloc(p.aux_pidx, A * (size_t)cells)) ||
        (rc = alloc(d_tb, A)) || (rc = alloc(d_serial, A)) || (rc = alloc(d_cmd, A * p.n_agents)))
      return rc;
    rt.h2d(d_tab, &tab, sizeof tab);
    rt.h2d(d_logt, logt.data(), logt.size() * sizeof(uint16_t));
    rt.h2d(d_exptab, exptab.data(), exptab.size() * sizeof(uint32_t));
    if ((rc = rt.sync())) return rc;  // the staging vectors above die with this scope
    rt.h2d(d_map_flags, map_flags.data(), map_flags.size());
    rt.h2d(d_map_pidx, map_pidx.data(), map_pidx.size() * sizeof(int16_t));
    rt.h2d(d_map_exits, map_exits.data(), map_exits.size() * sizeof(uint32_t));
    rt.zero(p.results, A * p.n_agents * 8 * sizeof(int32_t));
    rt.zero(p.scal, A * SC_WORDS * sizeof(int32_t));
    p.logt = d_logt, p.exptab = d_exptab;
    p.tab = d_tab, p.map_flags = d_map_flags, p.map_pidx = d_map_pidx, p.map_exits = d_map_exits;
    return rt.sync();
  }

  void destroy() {
    void *ptrs[] = {d_logt, d_exptab, d_tab, d_map_flags, d_map_pidx, d_map_exits, p.hum, p.zom, p.bul, p.por, p.rng, p.rng2, p.scal, p.results,
                    p.flags, p.aux_dmg, p.aux_pidx, d_tb, d_serial, d_cmd, d_obs, d_nzprev, d_perm, tab.ep_ring, d_ep_cursor, d_put_verdict, d_put_counters, d_put_status,
                    d_ep_plan, d_ep_out, d_ep_counts, (void *)rp.streams, (void *)rp.off, rp.status, rp.taken, d_amask};
    for (void *q : ptrs)
      if (q) rt.free(q);
    rt.shutdown();
  }

  int reset(const uint64_t *tb, const uint64_t *serial) {
    if (!tb || !serial) return fail(SF_ERR_ARG, "null seed array");
    rt.h2d(d_tb, tb, sizeof(uint64_t) * (size_t)p.A);
    rt.h2d(d_serial, serial, sizeof(uint64_t) * (size_t)p.A);
    rt.zero(p.results, (size_t)p.A * p.n_agents * 8 * sizeof(int32_t));
    if (tab.ep_ring) rt.zero(d_ep_cursor, (size_t)p.A * sizeof(int32_t));  // (k_ep_late empties the rings)
    if (rp.status) replay_rewind();
    int rc = rt.launch_reset(p, NB, d_tb, d_serial);
    if (rc || (rc = ep_late(true))) return rc;
    was_reset = true;
    mid_step = false;
    steps_since_rank = 1 << 30;
    return rt.sync();
  }

  // sf_reset_arenas: one stream-ordered launch that restarts the chosen arenas (sf_core.hpp reset_sel_body).  Nothing is
  // allocated, copied or waited for; the result latch, the episode-log rings and their cursors are left alone
  int reset_arenas(const sf_reset_sel *sel) {
    if (!sel) return fail(SF_ERR_ARG, "sf_reset_arenas: null sf_reset_sel");
    if (!was_reset) return fail(SF_ERR_STATE, "sf_reset_arenas before sf_reset");
    if (int rc = not_mid_step("sf_reset_arenas")) return rc;
    if (rp.status) return fail(SF_ERR_STATE, "sf_reset_arenas while a replay is loaded (sf_replay_load)");
    if (!sel->d_tb != !sel->d_serial) return fail(SF_ERR_ARG, "sf_reset_arenas: d_tb and d_serial must both be given or both be NULL");
    if (sel->d_mask && sel->mask_stride < 1) return fail(SF_ERR_ARG, "sf_reset_arenas: mask_stride must be at least 1");
    if (sel->max_steps < 0) return fail(SF_ERR_ARG, "sf_reset_arenas: max_steps must not be negative");
    const ResetSel r = {sel->d_mask, sel->d_mask ? sel->mask_stride : 0, sel->done_too, sel->max_steps, sel->d_tb, sel->d_serial, sel->d_selected};
    if (int rc = rt.launch_reset_sel(p, NB, r)) return rc;
    steps_since_rank = 1 << 30;  // the populations the launch order was built from are gone
    return SF_OK;
  }

  int step_host(const uint8_t *cmd) {
    if (!cmd) return fail(SF_ERR_ARG, "null command array");
    if (!was_reset) return fail(SF_ERR_STATE, "sf_step before sf_reset");
    if (mid_step) return fail(SF_ERR_STATE, "sf_step between sf_step_begin and sf_step_end");
    rt.h2d(d_cmd, cmd, (size_t)p.A * p.n_agents);
    return rt.launch_step(p, NB, d_cmd, 1);
  }
  int step_device(const uint8_t *d_cmds, int k) {
    if (!d_cmds || k < 1) return fail(SF_ERR_ARG, "bad command buffer / step count");
    if (!was_reset) return fail(SF_ERR_STATE, "sf_step_device before sf_reset");
    if (mid_step) return fail(SF_ERR_STATE, "sf_step_device between sf_step_begin and sf_step_end");
    // long launches: order the arenas by population first, so that the ones sharing a SIMD are of different loads (k_rank)
    Params q = p;
    // Below 1024 arenas every arena has a SIMD of its own (the chip has 1024): nothing to order.  Measured for 2048 ...
    // 16384 arenas, an arena count that is no multiple of 1024, and the maps whose flag plane stays in HBM
    // (profiles/r04b_rank_sweep.txt): +1 % (2048) ... +14 % (5000) on configs[2], +4 % on configs[4], -0.6 % on configs[3]
    // (every arena at its caps: nothing to order, k_rank's 7 us per 100 steps is what is left)
    if (balance && k >= rank_k_min && p.A >= 1024 && rt.can_rank()) {
      int rc;
      if (!d_perm && (rc = alloc(d_perm, (size_t)p.A))) return rc;
      if (steps_since_rank >= rank_every) {
        if ((rc = rt.launch_rank(p, d_perm))) return rc;
        steps_since_rank = 0;
      }
      steps_since_rank += k;
      q.perm = d_perm;
    }
    return rt.launch_step(q, NB, d_cmds, k);
  }
  // the iteration in two halves (the reference queries the agents of humans other than `ind` between them, G:988-999)
  int step_begin() {
    if (!was_reset) return fail(SF_ERR_STATE, "sf_step_begin before sf_reset");
    if (mid_step) return fail(SF_ERR_STATE, "sf_step_begin twice without sf_step_end");
    int rc = rt.launch_step_half(p, NB, d_cmd, 1);
    if (rc) return rc;
    mid_step = true;
    return SF_OK;
  }
  int step_end_device(const uint8_t *d_cmds) {
    if (!d_cmds) return fail(SF_ERR_ARG, "null command array");
    if (!mid_step) return fail(SF_ERR_STATE, "sf_step_end without sf_step_begin");
    int rc = rt.launch_step_half(p, NB, d_cmds, 2);
    if (rc || (rc = ep_late(false))) return rc;
    mid_step = false;
    return SF_OK;
  }
  int step_end_host(const uint8_t *cmd) {
    if (!cmd) return fail(SF_ERR_ARG, "null command array");
    if (!mid_step) return fail(SF_ERR_STATE, "sf_step_end without sf_step_begin");
    rt.h2d(d_cmd, cmd, (size_t)p.A * p.n_agents);
    return step_end_device(d_cmd);
  }
  // ---- replay of logged games: per-arena command streams fetched on the device (sf_replay_load / sf_replay_step) ----
  void replay_free() {
    void *old[] = {(void *)rp.streams, (void *)rp.off, rp.status, rp.taken};
    for (void *q : old)
      if (q) rt.free(q);
    rp = Replay{nullptr, nullptr, nullptr, nullptr, nullptr};
  }
  void replay_rewind() {  // every stream from its first line again, nothing taken yet
    rt.zero(rp.status, (size_t)p.A * RP_WORDS * sizeof(int32_t));
    rt.zero(rp.taken, (size_t)p.A * p.n_agents);
  }
  int replay_load(const uint8_t *streams, const int64_t *offsets) {
    if (int rc = not_mid_step("sf_replay_load")) return rc;
    int rc = rt.sync();  // launches still in flight may read the old streams
    if (rc) return rc;
    if (!streams && !offsets) {
      replay_free();
      return SF_OK;
    }
    if (!offsets) return fail(SF_ERR_ARG, "sf_replay_load: null offsets");
    if (p.auto_reset) return fail(SF_ERR_STATE, "sf_replay_load: a replay needs auto_reset == 0 (a logged game is one episode)");
    const size_t A = (size_t)p.A;
    if (offsets[0] < 0) return fail(SF_ERR_ARG, "sf_replay_load: negative offset");
    for (size_t a = 0; a < A; ++a)
      if (offsets[a + 1] < offsets[a]) return fail(SF_ERR_ARG, "sf_replay_load: offsets must not decrease");
    const int64_t total = offsets[A] - offsets[0];
    if (total >= ((int64_t)1 << 32)) return fail(SF_ERR_ARG, "sf_replay_load: 4 GiB of commands or more in one load");
    if (total > 0 && !streams) return fail(SF_ERR_ARG, "sf_replay_load: null streams");
    replay_free();
    std::vector<uint32_t> off(A + 1);
    for (size_t a = 0; a <= A; ++a) off[a] = (uint32_t)(offsets[a] - offsets[0]);
    uint8_t *d_streams = nullptr;
    uint32_t *d_off = nullptr;
    if ((rc = alloc(d_streams, (size_t)total)) || (rc = alloc(d_off, A + 1)) || (rc = alloc(rp.status, A * RP_WORDS)) ||
        (rc = alloc(rp.taken, A * p.n_agents))) {
      rp.streams = d_streams, rp.off = d_off;
      replay_free();
      return rc;
    }
    rp.streams = d_streams, rp.off = d_off, rp.cmd = d_cmd;
    if (total > 0) rt.h2d(d_streams, streams + offsets[0], (size_t)total);
    rt.h2d(d_off, off.data(), (A + 1) * sizeof(uint32_t));
    replay_rewind();
    return rt.sync();  // (the staging vector and the caller's buffer are free again)
  }
  int replay_loaded(const char *what) const {
    return rp.status ? SF_OK : fail(SF_ERR_STATE, std::string(what) + ": no command streams loaded (sf_replay_load)");
  }
  // one iteration of every arena, the commands taken from the streams on the device: loop-top check -> first half ->
  // fetch -> second half (+ k_ep_late where sf_step_end launches it); no host synchronisation
  int replay_step() {
    if (int rc = replay_loaded("sf_replay_step")) return rc;
    if (!was_reset) return fail(SF_ERR_STATE, "sf_replay_step before sf_reset");
    if (int rc = not_mid_step("sf_replay_step")) return rc;
    int rc;
    if ((rc = rt.launch_replay_fetch(p, rp, 0)) || (rc = rt.launch_step_half(p, NB, d_cmd, 1))) return rc;
    if (p.n_agents > 1 && (rc = rt.launch_replay_fetch(p, rp, 1))) return rc;  // (a lone player has no other lines)
    if ((rc = rt.launch_step_half(p, NB, d_cmd, 2))) return rc;
    return ep_late(false);
  }
  int replay_status_host(int32_t *out) {
    if (!out) return fail(SF_ERR_ARG, "null output buffer");
    if (int rc = replay_loaded("sf_replay_status")) return rc;
    rt.d2h(out, rp.status, (size_t)p.A * RP_WORDS * sizeof(int32_t));
    return rt.sync();
  }
  int replay_status_device(int32_t *d_out) {
    if (!d_out) return fail(SF_ERR_ARG, "null output buffer");
    if (int rc = replay_loaded("sf_replay_status_device")) return rc;
    rt.d2d(d_out, rp.status, (size_t)p.A * RP_WORDS * sizeof(int32_t));
    return SF_OK;
  }
  int replay_commands_device(uint8_t *d_out) {
    if (!d_out) return fail(SF_ERR_ARG, "null output buffer");
    if (int rc = replay_loaded("sf_replay_commands_device")) return rc;
    rt.d2d(d_out, rp.taken, (size_t)p.A * p.n_agents);
    return SF_OK;
  }

  int agent_alive_device(uint8_t *d_out) {
    if (!d_out) return fail(SF_ERR_ARG, "null output buffer");
    if (!was_reset) return fail(SF_ERR_STATE, "sf_agent_alive before sf_reset");
    return rt.launch_agent_alive(p, d_out);
  }
  int agent_alive_host(uint8_t *out) {
    if (!out) return fail(SF_ERR_ARG, "null output buffer");
    if (!was_reset) return fail(SF_ERR_STATE, "sf_agent_alive before sf_reset");
    // (d_cmd is free between calls: every step entry point uploads or receives its commands anew)
    int rc = rt.launch_agent_alive(p, d_cmd);
    if (rc) return rc;
    rt.d2h(out, d_cmd, (size_t)p.A * p.n_agents);
    return rt.sync();
  }

  int observe_device(float *d_out) {
    if (!d_out) return fail(SF_ERR_ARG, "null observation buffer");
    if (!was_reset) return fail(SF_ERR_STATE, "sf_observe before sf_reset");
    if (d_out == delta_ptr) delta_ptr = nullptr;  // a plain write: the non-zero map no longer describes this buffer
    return rt.launch_observe(p, NB, d_out, nullptr, 0);
  }
  int observe_sparse_device(uint32_t *d_keys, float *d_vals, uint32_t *d_counts, float *d_pov, int cap) {
    if (!d_keys || !d_vals || !d_counts || !d_pov) return fail(SF_ERR_ARG, "null buffer");
    if (cap < 1) return fail(SF_ERR_ARG, "sf_observe_sparse_device: cap must be positive");
    if (!was_reset) return fail(SF_ERR_STATE, "sf_observe before sf_reset");
    return rt.launch_observe_sparse(p, d_keys, d_vals, d_counts, d_pov, cap);
  }
  int observe_overflow_device(const uint32_t *d_counts, int cap, float *d_dense, float *d_pov) {
    if (!d_counts || !d_dense || !d_pov) return fail(SF_ERR_ARG, "null buffer");
    if (cap < 1) return fail(SF_ERR_ARG, "sf_observe_overflow_device: cap must be positive");
    if (!was_reset) return fail(SF_ERR_STATE, "sf_observe before sf_reset");
    if (d_dense == delta_ptr) delta_ptr = nullptr;
    return rt.launch_observe_overflow(p, d_counts, cap, d_dense, d_pov);
  }
  int observe_device_delta(float *d_out) {
    if (!d_out) return fail(SF_ERR_ARG, "null observation buffer");
    if (!was_reset) return fail(SF_ERR_STATE, "sf_observe before sf_reset");
    int rc;
    if (!d_nzprev && (rc = alloc(d_nzprev, (size_t)p.A * p.n_agents * 961))) return rc;
    const int mode = d_out == delta_ptr ? 2 : 1;  // 1: write everything and record the map; 2: write the differences
    delta_ptr = d_out;
    return rt.launch_observe(p, NB, d_out, d_nzprev, mode);
  }
  int observe_host(float *out) {
    if (!out) return fail(SF_ERR_ARG, "null observation buffer");
    const size_t n = (size_t)p.A * p.n_agents * SF_OBS_FLOATS;
    int rc;
    if (!d_obs && (rc = alloc(d_obs, n))) return rc;
    if ((rc = observe_device(d_obs))) return rc;
    rt.d2h(out, d_obs, n * sizeof(float));
    return rt.sync();
  }

  // between sf_step_begin and sf_step_end the episode-end bookkeeping is half done (the first half clears SC_ENDED): only
  // observe / dump / digest / agent_alive may be called there, as strikeforce.h says
  int not_mid_step(const char *what) const {
    return mid_step ? fail(SF_ERR_STATE, std::string(what) + " between sf_step_begin and sf_step_end") : SF_OK;
  }
  int results_host(int32_t *out) {
    if (!out) return fail(SF_ERR_ARG, "null results buffer");
    if (int rc = not_mid_step("sf_results")) return rc;
    rt.d2h(out, p.results, (size_t)p.A * p.n_agents * 8 * sizeof(int32_t));
    return rt.sync();
  }
  int results_device(int32_t *d_out) {
    if (!d_out) return fail(SF_ERR_ARG, "null results buffer");
    if (int rc = not_mid_step("sf_results_device")) return rc;
    rt.d2d(d_out, p.results, (size_t)p.A * p.n_agents * 8 * sizeof(int32_t));
    return SF_OK;
  }
  // ---- episode log ------------------------------------------------------------------------------
  size_t ep_ring_words() const { return (size_t)p.A * (size_t)tab.ep_depth * (size_t)ep_record_words(p.n_agents); }
  int episode_log(int depth) {
    if (depth < 0 || depth > 64 || (depth & (depth - 1)))
      return fail(SF_ERR_ARG, "sf_episode_log: depth must be 0 or a power of two in [1, 64]");
    if (int rc = not_mid_step("sf_episode_log")) return rc;
    const size_t A = (size_t)p.A, words = A * (size_t)depth * (size_t)ep_record_words(p.n_agents);
    if (words >= ((size_t)1 << 31)) return fail(SF_ERR_ARG, "sf_episode_log: ring of 2^31 words or more: lower depth");
    int rc = rt.sync();  // launches still in flight may write the old ring
    if (rc) return rc;
    auto release = [&] {
      void *old[] = {tab.ep_ring, d_ep_cursor, d_ep_plan, d_ep_out, d_ep_counts};
      for (void *q : old)
        if (q) rt.free(q);
      tab.ep_ring = nullptr, tab.ep_depth = 0;
      d_ep_cursor = d_ep_plan = d_ep_out = d_ep_counts = nullptr;
      ep_out_records = 0;
    };
    release();
    if (depth > 0) {
      if ((rc = alloc(tab.ep_ring, words)) || (rc = alloc(d_ep_cursor, A)) || (rc = alloc(d_ep_plan, 3 * A)) ||
          (rc = alloc(d_ep_counts, 3))) {
        release();  // (the device's Tables must not keep a freed ring: the log is off after a failure)
        rt.h2d(d_tab, &tab, sizeof tab);
        if constexpr (has_ep_late<RT>::value) rt.ep_log_on = false;
        rt.sync();
        return rc;
      }
      tab.ep_depth = depth;
      // every slot empty (episode -1); the cursors start at the episodes counted so far: only later ones are offered
      std::vector<uint32_t> fill(words, 0xffffffffu);
      std::vector<int32_t> sc(A * SC_WORDS), cur(A);
      rt.h2d(tab.ep_ring, fill.data(), words * sizeof(uint32_t));
      rt.d2h(sc.data(), p.scal, sc.size() * sizeof(int32_t));
      if ((rc = rt.sync())) return rc;
      for (size_t a = 0; a < A; ++a) cur[a] = sc[a * SC_WORDS + SC_EPISODES];
      rt.h2d(d_ep_cursor, cur.data(), A * sizeof(int32_t));
    }
    rt.h2d(d_tab, &tab, sizeof tab);
    if constexpr (has_ep_late<RT>::value) rt.ep_log_on = tab.ep_ring != nullptr;
    return rt.sync();  // (the staging vectors and `tab` stay untouched until the copies are done)
  }
  int ep_late(bool after_reset) {
    if (!tab.ep_ring) return SF_OK;
    if constexpr (has_ep_late<RT>::value) {
      return rt.launch_ep_late(p, after_reset);
    } else if (after_reset) {  // (the emulator's runtime: the rings are at least emptied)
      std::vector<uint32_t> fill(ep_ring_words(), 0xffffffffu);
      rt.h2d(tab.ep_ring, fill.data(), fill.size() * sizeof(uint32_t));
      return rt.sync();
    }
    return SF_OK;
  }
  int episode_log_state(const char *what) const {
    if (!tab.ep_ring) return fail(SF_ERR_STATE, std::string(what) + ": the episode log is off (sf_episode_log)");
    return not_mid_step(what);
  }
  int episodes_device(int32_t *d_out, int max_records, int32_t *d_counts) {
    if (int rc = episode_log_state("sf_episodes_device")) return rc;
    if (max_records < 0) return fail(SF_ERR_ARG, "sf_episodes_device: max_records must not be negative");
    if ((!d_out && max_records > 0) || !d_counts) return fail(SF_ERR_ARG, "null buffer");
    return rt.launch_episodes(p, tab.ep_ring, tab.ep_depth, d_ep_cursor, d_ep_plan, d_out, max_records, d_counts);
  }
  int episodes_host(int32_t *out, int max_records, int32_t *counts) {
    if (int rc = episode_log_state("sf_episodes")) return rc;
    if (max_records < 0) return fail(SF_ERR_ARG, "sf_episodes: max_records must not be negative");
    if ((!out && max_records > 0) || !counts) return fail(SF_ERR_ARG, "null buffer");
    const size_t rw = (size_t)ep_record_words(p.n_agents), cap = (size_t)p.A * (size_t)tab.ep_depth;
    const size_t n = (size_t)max_records < cap ? (size_t)max_records : cap;  // more than the ring holds is never written
    int rc;
    if (n > ep_out_records) {
      if ((rc = rt.sync())) return rc;
      if (d_ep_out) rt.free(d_ep_out), d_ep_out = nullptr, ep_out_records = 0;
      if ((rc = alloc(d_ep_out, n * rw))) return rc;
      ep_out_records = n;
    }
    if ((rc = episodes_device(d_ep_out, (int)n, d_ep_counts))) return rc;
    rt.d2h(counts, d_ep_counts, 3 * sizeof(int32_t));
    if ((rc = rt.sync())) return rc;
    if (counts[0] > 0) {
      rt.d2h(out, d_ep_out, (size_t)counts[0] * rw * sizeof(int32_t));
      rc = rt.sync();
    }
    return rc;
  }
  int episode_ring_host(int32_t *out) {
    if (!out) return fail(SF_ERR_ARG, "null output buffer");
    if (int rc = episode_log_state("sf_episode_ring")) return rc;
    rt.d2h(out, tab.ep_ring, ep_ring_words() * sizeof(int32_t));
    return rt.sync();
  }

  int done_host(uint8_t *out) {
    if (!out) return fail(SF_ERR_ARG, "null done buffer");
    if (int rc0 = not_mid_step("sf_done")) return rc0;
    std::vector<int32_t> sc((size_t)p.A * SC_WORDS);
    rt.d2h(sc.data(), p.scal, sc.size() * sizeof(int32_t));
    int rc = rt.sync();
    if (rc) return rc;
    for (int a = 0; a < p.A; ++a)
      out[a] = (uint8_t)(p.auto_reset ? sc[(size_t)a * SC_WORDS + SC_ENDED] : sc[(size_t)a * SC_WORDS + SC_DONE]);
    return SF_OK;
  }

  // generator draws of every arena's last step by phase: out[A][6] = zombie_action, update_bull (1st), human_action,
  // update_bull (2nd), the next loop top's spawns, everything else (0)
  int phase_draws_host(int32_t *out) {
    if (!out) return fail(SF_ERR_ARG, "null output buffer");
    if (!was_reset) return fail(SF_ERR_STATE, "sf_phase_draws before sf_reset");
    std::vector<int32_t> sc((size_t)p.A * SC_WORDS);
    rt.d2h(sc.data(), p.scal, sc.size() * sizeof(int32_t));
    int rc = rt.sync();
    if (rc) return rc;
    for (int a = 0; a < p.A; ++a) {
      const uint32_t w[3] = {(uint32_t)sc[(size_t)a * SC_WORDS + SC_PD01], (uint32_t)sc[(size_t)a * SC_WORDS + SC_PD23],
                             (uint32_t)sc[(size_t)a * SC_WORDS + SC_PD45]};
      int32_t *o = out + (size_t)a * 6;
      o[0] = (int32_t)(w[0] & 0xffffu), o[1] = (int32_t)(w[0] >> 16), o[2] = (int32_t)(w[1] & 0xffffu), o[3] = (int32_t)(w[1] >> 16);
      o[4] = (int32_t)(w[2] & 0xffffu), o[5] = (int32_t)(w[2] >> 16);
    }
    return SF_OK;
  }

  int done_device(uint8_t *d_out) {
    if (!d_out) return fail(SF_ERR_ARG, "null done buffer");
    if (int rc = not_mid_step("sf_done_device")) return rc;
    return rt.launch_done(p, d_out);
  }

  int done_view_device(const int32_t **d_words, int32_t *stride, int32_t *group) {
    if (!d_words || !stride || !group) return fail(SF_ERR_ARG, "null argument");
    *d_words = p.scal + (p.auto_reset ? SC_ENDED : SC_DONE), *stride = SC_WORDS, *group = p.n_agents;
    return SF_OK;
  }

  // ---- arena snapshots (sf_snapshot_*; the copy is sf_snapshot.hpp snapshot body, k_snapshot) ------------------------
  // row length and the environment's base of every piece of sf_types.hpp Snap, in the blob's order
  void snap_rows(uint32_t row[SNAP_PIECES], uint8_t *base[SNAP_PIECES]) const {
    const size_t A = (size_t)p.A;
    int i = 0;
    for (int f = 0; f < HW_WORDS; ++f, ++i) row[i] = 4u * (uint32_t)p.H, base[i] = (uint8_t *)(p.hum + (size_t)f * A * p.H);
    for (int f = 0; f < ZW_WORDS; ++f, ++i) row[i] = 4u * (uint32_t)p.Z, base[i] = (uint8_t *)(p.zom + (size_t)f * A * p.Z);
    for (int f = 0; f < BW_WORDS; ++f, ++i) row[i] = 4u * (uint32_t)p.B, base[i] = (uint8_t *)(p.bul + (size_t)f * A * p.B);
    row[i] = 4u * (uint32_t)p.P, base[i++] = (uint8_t *)p.por;
    row[i] = 4u * RNG_WORDS, base[i++] = (uint8_t *)p.rng;
    row[i] = 4u * RNG_WORDS, base[i++] = (uint8_t *)p.rng2;
    row[i] = (uint32_t)p.cells_pad, base[i++] = p.flags;
    row[i] = 4u * (uint32_t)cells, base[i++] = (uint8_t *)p.aux_dmg;
    row[i] = 2u * (uint32_t)cells, base[i++] = (uint8_t *)p.aux_pidx;
  }
  size_t snap_payload() const {  // bytes of one slot: every piece's row, then the scalar block
    uint32_t row[SNAP_PIECES];
    uint8_t *base[SNAP_PIECES];
    snap_rows(row, base);
    size_t n = (size_t)SC_WORDS * 4u;
    for (int i = 0; i < SNAP_PIECES; ++i) n += row[i];
    return n;
  }
  // Every configuration field that shapes or interprets an arena's state; not `arenas`, not `device`: a slot is one arena
  uint64_t snap_fingerprint() const {
    SnapHash h;
    const int32_t dims[] = {p.F, p.N, p.M, p.H, p.Z, p.B, p.P, p.C, p.mode, p.level, p.n_agents, p.ind, p.auto_reset,
                            p.reseed /* the effective stride */, p.timer_lim, cfg.timer_frames_per_level > 0 ? cfg.timer_frames_per_level : 7500,
                            cfg.n_agent_profiles};
    for (int32_t v : dims) h.word(v);
    for (int i = 0; i < SF_MAX_AGENTS; ++i) h.word(tab.teams[i]);
    auto words = [&](const void *q, size_t bytes) {
      const int32_t *w = static_cast<const int32_t *>(q);
      for (size_t i = 0; i < bytes / 4; ++i) h.word(w[i]);
    };
    words(&cfg.player, sizeof cfg.player), words(&cfg.npc, sizeof cfg.npc), words(&cfg.items, sizeof cfg.items);
    for (int i = 0; i < cfg.n_agent_profiles; ++i) words(&cfg.agent_profile[i], sizeof cfg.agent_profile[i]);
    h.bytes(map_flags.data(), (size_t)cells);
    for (int i = 0; i < cells; ++i) h.word(map_pidx[i]);
    for (int i = 0; i < p.P; ++i) h.word(map_exits[i]);
    return h.finish();
  }
  struct Snapshot {
    Env *owner = nullptr;
    int32_t slots = 0, parts = 1;
    uint8_t *block = nullptr;  // one allocation: every piece's [slots] rows, the scalar blocks, valid words, counters
    Snap k;                    // the launch's argument but for slot_of_arena
    size_t payload = 0;
  };
  int snapshot_slot_bytes(int64_t *device_bytes, int64_t *blob_bytes) const {
    if (!device_bytes && !blob_bytes) return fail(SF_ERR_ARG, "sf_snapshot_slot_bytes: null outputs");
    if (device_bytes) *device_bytes = (int64_t)snap_payload() + 4;  // (+ the valid word)
    if (blob_bytes) *blob_bytes = (int64_t)snap_payload() + SNAP_BLOB_HEADER;
    return SF_OK;
  }
  int snapshot_create(int32_t slots, Snapshot **out) {
    if (!out) return fail(SF_ERR_ARG, "sf_snapshot_create: null output handle");
    *out = nullptr;
    if (slots < 1) return fail(SF_ERR_ARG, "sf_snapshot_create: slots < 1");
    Snapshot *s = new (std::nothrow) Snapshot();
    if (!s) return fail(SF_ERR_MEMORY, "host allocation failed");
    s->owner = this, s->slots = slots, s->payload = snap_payload(), s->parts = snap_parts_for(s->payload);
    uint32_t row[SNAP_PIECES];
    uint8_t *base[SNAP_PIECES];
    snap_rows(row, base);
    size_t off[SNAP_PIECES], at = 0;
    for (int i = 0; i < SNAP_PIECES; ++i) off[i] = at, at = (at + (size_t)slots * row[i] + 255u) & ~(size_t)255u;
    const size_t scal_at = at, valid_at = scal_at + (size_t)slots * SC_WORDS * 4u, count_at = valid_at + (size_t)slots * 4u;
    const size_t total = count_at + SNAP_COUNTERS * 4u;
    if (int rc = alloc(s->block, total)) {
      delete s;
      return rc;
    }
    memset(&s->k, 0, sizeof s->k);
    for (int i = 0; i < SNAP_PIECES; ++i)
      s->k.piece[i] = SnapPiece{base[i], s->block + off[i], row[i], snap_part_bytes(row[i], s->parts), snap_width_for(row[i]), 0u};
    s->k.scal_env = p.scal, s->k.scal_snap = reinterpret_cast<int32_t *>(s->block + scal_at);
    s->k.valid = reinterpret_cast<int32_t *>(s->block + valid_at);
    s->k.counters = reinterpret_cast<uint32_t *>(s->block + count_at);
    s->k.A = p.A, s->k.slots = slots;
    rt.zero(s->block + valid_at, total - valid_at);  // every slot empty, the counters at 0
    if (int rc = rt.sync()) {
      rt.free(s->block);
      delete s;
      return rc;
    }
    *out = s;
    return SF_OK;
  }
  int snapshot_destroy(Snapshot *s) {
    if (!s) return SF_OK;
    int rc = rt.sync();  // launches still in flight may read or write the slots
    rt.free(s->block);
    delete s;
    return rc;
  }
  // one stream-ordered launch; nothing is allocated, copied or waited for
  int snapshot_copy(Snapshot *s, const int32_t *d_slot_of_arena, bool save) {
    const std::string who = save ? "sf_snapshot_save" : "sf_snapshot_load";
    if (!s || !d_slot_of_arena) return fail(SF_ERR_ARG, who + ": null argument");
    if (s->owner != this) return fail(SF_ERR_STATE, who + ": the snapshot was created for another environment");
    if (!was_reset) return fail(SF_ERR_STATE, who + " before sf_reset");
    if (int rc = not_mid_step(who.c_str())) return rc;
    if (rp.status) return fail(SF_ERR_STATE, who + " while a replay is loaded (sf_replay_load)");
    Snap k = s->k;
    k.slot_of_arena = d_slot_of_arena;
    if (int rc = rt.launch_snapshot(k, s->parts, save)) return rc;
    if (!save) steps_since_rank = 1 << 30;  // the populations the launch order was built from are gone
    return SF_OK;
  }
  int snapshot_status(Snapshot *s, int32_t out[4]) {
    if (!s || !out) return fail(SF_ERR_ARG, "sf_snapshot_status: null argument");
    rt.d2h(out, s->k.counters, SNAP_COUNTERS * sizeof(int32_t));
    rt.zero(s->k.counters, SNAP_COUNTERS * sizeof(int32_t));
    return rt.sync();
  }
  int snapshot_slot_check(const Snapshot *s, int32_t slot, const void *blob, int64_t bytes, const char *who) const {
    if (!s || !blob) return fail(SF_ERR_ARG, std::string(who) + ": null argument");
    if (slot < 0 || slot >= s->slots) return fail(SF_ERR_ARG, std::string(who) + ": slot out of range");
    if (bytes < SNAP_BLOB_HEADER + (int64_t)s->payload) return fail(SF_ERR_ARG, std::string(who) + ": " + snap_blob_message(SNAP_BLOB_SHORT));
    return SF_OK;
  }
  int snapshot_export(Snapshot *s, int32_t slot, void *blob, int64_t bytes) {
    if (int rc = snapshot_slot_check(s, slot, blob, bytes, "sf_snapshot_export")) return rc;
    int32_t valid = 0;
    rt.d2h(&valid, s->k.valid + slot, sizeof valid);
    if (int rc = rt.sync()) return rc;
    if (!valid) return fail(SF_ERR_STATE, "sf_snapshot_export: the slot was never saved or imported");
    uint8_t *out = static_cast<uint8_t *>(blob);
    snap_blob_header(out, s->payload, snap_fingerprint());
    out += SNAP_BLOB_HEADER;
    for (int i = 0; i < SNAP_PIECES; ++i) {
      const SnapPiece &pc = s->k.piece[i];
      rt.d2h(out, pc.snap + (size_t)slot * pc.row_bytes, pc.row_bytes);
      out += pc.row_bytes;
    }
    rt.d2h(out, s->k.scal_snap + (size_t)slot * SC_WORDS, SC_WORDS * 4u);
    return rt.sync();
  }
  int snapshot_import(Snapshot *s, int32_t slot, const void *blob, int64_t bytes) {
    if (!s || !blob) return fail(SF_ERR_ARG, "sf_snapshot_import: null argument");
    if (slot < 0 || slot >= s->slots) return fail(SF_ERR_ARG, "sf_snapshot_import: slot out of range");
    if (int v = snap_blob_check(blob, bytes, s->payload, snap_fingerprint()))
      return fail(SF_ERR_ARG, std::string("sf_snapshot_import: ") + snap_blob_message(v));
    const uint8_t *in = static_cast<const uint8_t *>(blob) + SNAP_BLOB_HEADER;
    for (int i = 0; i < SNAP_PIECES; ++i) {
      const SnapPiece &pc = s->k.piece[i];
      rt.h2d(pc.snap + (size_t)slot * pc.row_bytes, in, pc.row_bytes);
      in += pc.row_bytes;
    }
    rt.h2d(s->k.scal_snap + (size_t)slot * SC_WORDS, in, SC_WORDS * 4u);
    const int32_t one = 1;
    rt.h2d(s->k.valid + slot, &one, sizeof one);
    return rt.sync();  // (the caller's buffer and `one` are free again)
  }

  // ---- per-step signals (sf_signals_*; the per-agent body is sf_signals.hpp signals_agent, k_signals) -----------------
  struct SignalsObj {
    Env *owner = nullptr;
    int32_t *base = nullptr;                // [A * n_agents][SIG_BASE_WORDS], all zero = no baseline yet
    unsigned long long *counters = nullptr; // [SIG_COUNTERS]
  };
  int signals_create(SignalsObj **out) {
    if (!out) return fail(SF_ERR_ARG, "sf_signals_create: null output handle");
    *out = nullptr;
    SignalsObj *s = new (std::nothrow) SignalsObj();
    if (!s) return fail(SF_ERR_MEMORY, "host allocation failed");
    s->owner = this;
    const size_t words = (size_t)p.A * (size_t)p.n_agents * SIG_BASE_WORDS;
    int rc;
    if ((rc = alloc(s->base, words)) || (rc = alloc(s->counters, (size_t)SIG_COUNTERS))) {
      if (s->base) rt.free(s->base);
      delete s;
      return rc;
    }
    rt.zero(s->base, words * sizeof(int32_t));
    rt.zero(s->counters, SIG_COUNTERS * sizeof(unsigned long long));
    if ((rc = rt.sync())) {
      rt.free(s->base), rt.free(s->counters);
      delete s;
      return rc;
    }
    *out = s;
    return SF_OK;
  }
  int signals_destroy(SignalsObj *s) {
    if (!s) return SF_OK;
    int rc = rt.sync();  // launches still in flight may read or write the baseline
    rt.free(s->base), rt.free(s->counters);
    delete s;
    return rc;
  }
  // one stream-ordered launch; nothing is allocated, copied or waited for
  int signals_step(SignalsObj *s, const sf_signals_io *io) {
    if (!s || !io) return fail(SF_ERR_ARG, "sf_signals_step: null argument");
    if (s->owner != this) return fail(SF_ERR_STATE, "sf_signals_step: the signals object was created for another environment");
    if (!was_reset) return fail(SF_ERR_STATE, "sf_signals_step before sf_reset");
    if (int rc = not_mid_step("sf_signals_step")) return rc;
    Signals k;
    memset(&k, 0, sizeof k);
    k.hum = p.hum, k.scal = p.scal, k.results = p.results;
    k.base = s->base, k.counters = s->counters;
    k.vitals = io->d_vitals, k.delta = io->d_delta, k.reward = io->d_reward, k.rebase = io->d_rebase;
    k.A = p.A, k.H = p.H, k.n_agents = p.n_agents;
    if (io->d_reward) k.w = io->weights;
    return rt.launch_signals(k);
  }
  int signals_status(SignalsObj *s, int64_t out[4]) {
    if (!s || !out) return fail(SF_ERR_ARG, "sf_signals_status: null argument");
    unsigned long long c[SIG_COUNTERS] = {0, 0, 0, 0};
    rt.d2h(c, s->counters, sizeof c);
    rt.zero(s->counters, sizeof c);
    if (int rc = rt.sync()) return rc;
    for (int i = 0; i < SIG_COUNTERS; ++i) out[i] = (int64_t)c[i];
    return SF_OK;
  }

  // ---- action masks (sf_action_mask_*; the wavefront's body is sf_action_mask.hpp ActionMaskCore, k_action_mask) -------
  // one stream-ordered launch; nothing is allocated, copied or waited for.  No not_mid_step(): the state is stored between
  // the halves of a step too
  int action_mask_device(const sf_action_mask_io *io) {
    if (!io) return fail(SF_ERR_ARG, "sf_action_mask_device: null argument");
    if (!was_reset) return fail(SF_ERR_STATE, "sf_action_mask_device before sf_reset");
    if (!io->d_commands && !io->d_actions && !io->action_string) return fail(SF_ERR_ARG, "sf_action_mask_device: no output");
    if (!io->d_actions != !io->action_string)
      return fail(SF_ERR_ARG, "sf_action_mask_device: d_actions and action_string must both be given or both be NULL");
    ActionMask k;
    memset(&k, 0, sizeof k);
    memset(k.action_bit, 31, sizeof k.action_bit);
    if (io->action_string) {
      const size_t n = strnlen(io->action_string, 33);
      if (n < 1 || n > 32) return fail(SF_ERR_ARG, "sf_action_mask_device: action_string must hold 1..32 characters");
      for (size_t j = 0; j < n; ++j) {
        const char *at = strchr(SF_COMMANDS, io->action_string[j]);
        if (!at) return fail(SF_ERR_ARG, "sf_action_mask_device: action_string holds a character that is not in SF_COMMANDS");
        k.action_bit[j] = (uint8_t)(at - SF_COMMANDS);
      }
      k.n_actions = (int32_t)n;
    }
    k.hum = p.hum, k.zom = p.zom, k.bul = p.bul, k.por = p.por, k.scal = p.scal, k.flags = p.flags, k.tab = p.tab;
    k.commands = io->d_commands, k.actions = io->d_actions;
    k.A = p.A, k.F = p.F, k.N = p.N, k.M = p.M, k.cells_pad = p.cells_pad, k.H = p.H, k.Z = p.Z, k.B = p.B, k.P = p.P;
    k.n_agents = p.n_agents, k.npc_block = p.npc_block;
    return rt.launch_action_mask(k);
  }
  // the command words through the host: the launch into a buffer of the environment's own (allocated by the first call)
  uint32_t *d_amask = nullptr;
  int action_mask_host(uint32_t *out) {
    if (!out) return fail(SF_ERR_ARG, "sf_action_mask: null output buffer");
    if (!was_reset) return fail(SF_ERR_STATE, "sf_action_mask before sf_reset");
    const size_t n = (size_t)p.A * (size_t)p.n_agents;
    if (!d_amask)
      if (int rc = alloc(d_amask, n)) return rc;
    sf_action_mask_io io = {d_amask, nullptr, nullptr};
    if (int rc = action_mask_device(&io)) return rc;
    rt.d2h(out, d_amask, n * sizeof(uint32_t));
    return rt.sync();
  }

  // ---- recording of games as command streams (sf_record_*; the lane functions are sf_record.hpp's, k_record*) ----------
  struct Recorder {
    Env *owner = nullptr;
    Record k;                       // the kernels' struct: the environment's buffers and the recorder's own
    int64_t *counts = nullptr;      // [SF_RECORD_COUNT_WORDS]: sf_record_collect's staging
    uint8_t *out_bytes = nullptr;   // ... and its outputs, grown on demand
    int32_t *out_games = nullptr;
    int64_t out_bytes_n = 0, out_games_n = 0;
  };
  void record_release(Recorder *r) {
    void *ptrs[] = {r->k.bytes, r->k.games, r->k.st, r->k.plan, r->counts, r->out_bytes, r->out_games};
    for (void *q : ptrs)
      if (q) rt.free(q);
    delete r;
  }
  int record_create(int64_t bytes_per_arena, int32_t games_per_arena, Recorder **out) {
    if (!out) return fail(SF_ERR_ARG, "sf_record_create: null output handle");
    *out = nullptr;
    if (bytes_per_arena < p.n_agents || bytes_per_arena >= ((int64_t)1 << 31))
      return fail(SF_ERR_ARG, "sf_record_create: bytes_per_arena must be at least n_agents (one iteration) and below 2^31");
    if (games_per_arena < 1 || (int64_t)games_per_arena * RG_WORDS >= ((int64_t)1 << 31))
      return fail(SF_ERR_ARG, "sf_record_create: games_per_arena must be at least 1");
    Recorder *r = new (std::nothrow) Recorder();
    if (!r) return fail(SF_ERR_MEMORY, "host allocation failed");
    r->owner = this;
    memset(&r->k, 0, sizeof r->k);
    const size_t A = (size_t)p.A;
    int rc;
    if ((rc = alloc(r->k.bytes, A * (size_t)bytes_per_arena)) || (rc = alloc(r->k.games, A * (size_t)games_per_arena * RG_WORDS)) ||
        (rc = alloc(r->k.st, A * RC_WORDS)) || (rc = alloc(r->k.plan, A * RPL_WORDS)) || (rc = alloc(r->counts, (size_t)SF_RECORD_COUNT_WORDS))) {
      record_release(r);
      return rc;
    }
    r->k.hum = p.hum, r->k.scal = p.scal, r->k.results = p.results;
    r->k.A = p.A, r->k.H = p.H, r->k.n_agents = p.n_agents, r->k.ind = p.ind, r->k.auto_reset = p.auto_reset;
    r->k.G = games_per_arena, r->k.bpa = (int32_t)bytes_per_arena;
    rt.zero(r->k.st, A * RC_WORDS * sizeof(int32_t));  // no open game, empty region and index
    if ((rc = rt.sync())) {
      record_release(r);
      return rc;
    }
    *out = r;
    return SF_OK;
  }
  int record_destroy(Recorder *r) {
    if (!r) return SF_OK;
    int rc = rt.sync();  // launches still in flight may read or write the regions
    record_release(r);
    return rc;
  }
  int record_usable(const Recorder *r, const char *who) const {
    if (!r) return fail(SF_ERR_ARG, std::string(who) + ": null recorder");
    if (r->owner != this) return fail(SF_ERR_ARG, std::string(who) + ": the recorder was created for another environment");
    if (!was_reset) return fail(SF_ERR_STATE, std::string(who) + " before sf_reset");
    if (int rc = not_mid_step(who)) return rc;
    if (rp.status) return fail(SF_ERR_STATE, std::string(who) + " while a replay is loaded (sf_replay_load)");
    return SF_OK;
  }
  // one iteration of every arena as the split step plays it, with the record launches around its halves: loop top ->
  // first half -> the other players' lines -> second half (+ k_ep_late where sf_step_end launches it) -> closing; no host
  // synchronisation
  int record_step(Recorder *r, const uint8_t *d_cmds) {
    if (int rc = record_usable(r, "sf_record_step")) return rc;
    if (!d_cmds) return fail(SF_ERR_ARG, "sf_record_step: null command array");
    Record k = r->k;
    k.cmd = d_cmds;
    int rc;
    if ((rc = rt.launch_record(k, 0)) || (rc = rt.launch_step_half(p, NB, d_cmds, 1))) return rc;
    if (p.n_agents > 1 && (rc = rt.launch_record(k, 1))) return rc;  // (a lone player has no other lines)
    if ((rc = rt.launch_step_half(p, NB, d_cmds, 2)) || (rc = ep_late(false))) return rc;
    return rt.launch_record(k, 2);
  }
  int record_flush(Recorder *r) {
    if (int rc = record_usable(r, "sf_record_flush")) return rc;
    return rt.launch_record(r->k, 3);
  }
  int record_collect_device(Recorder *r, uint8_t *d_bytes, int64_t max_bytes, int32_t *d_games, int32_t max_games, int64_t *d_counts) {
    if (!r || !d_bytes || !d_games || !d_counts) return fail(SF_ERR_ARG, "sf_record_collect_device: null argument");
    if (max_bytes < 1 || max_games < 1) return fail(SF_ERR_ARG, "sf_record_collect_device: max_bytes and max_games must be positive");
    return rt.launch_record_collect(r->k, d_bytes, max_bytes, d_games, max_games, d_counts);
  }
  int record_collect_host(Recorder *r, uint8_t *bytes, int64_t max_bytes, int32_t *games, int32_t max_games, int64_t *counts) {
    if (!r || !bytes || !games || !counts) return fail(SF_ERR_ARG, "sf_record_collect: null argument");
    if (max_bytes < 1 || max_games < 1) return fail(SF_ERR_ARG, "sf_record_collect: max_bytes and max_games must be positive");
    int rc;
    if (r->out_bytes_n < max_bytes) {
      if ((rc = rt.sync())) return rc;
      if (r->out_bytes) rt.free(r->out_bytes);
      r->out_bytes = nullptr, r->out_bytes_n = 0;
      if ((rc = alloc(r->out_bytes, (size_t)max_bytes))) return rc;
      r->out_bytes_n = max_bytes;
    }
    if (r->out_games_n < max_games) {
      if ((rc = rt.sync())) return rc;
      if (r->out_games) rt.free(r->out_games);
      r->out_games = nullptr, r->out_games_n = 0;
      if ((rc = alloc(r->out_games, (size_t)max_games * RG_WORDS))) return rc;
      r->out_games_n = max_games;
    }
    if ((rc = rt.launch_record_collect(r->k, r->out_bytes, max_bytes, r->out_games, max_games, r->counts))) return rc;
    rt.d2h(counts, r->counts, SF_RECORD_COUNT_WORDS * sizeof(int64_t));
    if ((rc = rt.sync())) return rc;
    if (counts[0] > 0) rt.d2h(games, r->out_games, (size_t)counts[0] * RG_WORDS * sizeof(int32_t));
    if (counts[1] > 0) rt.d2h(bytes, r->out_bytes, (size_t)counts[1]);
    return rt.sync();
  }

  // ---- parity tooling ----------------------------------------------------------------------------
  int snapshot() {
    const size_t A = (size_t)p.A;
    s_hum.resize(HW_WORDS * A * p.H), s_zom.resize(ZW_WORDS * A * p.Z), s_bul.resize(BW_WORDS * A * p.B);
    s_por.resize(A * p.P), s_rng.resize(A * RNG_WORDS), s_scal.resize(A * SC_WORDS);
    s_flags.resize(A * (size_t)p.cells_pad), s_dmg.resize(A * (size_t)cells), s_pidx.resize(A * (size_t)cells);
    rt.d2h(s_hum.data(), p.hum, s_hum.size() * 4), rt.d2h(s_zom.data(), p.zom, s_zom.size() * 4);
    rt.d2h(s_bul.data(), p.bul, s_bul.size() * 4), rt.d2h(s_por.data(), p.por, s_por.size() * 4);
    rt.d2h(s_rng.data(), p.rng, s_rng.size() * 4), rt.d2h(s_scal.data(), p.scal, s_scal.size() * 4);
    rt.d2h(s_flags.data(), p.flags, s_flags.size()), rt.d2h(s_dmg.data(), p.aux_dmg, s_dmg.size() * 4);
    rt.d2h(s_pidx.data(), p.aux_pidx, s_pidx.size() * 2);
    return rt.sync();
  }

  // decode arena `a` of the snapshot into the canonical records of strikeforce.h: the per-record text is
  // sf_state_records.hpp's, which k_state_records compiles too
  void decode(int a, sf_arena_hdr *hdr, sf_human_rec *hs, sf_zombie_rec *zs, sf_bullet_rec *bs, sf_portal_rec *ps,
              uint8_t *cf, int32_t *cd, int32_t *cp) const {
    const size_t A = (size_t)p.A;
    if (hdr) {
      int32_t hw[REC_HDR_WORDS];
      for (int j = 0; j < REC_HDR_WORDS; ++j) hw[j] = hdr_word(j, &s_scal[(size_t)a * SC_WORDS], &s_rng[(size_t)a * RNG_WORDS]);
      memcpy(hdr, hw, sizeof *hdr);
    }
    if (hs)
      for (int i = 0; i < p.H; ++i) {
        uint32_t w[HW_WORDS];
        for (int f = 0; f < HW_WORDS; ++f) w[f] = s_hum[((size_t)f * A + a) * p.H + i];
        decode_human(w, hs[i]);
      }
    if (zs)
      for (int i = 0; i < p.Z; ++i) {
        auto w = [&](int f) { return s_zom[((size_t)f * A + a) * p.Z + i]; };
        decode_zombie(w(ZW_POS), w(ZW_HP), w(ZW_MINDAMAGE), zs[i]);
      }
    if (bs)
      for (int i = 0; i < p.B; ++i) {
        auto w = [&](int f) { return s_bul[((size_t)f * A + a) * p.B + i]; };
        decode_bullet(w(BW_A), w(BW_DAMAGE), w(BW_B), w(BW_C), bs[i]);
      }
    if (ps)
      for (int i = 0; i < p.P; ++i) decode_portal(s_por[(size_t)a * p.P + i], ps[i]);
    for (int ci = 0; ci < cells; ++ci) {
      const uint8_t fl = s_flags[(size_t)a * p.cells_pad + ci];
      if (cf) cf[ci] = fl;
      if (cd) cd[ci] = cell_dmg_of(fl, s_dmg[(size_t)a * cells + ci]);
      if (cp) cp[ci] = cell_portal_of(fl, s_pidx[(size_t)a * cells + ci], map_pidx[ci]);
    }
  }

  uint64_t digest_of(const sf_arena_hdr &hdr, const sf_human_rec *hs, const sf_zombie_rec *zs, const sf_bullet_rec *bs,
                     const sf_portal_rec *ps, const uint8_t *cf, const int32_t *cd, const int32_t *cp) const {
    uint64_t d = 0;
    int32_t hw[REC_HDR_WORDS];
    memcpy(hw, &hdr, sizeof hdr);
    for (int j = 0; j < DG_HDR_TERMS; ++j) d += digest_hdr_term(j, hw);
    for (int i = 0; i < p.H; ++i) d += digest_human(i, hs[i]);
    for (int i = 0; i < p.Z; ++i) d += digest_zombie(i, zs[i]);
    for (int i = 0; i < p.B; ++i) d += digest_bullet(i, bs[i]);
    for (int i = 0; i < p.P; ++i) d += digest_portal(i, ps[i]);
    for (int ci = 0; ci < cells; ++ci) d += digest_cell(ci, cf[ci], cd[ci], cp[ci]);
    return d;
  }

  int dump_arena(int a, sf_arena_hdr *hdr, sf_human_rec *hs, sf_zombie_rec *zs, sf_bullet_rec *bs, sf_portal_rec *ps,
                 uint8_t *cf, int32_t *cd, int32_t *cp) {
    if (a < 0 || a >= p.A) return fail(SF_ERR_ARG, "arena out of range");
    if (!was_reset) return fail(SF_ERR_STATE, "dump before reset");
    int rc = snapshot();
    if (rc) return rc;
    decode(a, hdr, hs, zs, bs, ps, cf, cd, cp);
    return SF_OK;
  }

  int state_digest(uint64_t *out) {
    if (!out) return fail(SF_ERR_ARG, "null digest buffer");
    if (!was_reset) return fail(SF_ERR_STATE, "digest before reset");
    int rc = snapshot();
    if (rc) return rc;
    sf_arena_hdr hdr;
    std::vector<sf_human_rec> hs(p.H);
    std::vector<sf_zombie_rec> zs(p.Z);
    std::vector<sf_bullet_rec> bs(p.B);
    std::vector<sf_portal_rec> ps(p.P);
    std::vector<uint8_t> cf(cells);
    std::vector<int32_t> cd(cells), cp(cells);
    for (int a = 0; a < p.A; ++a) {
      decode(a, &hdr, hs.data(), zs.data(), bs.data(), ps.data(), cf.data(), cd.data(), cp.data());
      out[a] = digest_of(hdr, hs.data(), zs.data(), bs.data(), ps.data(), cf.data(), cd.data(), cp.data());
    }
    return SF_OK;
  }

  // ---- sf_state_put_device / sf_load_arena (the lane functions are sf_state_put.hpp's, k_put_*) ---------------------
  // the rows' verdicts and extents and the call's counters: allocated by the first call that needs more rows than any
  // call before it, as sf_rollout_gae's array is
  int32_t *d_put_verdict = nullptr;
  unsigned long long *d_put_counters = nullptr;
  int32_t put_rows = 0;
  // the kernels' struct and the bytes each of the eleven buffers must hold (the row map, the eight parts, the two outputs)
  int put_fill(const sf_state_put_io *io, StatePut &k, int64_t bytes[11]) {
    const std::string who = "sf_state_put_device";
    if (!io) return fail(SF_ERR_ARG, who + ": null argument");
    if (!was_reset) return fail(SF_ERR_STATE, who + " before sf_reset");
    if (int rc = not_mid_step(who.c_str())) return rc;
    if (rp.status) return fail(SF_ERR_STATE, who + " while a replay is loaded (sf_replay_load)");
    if (!io->d_row_of_arena) return fail(SF_ERR_ARG, who + ": null d_row_of_arena");
    if (io->rows < 1) return fail(SF_ERR_ARG, who + ": rows must be at least 1");
    if (io->humans < 0 || io->humans > p.H || io->zombies < 0 || io->zombies > p.Z || io->bullets < 0 || io->bullets > p.B ||
        io->portals < 0 || io->portals > p.P)
      return fail(SF_ERR_ARG, who + ": humans / zombies / bullets / portals must be 0 .. the configuration's cap");
    const int ncell = (io->d_cell_flags ? 1 : 0) + (io->d_cell_dmg ? 1 : 0) + (io->d_cell_portal ? 1 : 0);
    if (ncell != 0 && ncell != 3) return fail(SF_ERR_ARG, who + ": d_cell_flags, d_cell_dmg and d_cell_portal must be given all or none");
    if (!io->d_hdr && !io->d_humans && !io->d_zombies && !io->d_bullets && !io->d_portals && !ncell)
      return fail(SF_ERR_ARG, who + ": every part is NULL");
    memset(&k, 0, sizeof k);
    k.hum = p.hum, k.zom = p.zom, k.bul = p.bul, k.por = p.por, k.rng = p.rng, k.rng2 = p.rng2, k.scal = p.scal, k.flags = p.flags;
    k.aux_dmg = p.aux_dmg, k.aux_pidx = p.aux_pidx, k.map_pidx = p.map_pidx;
    k.A = p.A, k.cells_pad = p.cells_pad;
    k.c = PutCfg{p.F, p.N, p.M, p.H, p.Z, p.B, p.P, cells, p.mode, p.n_agents, p.ind, p.npc_block, p.auto_reset, p.reseed};
    k.io = *io;
    const int64_t R = io->rows, C = cells;
    const int64_t b[11] = {(int64_t)p.A * 4, R * (int64_t)sizeof(sf_arena_hdr), R * io->humans * (int64_t)sizeof(sf_human_rec),
                           R * io->zombies * (int64_t)sizeof(sf_zombie_rec), R * io->bullets * (int64_t)sizeof(sf_bullet_rec),
                           R * io->portals * (int64_t)sizeof(sf_portal_rec), R * C, R * C * 4, R * C * 4, (int64_t)p.A * 4,
                           (int64_t)p.A * p.n_agents};
    memcpy(bytes, b, sizeof b);
    return SF_OK;
  }
  // three stream-ordered launches; nothing is copied or waited for, and nothing allocated once the verdict rows suffice
  int state_put_device(const sf_state_put_io *io) {
    if constexpr (has_state_put<RT>::value) {
      StatePut k;
      int64_t bytes[11];
      if (int rc = put_fill(io, k, bytes)) return rc;
      if (int rc = rt.check_state_put(k, bytes)) return rc;
      if (!d_put_counters) {
        if (int rc = alloc(d_put_counters, (size_t)PUT_COUNTERS)) return rc;
        rt.zero(d_put_counters, PUT_COUNTERS * sizeof(unsigned long long));
      }
      if (io->rows > put_rows) {
        if (d_put_verdict) {
          if (int rc = rt.sync()) return rc;  // an earlier call's launches may still read the rows
          rt.free(d_put_verdict);
          d_put_verdict = nullptr, put_rows = 0;
        }
        if (int rc = alloc(d_put_verdict, (size_t)io->rows * PUT_ROW_WORDS)) return rc;
        put_rows = io->rows;
      }
      k.verdict = d_put_verdict, k.counters = d_put_counters;
      if (int rc = rt.launch_state_put(k, bytes)) return rc;
      steps_since_rank = 1 << 30;  // the populations the launch order was built from are gone
      return SF_OK;
    } else {
      (void)io;
      return fail(SF_ERR_STATE, "sf_state_put_device: this runtime has no state-put kernels");
    }
  }
  int state_put_status(int64_t out[4]) {
    if (!out) return fail(SF_ERR_ARG, "sf_state_put_status: null argument");
    for (int j = 0; j < 4; ++j) out[j] = 0;
    if (!d_put_counters) return rt.sync();
    unsigned long long c[PUT_COUNTERS];
    rt.d2h(c, d_put_counters, sizeof c);
    rt.zero(d_put_counters, sizeof c);
    if (int rc = rt.sync()) return rc;
    for (int j = 0; j < 4; ++j) out[j] = (int64_t)c[j];
    return SF_OK;
  }
  // the host mirror of sf_dump_arena: one row of whole pools through staging memory of the call's own, then the device path
  int load_arena(int a, const sf_arena_hdr *hdr, const sf_human_rec *hs, const sf_zombie_rec *zs, const sf_bullet_rec *bs,
                 const sf_portal_rec *ps, const uint8_t *cf, const int32_t *cd, const int32_t *cp) {
    if constexpr (has_state_put<RT>::value) {
      if (a < 0 || a >= p.A) return fail(SF_ERR_ARG, "sf_load_arena: arena out of range");
      const size_t C = (size_t)cells;
      const struct { const void *src; size_t bytes; } part[8] = {
          {hdr, sizeof(sf_arena_hdr)}, {hs, p.H * sizeof(sf_human_rec)}, {zs, p.Z * sizeof(sf_zombie_rec)}, {bs, p.B * sizeof(sf_bullet_rec)},
          {ps, p.P * sizeof(sf_portal_rec)}, {cf, C}, {cd, C * 4}, {cp, C * 4}};
      size_t off[8], at = ((size_t)p.A * 4 + 255u) & ~(size_t)255u;  // the row map first
      for (int j = 0; j < 8; ++j) off[j] = at, at = (at + (part[j].src ? part[j].bytes : 0) + 255u) & ~(size_t)255u;
      uint8_t *stage = nullptr;
      if (int rc = alloc(stage, at)) return rc;
      std::vector<int32_t> map((size_t)p.A, -1);
      map[(size_t)a] = 0;
      rt.h2d(stage, map.data(), map.size() * 4);
      for (int j = 0; j < 8; ++j)
        if (part[j].src) rt.h2d(stage + off[j], part[j].src, part[j].bytes);
      auto at_or_null = [&](int j) -> const void * { return part[j].src ? stage + off[j] : nullptr; };
      sf_state_put_io io;
      memset(&io, 0, sizeof io);
      io.d_row_of_arena = reinterpret_cast<const int32_t *>(stage), io.rows = 1;
      io.humans = p.H, io.zombies = p.Z, io.bullets = p.B, io.portals = p.P;
      io.d_hdr = static_cast<const sf_arena_hdr *>(at_or_null(0)), io.d_humans = static_cast<const sf_human_rec *>(at_or_null(1));
      io.d_zombies = static_cast<const sf_zombie_rec *>(at_or_null(2)), io.d_bullets = static_cast<const sf_bullet_rec *>(at_or_null(3));
      io.d_portals = static_cast<const sf_portal_rec *>(at_or_null(4)), io.d_cell_flags = static_cast<const uint8_t *>(at_or_null(5));
      io.d_cell_dmg = static_cast<const int32_t *>(at_or_null(6)), io.d_cell_portal = static_cast<const int32_t *>(at_or_null(7));
      int rc = rt.sync();
      int32_t status = 0;
      if (!rc) rc = state_put_one(io, a, &status);
      rt.free(stage);
      if (rc) return rc;
      if (status != 0) {
        static const char *names[] = {"the header", "a human", "a zombie", "a bullet", "an exit", "a cell"};
        std::string why;
        for (int j = 0; j < 6; ++j)
          if (status & (1 << j)) why += std::string(why.empty() ? "" : ", ") + names[j];
        return fail(SF_ERR_ARG, "sf_load_arena: refused, a field out of range in " + why);
      }
      return SF_OK;
    } else {
      (void)a, (void)hdr, (void)hs, (void)zs, (void)bs, (void)ps, (void)cf, (void)cd, (void)cp;
      return fail(SF_ERR_STATE, "sf_load_arena: this runtime has no state-put kernels");
    }
  }
  // sf_load_arena's launch, with a status array of the library's own of which arena a's word is read back
  int32_t *d_put_status = nullptr;
  int state_put_one(sf_state_put_io &io, int a, int32_t *status) {
    if (!d_put_status)
      if (int rc = alloc(d_put_status, (size_t)p.A)) return rc;
    io.d_status = d_put_status;
    if (int rc = state_put_device(&io)) return rc;
    rt.d2h(status, d_put_status + a, 4);
    return rt.sync();
  }

  // sf_state_device / sf_state_bytes: the kernel's struct and the bytes each of the ten outputs must hold
  int state_fill(const sf_state_io *io, StateRec &k, int64_t bytes[10], const char *who) const {
    if (!io) return fail(SF_ERR_ARG, std::string(who) + ": null argument");
    if (!was_reset) return fail(SF_ERR_STATE, std::string(who) + " before sf_reset");
    if (io->d_arena_ids && io->rows < 1) return fail(SF_ERR_ARG, std::string(who) + ": rows must be at least 1 with d_arena_ids");
    if (io->humans < 0 || io->humans > p.H || io->zombies < 0 || io->zombies > p.Z || io->bullets < 0 || io->bullets > p.B ||
        io->portals < 0 || io->portals > p.P)
      return fail(SF_ERR_ARG, std::string(who) + ": humans / zombies / bullets / portals must be 0 .. the configuration's cap");
    memset(&k, 0, sizeof k);
    k.hum = p.hum, k.zom = p.zom, k.bul = p.bul, k.por = p.por, k.rng = p.rng, k.scal = p.scal, k.flags = p.flags;
    k.aux_dmg = p.aux_dmg, k.aux_pidx = p.aux_pidx, k.map_pidx = p.map_pidx;
    k.A = p.A, k.H = p.H, k.Z = p.Z, k.B = p.B, k.P = p.P, k.cells = cells, k.cells_pad = p.cells_pad;
    k.io = *io;
    if (!io->d_arena_ids) k.io.rows = p.A;
    k.parts = state_parts_for(state_units(k).total(), k.io.rows);
    const int64_t R = k.io.rows, C = cells;
    const int64_t b[10] = {R * (int64_t)sizeof(sf_arena_hdr), R * io->humans * (int64_t)sizeof(sf_human_rec),
                           R * io->zombies * (int64_t)sizeof(sf_zombie_rec), R * io->bullets * (int64_t)sizeof(sf_bullet_rec),
                           R * io->portals * (int64_t)sizeof(sf_portal_rec), R * C, R * C * 4, R * C * 4,
                           R * SF_STATE_COUNT_WORDS * 4, R * 8};
    memcpy(bytes, b, sizeof b);
    return SF_OK;
  }
  int state_bytes(const sf_state_io *io, int64_t *out) const {
    if (!out) return fail(SF_ERR_ARG, "sf_state_bytes: null argument");
    StateRec k;
    return state_fill(io, k, out, "sf_state_bytes");
  }
  // one or two stream-ordered launches; nothing is allocated, copied or waited for
  int state_device(const sf_state_io *io) {
    StateRec k;
    int64_t bytes[10];
    if (int rc = state_fill(io, k, bytes, "sf_state_device")) return rc;
    if constexpr (has_state_records<RT>::value) {
      return rt.launch_state_records(k, bytes);
    } else {
      return fail(SF_ERR_STATE, "sf_state_device: this runtime has no state-record kernels");
    }
  }
};

// Items/ text files and character/*.txt of the reference as defaults (values: SURVEY.md Appendix B)
inline void config_defaults(sf_config *c) {
  memset(c, 0, sizeof *c);
  c->abi_version = SF_ABI_VERSION;
  static const int cons[4][3] = {{20, 0, 20}, {0, 200, 10}, {20, 50, 10}, {20, 400, 20}};
  static const int thr[4][4] = {{-15, 50, -20, 100}, {-20, 75, -200, 100}, {-30, 100, -80, 100}, {-35, 125, -80, 100}};
  static const int wp[8][4] = {{-25, 150, -50, 1},  {-40, 175, -60, 1},   {-40, 200, -70, 1},   {-45, 225, -80, 1},
                               {-50, 150, -55, 100}, {-50, 175, -65, 100}, {-50, 200, -75, 100}, {-50, 225, -85, 100}};
  memcpy(c->items.cons, cons, sizeof cons), memcpy(c->items.thr, thr, sizeof thr), memcpy(c->items.weapon, wp, sizeof wp);
  sf_profile human = {1000, 100, 1000, 1, 1, 1, 1000, 0, 0, 0, 0, {0, 0, 0, 0}, {{1, 0}, {1, 0}, {1, 0}, {1, 0}}, {0}, 1};
  sf_profile enemy = {1000, 100, 1000000, 1, 1, 1, 1000, 1, 1, 1, 1, {1, 1, 1, 1}, {{1, 1}, {1, 1}, {1, 1}, {1, 1}},
                      {1, 1, 1, 1, 1, 1, 1, 1}, 1};
  c->player = human, c->npc = enemy;
  c->cap_chests = 9000, c->cap_portals = 16, c->level = 1, c->n_agents = 1, c->arenas = 1;
  for (int i = 0; i < SF_MAX_AGENTS; ++i) c->agent_team[i] = i + 1;
}

}  // namespace sf
