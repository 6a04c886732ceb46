/*
 * strikeforce.h — C-ABI of the MI355X-native batched StrikeForce arena simulator.
 *
 * This is the drop-in boundary for the reference's per-tick gameplay path.  The reference
 * (bistoyek21-ric/StrikeForce, all paths relative to StrikeForce-client/) has no FFI: its
 * boundary is compile-time — `class Agent` (bots/bot-0.5/Agent.hpp:178,217,239,266;
 * minimal form bots/bot-0/Agent.hpp:27-37) plus three declared-only members of
 * `struct gameplay`: `char bot(Human&) const` (gameplay.hpp:477), `void prepare(Human&)`
 * (gameplay.hpp:481), `void view() const` (gameplay.hpp:485).  Each entry point below names
 * the reference code it replaces.  `include/sf_agent_adapter.hpp` rebuilds the reference's
 * Agent contract on top of these calls so that existing Agent.hpp bots drop in.
 *
 * Plain C, plain pointers and sizes, no torch / HIP types in any signature.
 * All integer game state is bit-identical to the reference CPU loop under the same
 * (tb, serial) seed; see DESIGN.md for the documented deviations (frame clock for Timer).
 */
#ifndef STRIKEFORCE_H
#define STRIKEFORCE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SF_ABI_VERSION 2

/* Observation geometry — bots/bot-0.5/Custom.hpp:137-159 (32 channels, 31x31 window). */
#define SF_OBS_CHANNELS 32
#define SF_OBS_WINDOW 31
#define SF_OBS_FLOATS (SF_OBS_CHANNELS * SF_OBS_WINDOW * SF_OBS_WINDOW) /* 30752 */

/* Slot caps supported by the device kernels.  Humans: one wavefront lane each; bullets: four registers per lane.
 * Zombies and portal exits: the reference's own pool size (gameplay.hpp:37 `Z = 9000`, :51-53 `portal[B]`); pools of
 * more than 64 slots live in the arena's LDS (12 B per zombie slot, 4 B per exit) and sf_create refuses a
 * configuration whose flag plane and tables do not fit the CU's 160 KiB.  A whole Timer game of the reference on its
 * shipped maps holds at most 22 humans and 25 bullets at once (level 10, 37 500 steps), but 564 zombies and ~290 exits. */
#define SF_MAX_HUMANS 64
#define SF_MAX_ZOMBIES 9000
#define SF_MAX_BULLETS 256
#define SF_MAX_PORTALS 9000
#define SF_MAX_AGENTS 16
#define SF_MAX_COORD 1024 /* random.hpp:62 — _rand() is 10 bits, so rand()%N never reaches 1024 */

/* Game modes — gameplay.hpp:1530,1567,1604,1642,1660 (`mode` strings). */
enum { SF_MODE_SOLO = 0, SF_MODE_TIMER = 1, SF_MODE_SQUAD = 2, SF_MODE_BATTLE = 3 };

/* Episode outcome codes written to sf_results()[..][7] — gameplay.hpp:1102-1229 (check_end). */
enum { SF_RUNNING = 0, SF_DIED = 1, SF_WON = 2, SF_TIME_LOST = 3, SF_TIME_WON = 4, SF_QUIT = 5,
       SF_SAMPLE_END = 6 /* not an outcome of check_end: a replayed arena whose command stream ran out (sf_replay_step) */ };

/* Status codes (API misuse only; gameplay "failures" stay silent no-ops as in the reference). */
enum {
  SF_OK = 0,
  SF_ERR_ARG = -1,      /* null pointer / out-of-range config */
  SF_ERR_DEVICE = -2,   /* no HIP device or a HIP runtime error: the product never falls back to CPU */
  SF_ERR_MEMORY = -3,
  SF_ERR_STATE = -4     /* call order (e.g. step before reset) */
};

/* Cell flag byte (one per cell per arena) — the persistent subset of `node::s`
 * (gameplay.hpp:237-241).  s[0] human / s[1] zombie / s[2] bullet are derived from the
 * entity tables; s[8] corpse and s[9] hit-flash are render-only. */
enum {
  SF_CELL_WALL = 0x01,    /* s[3]  '#' */
  SF_CELL_TEMP = 0x02,    /* s[10] destructible (player-built) */
  SF_CELL_PIN_UP = 0x04,  /* s[5]  '^' portal entrance */
  SF_CELL_PIN_DN = 0x08,  /* s[6]  'v' portal entrance */
  SF_CELL_POUT = 0x10,    /* s[7]  'O' portal exit */
  SF_CELL_CHEST = 0x20,   /* s[4]  '?' */
  SF_CELL_CONS_SHIFT = 6  /* bits 6-7: consumable type of the chest (gameplay.hpp:539) */
};

/* A character record in the reference's 33-token text format minus the name
 * (Character.hpp:650-709 `Human::build`; files character/human.txt, character/human_enemy.txt,
 * accounts/game/<user>/info, <user>.txt). */
typedef struct sf_profile {
  int32_t def_hp, mindamage_def, def_stamina;
  int32_t level_solo, level_timer, level_squad;
  int32_t money;
  int32_t rate_solo, rate_timer, rate_squad, rate;
  int32_t cons[4];          /* owned consumables */
  int32_t throw_lvl_cnt[4][2]; /* (level, count) per throwable */
  int32_t weapon_lvl[8];    /* 0 = not owned */
  int32_t backpack_lvl;
} sf_profile;

/* Item stat tables — Item.hpp:69-74,113-118,149-154; files Items/{cons,throw,w}*.txt. */
typedef struct sf_items {
  int32_t cons[4][3];   /* stamina, Hp, effect */
  int32_t thr[4][4];    /* stamina, damage, effect, range */
  int32_t weapon[8][4]; /* stamina, damage, effect, range (level 0; each owned level +50/-50) */
} sf_items;

typedef struct sf_config {
  int32_t abi_version;      /* SF_ABI_VERSION */
  int32_t arenas;           /* independent worlds on this device */
  int32_t floors, rows, cols; /* gameplay.hpp:37 F, N, M */
  int32_t cap_humans, cap_zombies, cap_bullets, cap_portals, cap_chests; /* gameplay.hpp:37 H, Z, B, (B), C */
  int32_t mode;             /* SF_MODE_* */
  int32_t level;            /* 1..10, gameplay.hpp:459 L */
  int32_t n_agents;         /* humans commanded through sf_step */
  int32_t ind;              /* which of them is the reference's `ind` (gameplay.hpp:39): the player whose death ends the
                               episode and whose team the kill/loot counters follow.  0 except in lock-step Battle matches,
                               where the match server assigns it (server.cpp:243-246) */
  int32_t agent_team[SF_MAX_AGENTS]; /* BATTLE mode teams (server.cpp:239-246); ignored otherwise */
  int32_t auto_reset;       /* re-seed (tb += reseed_stride) and restart an arena when its episode ends */
  int32_t reseed_stride;    /* 0 -> arenas; multi-GPU runs pass the global arena count so that shards never reuse a seed */
  int32_t timer_frames_per_level; /* frame clock replacing time(0) in Timer mode (gameplay.hpp:1145-1146); 0 -> 7500 */
  int32_t device;           /* HIP device ordinal */
  const char *map;          /* floors*rows*cols chars from {# . O ^ v}; map/floor*.txt, gameplay.hpp:1249-1274 */
  const int16_t *map_portal;/* per cell: exit number for '^'/'v' cells, ignored elsewhere */
  sf_profile player;        /* profile of every commanded human (Character::me) */
  sf_profile npc;           /* character/human_enemy.txt */
  sf_items items;
  /* ABI 2: one character record per commanded human, as the players of a lock-step match exchange them before the
   * first tick (give_info / get_info gameplay.hpp:120-151; blob = Human::log_file / scan_file Character.hpp:570-648).
   * 0: every commanded human is built from `player`; n_agents: commanded human i is built from agent_profile[i]
   * (and `player` is unused).  NPC humans always come from `npc`. */
  int32_t n_agent_profiles;
  sf_profile agent_profile[SF_MAX_AGENTS];
} sf_config;

typedef struct sf_env sf_env; /* opaque; one per GPU */

/* ---- state dump (parity tests; not on the hot path) ---------------------------------------- */
typedef struct sf_arena_hdr {
  int64_t frame, kills, teams_kills, loot, chests; /* gameplay.hpp:461 */
  int64_t jomle;            /* random.hpp:29 */
  int64_t tb, serial;       /* seed of the running episode */
  int64_t steps;            /* loop iterations completed in this episode */
  int64_t episodes;         /* episodes completed by this arena since sf_create */
  int32_t rng[18];          /* random.hpp:31 `random[]` */
  int32_t done, outcome;
} sf_arena_hdr;

typedef struct sf_human_rec {
  int32_t alive, remote, rnpc, profile; /* mh / remote bitsets gameplay.hpp:55; profile 0 player, 1 npc */
  int32_t f, r, c, way, team;
  int32_t hp, stamina, mindamage;
  int32_t kills, damage, effect;         /* Character.hpp:294 */
  int32_t vec, ind;                      /* Backpack selection Character.hpp:65 */
  int32_t cons[4], throw_cnt[4];
  int32_t blocks, portals, portal_ind;
} sf_human_rec;

typedef struct sf_zombie_rec {
  int32_t alive, f, r, c, hp, mindamage, super_;
} sf_zombie_rec;

typedef struct sf_bullet_rec {
  int32_t alive, f, r, c, way, traveled, damage, effect, range, owner /* human slot + 1, 0 = none */,
      ref /* 1 if the cell's bullet pointer designates this bullet (gameplay.hpp:814-816,1087-1089) */;
} sf_bullet_rec;

typedef struct sf_portal_rec {
  int32_t active, f, r, c;
} sf_portal_rec;

/* ---- lifecycle ----------------------------------------------------------------------------- */

/* Replaces: compile-time dims gameplay.hpp:37, download_items() Item.hpp:179-188, make_p()
 * random.hpp:33-40, Human::build Character.hpp:650-709.  Allocates all device state. */
int sf_create(const sf_config *cfg, sf_env **out);
int sf_destroy(sf_env *env);

/* Fills `cfg` with the reference's shipped tables (Items/ text files, character/human.txt as player,
 * character/human_enemy.txt as npc) and zeroes everything else. */
void sf_config_defaults(sf_config *cfg);

/* Replaces gameplay::setup() + load_data() (gameplay.hpp:1231-1277,1741-1925) for every arena:
 * reset slots, rebuild the map, Random::_srand(tb[a], serial[a]) (random.hpp:64-76; the libc
 * srand/rand derivation of `serial` at gameplay.hpp:1745-1746 is bypassed), place players per mode,
 * then run the first loop-top (spawns at frame 1, gameplay.hpp:1441-1450).
 * tb/serial: host arrays of `arenas` entries. */
int sf_reset(sf_env *env, const uint64_t *tb, const uint64_t *serial);

/* ---- restart of chosen arenas, on the device ------------------------------------------------------------------
 * The reference starts each new game with a fresh setup() and a new `tb` (gameplay.hpp:1231-1277, :1233) whenever the
 * player starts one, whatever any other game is doing.  sf_reset_arenas does that for the arenas a selection names and
 * leaves every other arena alone: no word of any buffer of an arena that is not chosen is written.
 * An arena is chosen if its mask flag is set, or (done_too) its game has ended (sf_arena_hdr.done == 1), or (max_steps >
 * 0) its game is still running and has sf_arena_hdr.steps >= max_steps.  A chosen arena ends up as sf_reset with that
 * (tb, serial) would have left it — setup() + load_data() + _srand + ++frame + the first loop top; done 0, sf_done 0;
 * with auto_reset the warm-up of the episode after it armed at the new tb + reseed_stride — except that
 *   - sf_arena_hdr.episodes keeps counting (it stays "episodes since the last whole sf_reset"), and
 *   - the arena's result latch (sf_results), episode-log ring and log cursor are not touched: undelivered records survive.
 * The game that was cut is abandoned: it is no episode, it is not logged and no counter moves.  A caller who wants the cut
 * game's record ends it one tick earlier with the reference's own quit command '_' (gameplay.hpp:696, 874-877, 941-954;
 * here the player's Hp drops to 0 and check_end ends the game, outcome SF_DIED): that game ends as an episode, is latched
 * and logged, and done_too then restarts it.
 * The restart is reported through d_selected, not through the done flags: a caller that lets sf_policy_predict_sparse read
 * the flags in place (sf_done_view_device) must pass d_selected to sf_policy_reset_memory for arenas restarted this way.
 * The call is one kernel launch in stream order on the environment's stream: no allocation, no copy, no host
 * synchronisation; the struct travels in the kernel arguments (it may be a temporary).
 * SF_ERR_STATE: before the first sf_reset, between sf_step_begin and sf_step_end, while a replay is loaded.  SF_ERR_ARG:
 * exactly one of d_tb / d_serial NULL, mask_stride < 1 with a mask, max_steps < 0, or a non-NULL pointer that is not
 * device memory of the environment's device, is not aligned (d_tb / d_serial: 8 bytes) or whose extent — d_mask:
 * (arenas - 1) * mask_stride + 1 bytes, the others as below — reaches past its allocation; nothing is launched then. */
typedef struct sf_reset_sel {
  const uint8_t *d_mask;    /* device; arena a is chosen if d_mask[a * mask_stride] != 0.  NULL: nobody by mask */
  int32_t mask_stride;      /* bytes between two arenas' flags: 1, or n_agents to pass sf_done_device's output as it is */
  int32_t done_too;         /* != 0: also every arena whose game has ended (done == 1) */
  int32_t max_steps;        /* > 0: also every arena whose running game has sf_arena_hdr.steps >= max_steps */
  const uint64_t *d_tb;     /* device, [arenas]; entries of arenas not chosen are not read */
  const uint64_t *d_serial; /* both NULL: the next seed by auto_reset's own rule, tb + reseed_stride, serial kept */
  uint8_t *d_selected;      /* optional out, device, [arenas][n_agents]: 1 for every agent of a restarted arena, else 0 —
                               the layout sf_policy_reset_memory and sf_rollout_record take */
} sf_reset_sel;
int sf_reset_arenas(sf_env *env, const sf_reset_sel *sel);

/* ---- save, restore and fork arenas mid-game, on the device ------------------------------------------------------
 * The reference can return to an earlier moment of a game in one way only: replaying its logged commands from tick 0
 * (gameplay.hpp:968-986; here sf_replay_*).  A snapshot keeps `slots` arena states in device memory of its own; save copies
 * arenas into slots, load copies slots into arenas, and many arenas may load one slot: that is the fork.
 * A slot carries the arena's rows of the human, zombie, bullet and exit tables, both generators (the running one and the
 * next episode's being warmed under auto_reset), the whole scalar block (frame, counters, seeds, done / ended flags, the
 * phase draws), the cell flags and the two per-cell side tables: everything sf_state_digest, sf_dump_arena, sf_phase_draws,
 * sf_done* and the next step read.  A slot does NOT carry, and a load does not touch:
 *   - sf_arena_hdr.episodes of the destination, which keeps counting as after sf_reset_arenas;
 *   - the result latch (sf_results);
 *   - the episode-log ring and its cursor: undelivered records survive and the log's ordinals stay monotonic;
 *   - the cursors of a loaded replay, rollout buffers, and the memory of any network (sf_policy_memory_rows moves that).
 * Every other scalar comes from the slot as it is, the done / ended flags and the seed included: a save taken between a step
 * and the next predict resumes with the same restart flags, and a loaded arena's later auto_reset restarts follow the
 * SOURCE's seed sequence.  Forks are therefore twins until their commands differ, and the episode log's "tb is unique
 * across shards" no longer holds for them: tell forks apart by arena, not by seed.
 * d_slot_of_arena: device int32 [arenas].  -1: the arena takes no part — no word of it is written (load), and no word of
 * a slot nobody names is written (save).  An index outside [-1, slots), and a load from a slot that was never saved or
 * imported, are skipped with the state left as it was and counted (sf_snapshot_status); such an index never becomes an
 * address.  Two arenas saving into one slot in one call is a caller error whose only guarantee is memory safety.
 * Save and load are one kernel launch each, in stream order on the environment's stream: no allocation, no copy, no host
 * synchronisation.  create, destroy, status, export and import synchronise.  Destroy a snapshot before its environment.
 * SF_ERR_STATE: before the first sf_reset, between sf_step_begin and sf_step_end, while a replay is loaded, a snapshot used
 * with an environment other than the one it was created for, an export of an empty slot.  SF_ERR_ARG: null handles,
 * slots < 1, a slot out of range (export / import), a d_slot_of_arena that is not device memory of the environment's
 * device, is not 4-byte aligned or is shorter than `arenas` entries; nothing is launched then.
 * A blob (export / import, the checkpoint path) is a 24-byte header — magic, layout version, payload length, a 64-bit
 * fingerprint of the configuration — and the slot's bytes.  The fingerprint covers every sf_config field that shapes or
 * interprets the state (dimensions, caps, mode, level, n_agents, ind, teams, auto_reset, the effective reseed stride,
 * timer_frames_per_level, map and portal table, profiles, items) and leaves out `arenas` and `device`: a blob may go into
 * an environment with another arena count (set reseed_stride explicitly then: its default is the arena count).
 * sf_snapshot_import refuses a blob that is too short or has another magic, version, length or fingerprint with
 * SF_ERR_ARG and touches nothing. */
typedef struct sf_snapshot sf_snapshot;       /* opaque; device memory for `slots` arena states of env's configuration */
int sf_snapshot_create(sf_env *env, int32_t slots, sf_snapshot **out);
int sf_snapshot_destroy(sf_snapshot *s);
int sf_snapshot_slot_bytes(sf_env *env, int64_t *device_bytes, int64_t *blob_bytes);   /* to budget before create */
/* arena a -> slot d_slot_of_arena[a]; -1: arena not saved.  Device int32 [arenas]. */
int sf_snapshot_save(sf_env *env, sf_snapshot *s, const int32_t *d_slot_of_arena);
/* arena a <- slot d_slot_of_arena[a]; -1: arena untouched.  Many arenas may name one slot: that is the fork. */
int sf_snapshot_load(sf_env *env, sf_snapshot *s, const int32_t *d_slot_of_arena);
int sf_snapshot_status(sf_snapshot *s, int32_t out_host[4]);   /* skipped: empty slot, index out of range, 0, 0; clears */
int sf_snapshot_export(sf_snapshot *s, int32_t slot, void *blob_host, int64_t bytes);        /* one slot -> host blob */
int sf_snapshot_import(sf_snapshot *s, int32_t slot, const void *blob_host, int64_t bytes);  /* host blob -> one slot */

/* ---- per-step game signals and a shaped reward, on the device ------------------------------------------------------
 * The reference keeps `kills / teams_kills / loot` per game (gameplay.hpp:461, counted up in hit_human and hit_zombie,
 * gameplay.hpp:588-593,625-629) and `kills / damage / effect` per human (Character.hpp:294) up to date every tick; Hp,
 * stamina and mindamage are the human's own fields (Character.hpp:286-293).  sf_results shows them once per game and
 * sf_dump_arena one arena at a time through the host.  sf_signals_step hands them out behind any step, for every (arena,
 * agent) at once and without leaving the device: their levels now (vitals), their change since the previous call on the
 * same signals object (delta), and a weighted sum of that change (reward) in the layout sf_rollout_step.d_reward takes.
 * It writes nothing of the environment: digests, dumps and the next step are as without the call.
 * A signals object belongs to one environment and owns, in device memory, one baseline per (arena, agent): the arena's
 * seed, step count, episode count and done flag, the agent's six counters (sf_results' words 0..5) and whether it was
 * present, all as of the previous call.
 *
 * Vitals, SF_VITALS_WORDS x int32:  flags, hp, stamina, mindamage, kills, damage, effect, floor, row, col, way, team |
 *   arena kills, teams_kills, loot, steps.  Words 1..11 are what sf_dump_arena shows for human slot g (Character.hpp:
 *   286-294, position and way gameplay.hpp:43) and are 0 for an agent that is not present; words 12..15 are
 *   sf_arena_hdr's (gameplay.hpp:461).
 * Delta, SF_DELTA_WORDS x int32:  flags, d kills, d teams_kills, d loot, d damage, d effect, d Hp, outcome — the
 *   differences of sf_results' words 0..5; outcome is an SF_* outcome code, 0 unless SF_SIG_ENDED is set.
 * Both carry the same flag word:
 *   SF_SIG_PRESENT     alive and commanded now: sf_agent_alive's bit (Character.hpp:291,333-338)
 *   SF_SIG_DIED        present at the previous call, gone now, and its game was not ended by that (hit_human's
 *                      deleteAgent, gameplay.hpp:648-649)
 *   SF_SIG_ENDED       this agent's game ended since the previous call (check_end, gameplay.hpp:1102-1229,1450)
 *   SF_SIG_REBASED     rule 1 below: the baseline was set anew, deltas and reward are 0
 *   SF_SIG_UNRESOLVED  rule 2, or a death that rule 4 cannot attribute
 *   SF_SIG_IDLE        the arena stands still: done, and already done at the previous call; the reward is 0
 * Rules, per arena in this order; n = sf_arena_hdr.episodes now - in the baseline.  After every rule the baseline becomes
 * the current state.
 *   1. Rebase: the first call after create; the agent's d_rebase byte set; n < 0 (a whole sf_reset); n == 0 with another
 *      (tb, serial) or with fewer steps than the baseline's (an sf_reset_arenas or sf_snapshot_load the caller did not
 *      announce).  Flags REBASED (and PRESENT), deltas 0.  d_rebase is authoritative: pass sf_reset_sel.d_selected, or
 *      the agents of the arenas an sf_snapshot_load named.  The detection is a guard, and what it catches is counted; it
 *      cannot see a whole sf_reset onto the running seed before the first game has ended, nor a load of the arena's OWN
 *      state of the same game with a step count that is not below the baseline's (a save, steps, load, the same number of
 *      steps again): such calls read as one game going on, with the differences of the counters as deltas.
 *   2. n >= 2: several games ended inside one launch (sf_step_device with k > 1 under auto_reset).  Flags ENDED |
 *      UNRESOLVED, deltas 0, outcome the latch's (the last game's).  The episode log has every one of those games.
 *   3. n == 1: the ended game's last values are its row of the result latch (sf_results), whether or not the arena has
 *      restarted since.  Agents present in the baseline: delta = latch - baseline.  Flags ENDED, outcome = latch word 7.
 *      The latch row of a commanded human other than `ind` holds whatever stands in its slot when the game ends
 *      (sf_results' own rule): a human that died in that very step still shows its corpse, one whose slot a spawned NPC
 *      took shows the NPC.
 *   4. n == 0, the same game.  An agent present in the baseline and
 *        - still present: delta = current - baseline, PRESENT;
 *        - gone, its slot not alive, exactly one step since the baseline: the row is its own corpse's: delta = current -
 *          baseline, DIED;
 *        - gone otherwise (the slot alive again: h_ind handed it to a spawned NPC, gameplay.hpp:216-221; or several steps
 *          passed, in which that may have happened and ended again): d kills, d damage, d effect 0, d teams_kills and d
 *          loot current - baseline (they are the arena's), d Hp = -(baseline Hp); DIED, and UNRESOLVED if more than one
 *          step passed.
 *      An agent not present in the baseline has all-zero deltas (under rules 2 and 3 it still gets ENDED and the outcome).
 *      A replayed arena whose stream ran out (sf_replay_step: done newly set, no episode counted) reports ENDED with
 *      outcome SF_SAMPLE_END beside the above.
 * Reward, float32, separate multiplies and adds in this order, nothing fused:
 *      r = 0
 *      if present in the baseline:  r = per_step;  for j in 0..5:  r = r + w[j] * (float)delta[j]
 *      if DIED:  r = r + died
 *      if ENDED and present in the baseline and not UNRESOLVED:  r = r + outcome[code]
 *   and 0 under REBASED and IDLE.
 * sf_signals_step is one kernel launch in stream order on the environment's stream: no allocation, no copy, no host
 * synchronisation; the struct travels in the kernel arguments (it may be a temporary) and the call may be captured in a
 * graph behind sf_step_device.  create, destroy and status synchronise.  Destroy a signals object before its environment.
 * sf_signals_status: how many delta records carried UNRESOLVED, how many were rebased by the detection alone (valid
 * baseline, d_rebase byte clear), 0, 0, since create or the last status call; it clears the counters.
 * SF_ERR_STATE: before the first sf_reset, between sf_step_begin and sf_step_end, a signals object of another environment.
 * SF_ERR_ARG: null handles, or a non-NULL pointer that is not device memory of the environment's device, is not aligned
 * (4 bytes; d_rebase 1) or whose extent reaches past its allocation; nothing is launched then. */
#define SF_VITALS_WORDS 16
#define SF_DELTA_WORDS 8
enum { SF_SIG_PRESENT = 1, SF_SIG_DIED = 2, SF_SIG_ENDED = 4, SF_SIG_REBASED = 8, SF_SIG_UNRESOLVED = 16, SF_SIG_IDLE = 32 };
typedef struct sf_signals sf_signals;          /* opaque; belongs to one env; owns a per-(arena, agent) baseline on the device */
int sf_signals_create(sf_env *env, sf_signals **out);
int sf_signals_destroy(sf_signals *s);         /* before its env */
typedef struct sf_reward_weights {             /* travels by value in the kernel arguments */
  float per_step;                              /* for an agent that was present at the previous call */
  float w[6];                                  /* kills, teams_kills, loot, damage, effect, Hp: sf_results' words 0..5 */
  float died;                                  /* added on SF_SIG_DIED */
  float outcome[8];                            /* by SF_* outcome code, added on SF_SIG_ENDED */
} sf_reward_weights;
typedef struct sf_signals_io {
  int32_t *d_vitals;         /* optional, [arenas][n_agents][SF_VITALS_WORDS] */
  int32_t *d_delta;          /* optional, [arenas][n_agents][SF_DELTA_WORDS] */
  float   *d_reward;         /* optional, [arenas * n_agents]: the layout sf_rollout_step.d_reward takes */
  const uint8_t *d_rebase;   /* optional, [arenas][n_agents] (sf_reset_sel.d_selected's layout): != 0 -> rule 1 */
  sf_reward_weights weights; /* read only when d_reward != NULL */
} sf_signals_io;
int sf_signals_step(sf_env *env, sf_signals *s, const sf_signals_io *io);
int sf_signals_status(sf_signals *s, int64_t out_host[4]);   /* unresolved, rebased by detection, 0, 0; synchronises; clears */

/* ---- action masks: which commands would do anything right now, on the device ----------------------------------------
 * The reference's obey() (gameplay.hpp:695-821) silently drops most of what a bot may send: a step into a wall, a zombie
 * or the map's edge, a shot with the bullet pool dry, 'u' with the selection on a weapon, '[' with no blocks left, a
 * selection that is the selection already.  sf_action_mask_device says, for every (arena, commanded human) at once and
 * without leaving the device, which commands are not such no-ops.
 * The command table is valid_commands (gameplay.hpp:45) with '_' appended: SF_COMMANDS, SF_N_COMMANDS characters; bit k of
 * a mask word stands for SF_COMMANDS[k].
 * Definition.  For a commanded human g (slot g < n_agents) of arena a that is present (alive and commanded: SF_SIG_PRESENT's
 * rule), bit k is set exactly when obey(SF_COMMANDS[k]) for that human, run on the arena's state as it is stored at the
 * moment of the launch, would change at least one word of that state.  One exception: bit 0 ('+') is set for every present
 * agent, so the word of a present agent is never 0.  An agent that is not present gets the word 0.  The one rule decides
 * every corner: 'q' and 'e' are always set and '3' never; a selection that is the selection already is clear; 'x' that
 * charges stamina but whose bullet may not enter the cell is set (the state changed), 'x' without enough stamina is clear;
 * '_' is set while Hp != 0.  A present agent without a position (the value a Battle seat has before it is placed; no stored
 * state holds it) gets bit 0 only.
 * What a set bit is not: a promise.  The mask is taken from the stored state, and zombie_action, the bullets' half-tick and
 * the humans earlier in the sweep run between that state and this human's obey (gameplay.hpp:1455-1464).  Nor does it say
 * that a command is useful: a shot that charges stamina but cannot leave the muzzle stays set.  teleport and claim_chest
 * follow obey and are not commands.
 * One kernel launch in stream order on the environment's stream: no allocation, no copy, no host synchronisation; nothing
 * of the environment is written; the struct and the action string travel in the kernel arguments (both may be temporaries)
 * and the call may be captured in a graph behind sf_step_device.  Allowed whenever the state is stored: after any step,
 * between sf_step_begin and sf_step_end, while a replay is loaded.
 * SF_ERR_STATE: before the first sf_reset.  SF_ERR_ARG: null handles; no output at all; d_actions without action_string or
 * the reverse; an action string that is empty, longer than 32 or holds a character that is not in SF_COMMANDS; a non-NULL
 * output that is not device memory of the environment's device, is not 4-byte aligned or whose extent reaches past its
 * allocation.  Nothing is launched then. */
#define SF_COMMANDS "+qe3uzxawsdfghjkl;'cvbnm,./[]_"
#define SF_N_COMMANDS 30
typedef struct sf_action_mask_io {
  uint32_t *d_commands;       /* optional out, device, [arenas][n_agents]: the 30-bit word, bit k = SF_COMMANDS[k] */
  const char *action_string;  /* optional, host, 1..32 chars of SF_COMMANDS: a bot's action set ("+xzqeawsd"); repeats allowed */
  uint32_t *d_actions;        /* optional out, device, [arenas][n_agents]: bit j = the bit of action_string[j]; what
                                 sf_policy_act_masked takes as d_action_mask.  Needs action_string, and the reverse */
} sf_action_mask_io;
int sf_action_mask_device(sf_env *env, const sf_action_mask_io *io);
int sf_action_mask(sf_env *env, uint32_t *out_host);   /* the command words [arenas][n_agents] through the host; synchronises */

/* One iteration of gameplay::play()'s while(true) body, gameplay.hpp:1452-1471, followed by the next
 * iteration's loop-top (spawns + check_end, gameplay.hpp:1444-1450), for every arena.
 * cmd: host array [arenas][n_agents] of reference command chars (valid_commands gameplay.hpp:45, plus
 * '_' gameplay.hpp:696); replaces get_my_action()/client.recieve() (gameplay.hpp:939-963,170-193). */
int sf_step(sf_env *env, const uint8_t *cmd);

/* Same, `k` iterations in one launch, commands already resident in device memory
 * ([k][arenas][n_agents]).  This is the throughput path. */
int sf_step_device(sf_env *env, const uint8_t *d_cmd, int32_t k);

/* The same iteration in two calls, cut where the reference asks the agents of humans OTHER than `ind` for their command:
 * get_command(i) -> bot(hum[i]) runs inside human_action (gameplay.hpp:988-999), i.e. after zombie_action ... the first
 * update_bull (gameplay.hpp:1455-1463), whereas the player `ind` was asked at the loop top (gameplay.hpp:955-958).
 *   sf_step_begin          gameplay.hpp:1455-1463
 *   sf_observe...          what bot(hum[i]), i != ind, encodes (only built with USE_AGENT_IN_SQUAD_NPCS does the
 *                          reference have such agents: Squad mode, gameplay.hpp:1883-1885,1896-1898)
 *   sf_step_end(cmd)       gameplay.hpp:1464-1471 + the next loop top; cmd as for sf_step (the entry of `ind` being
 *                          the command chosen at the loop top)
 * sf_step == sf_step_begin + sf_step_end on the same commands, bit for bit.  Between the two calls only the observe /
 * dump / digest / agent_alive entry points may be used (SF_ERR_STATE otherwise). */
int sf_step_begin(sf_env *env);
int sf_step_end(sf_env *env, const uint8_t *cmd);
int sf_step_end_device(sf_env *env, const uint8_t *d_cmd);

/* Replaces Human::active_agent / deleteAgent (Character.hpp:291,333-338): out[arenas][n_agents], 1 while the commanded
 * human is alive and still driven through sf_step.  The reference deletes a dead human's Agent in hit_human
 * (gameplay.hpp:648-649) and never queries it again (gameplay.hpp:985,991: `mh[i]`, get_active_agent()); its slot may
 * be handed to a spawned NPC (h_ind, gameplay.hpp:216-221), which then runs on human_rnpc_bot: commands sent for a
 * dead agent are ignored and its observation is all zero.  (The player `ind` dying ends the episode: sf_done.) */
int sf_agent_alive(sf_env *env, uint8_t *out_host);
int sf_agent_alive_device(sf_env *env, uint8_t *d_out);

/* Replaces gameplay::bot() observation encoding, bots/bot-0.5/Custom.hpp:29-159, for every
 * (arena, agent): out[arenas][n_agents][32][31][31] float32. */
int sf_observe(sf_env *env, float *out_host);
int sf_observe_device(sf_env *env, float *d_out);
/* The same observation for a caller that keeps ONE device buffer per env and never writes to it: only the floats
 * that were non-zero after the previous call on this buffer, or are non-zero now, are written (an observation is
 * about 1 % non-zero, so this is a small fraction of the 123 KB per agent).  The first call on a buffer, a call with
 * another pointer, or one after a plain observe call on it writes everything.  The buffer ends up bit-identical
 * to what the plain call would have written. */
int sf_observe_device_delta(sf_env *env, float *d_out);
/* The same observation as the list of its non-zero floats, for a consumer on the device that can take it in that form
 * (sf_policy_forward_sparse: the bot network's first convolution works on the non-zeros anyway): nothing dense is
 * written at all.  Per (arena, agent) i: d_counts[i] entries, in the dense buffer's own order (channel, then row, then
 * column), d_keys[i * cap + e] = channel * 9 | row << 9 | column << 14 and d_vals[i * cap + e] the float the dense
 * call would have written there, bit for bit; d_pov[i * 160 ..] = the 5 x 32 floats around the window's centre that
 * AgentModel::forward reads directly (Modules.hpp:114-121: cells (-1,0) (0,-1) (0,0) (0,1) (1,0), channel fastest).
 * d_counts[i] > cap (the list was cut) or == 0xffffffff (a window more crowded than the kernel's record table) means:
 * take the dense call for this step.  An observation of the BASELINE configurations has ~250 non-zeros. */
#define SF_OBS_POV_FLOATS 160
int sf_observe_sparse_device(sf_env *env, uint32_t *d_keys, float *d_vals, uint32_t *d_counts, float *d_pov, int32_t cap);
/* The dense call for exactly the agents whose list did not fit (d_counts[i] > cap, or the 0xffffffff marker), to be
 * issued right behind sf_observe_sparse_device with the same d_counts / cap: their rows of d_dense
 * ([arenas][n_agents][32][31][31], the other rows are not touched) get the observation sf_observe_device would write,
 * and their rows of d_pov are rewritten from it.  Normally no agent qualifies and the two launches exit at once; no
 * host synchronisation either way.  sf_policy_forward_sparse_or_dense then evaluates those agents from d_dense. */
int sf_observe_overflow_device(sf_env *env, const uint32_t *d_counts, int32_t cap, float *d_dense, float *d_pov);

/* Per (arena, agent) 8 x int32: kills, teams_kills, loot, damage, effect, Hp, frames, outcome
 * (gameplay.hpp:461,588-593,625-629; Character.hpp:294).  Latched at episode end: one record per arena, which the next
 * end overwrites.  To receive every finished episode's record, also those of an arena that ended two inside one
 * launch, turn on the episode log below. */
int sf_results(sf_env *env, int32_t *out_host);
int sf_results_device(sf_env *env, int32_t *d_out);

/* ---- episode log: every finished episode's result record, kept on the device ---------------------------------
 * The reference ends a game where `if(check_end()) break;` leaves play()'s loop (gameplay.hpp:1450; check_end
 * gameplay.hpp:1102-1229) and the caller reads the counters of that game (the fields sf_results carries,
 * gameplay.hpp:461,588-593,625-629; Character.hpp:294).  With the log on, each arena keeps a device ring of its last
 * `depth` finished episodes, written by the step kernels at the moment check_end ends a game, whichever entry point
 * stepped it (sf_step, sf_step_device, sf_step_begin / sf_step_end).  A game that sf_reset's own first loop top ends is
 * not counted by sf_arena_hdr.episodes (the arena stands still before its first iteration) and is not logged.  Off by
 * default; while off nothing is allocated, the step kernels launched are the ones without log code, and nothing behaves
 * differently.
 * One record = SF_EPISODE_HDR_WORDS header words, then n_agents x 8 words:
 *   arena, episode, tb_lo, tb_hi, serial_lo, serial_hi, steps, outcome | per agent exactly what sf_results held then
 * episode: 0-based ordinal since sf_reset (sf_arena_hdr.episodes while it ran); tb / serial: the seed of the episode
 * that ended (with auto_reset and reseed_stride, tb = the arena's first tb + episode x stride: a key unique across
 * shards); steps: loop iterations, as sf_arena_hdr.steps; outcome: SF_WON ... as in sf_results. */
#define SF_EPISODE_HDR_WORDS 8
/* depth: a power of two in [1, 64] (re)allocates an empty ring; 0 turns the log off and frees it.  Not between
 * sf_step_begin and sf_step_end.  Only episodes that end from now on are offered (each arena's cursor starts at its
 * current count); sf_reset empties the rings and restarts the cursors at episode 0. */
int sf_episode_log(sf_env *env, int32_t depth);
/* The records not delivered yet, as one dense list in arena-ascending then episode-ascending order, at most max_records
 * of them: d_out [max_records][SF_EPISODE_HDR_WORDS + 8 n_agents] int32 and d_counts [3] = written, lost (ended since
 * the last call but already overwritten in the ring: more than `depth` in between), still pending (did not fit; offered
 * again by the next call).  Each arena's cursor advances past what it delivered and what it lost.  The device form is
 * two kernel launches on the library's stream with no host synchronisation: it may be captured in a graph behind
 * sf_step_device.  A captured graph holds the ring's, the cursors' and the plan's addresses and the k_step instance
 * chosen at capture time (the log has one of its own): any later sf_episode_log call invalidates it, so capture again
 * after one.  SF_ERR_STATE while the log is off or between sf_step_begin and sf_step_end. */
int sf_episodes(sf_env *env, int32_t *out_host, int32_t max_records, int32_t *counts_host);
int sf_episodes_device(sf_env *env, int32_t *d_out, int32_t max_records, int32_t *d_counts);
/* The raw rings, out [arenas][depth][record] int32 (episode e of an arena in slot e & (depth - 1)); empty slots have
 * episode == -1.  Leaves the cursors alone. */
int sf_episode_ring(sf_env *env, int32_t *out_host);

/* ---- replay of logged games: per-arena command streams, fetched on the device ------------------------------------
 * The reference replays a logged game (`.sf_sample`, include/sf_sample.hpp) by reading its commands back inside the
 * loop: `replay_file >> command[ind]` at the head of human_action (gameplay.hpp:968-969) and, in a match, one
 * `replay_file >> command[i]` for every other human with mh[i] && remote[i], slots ascending (gameplay.hpp:979-986;
 * the file is opened and its header read in load_data, gameplay.hpp:1749-1806).  How many lines an iteration takes thus
 * depends on who is still alive after the first half of that very iteration (gameplay.hpp:1455-1463), so the lines
 * cannot be laid out beforehand as [k][arenas][n_agents]: they are fetched where the state is.
 *
 * sf_replay_load: one stream of command chars per arena, in file order; arena a owns streams[offsets[a] ..
 * offsets[a + 1]) (host memory, offsets [arenas + 1] non-decreasing, less than 4 GiB in all).  Uploads them and puts every
 * cursor at its stream's start.  Needs auto_reset == 0 (SF_ERR_STATE otherwise); the seeds are sf_reset's, which also
 * rewinds the streams.  sf_replay_load(env, NULL, NULL) frees everything; while nothing is loaded nothing is allocated
 * and no other entry point behaves differently.
 *
 * sf_replay_step: one iteration of every arena with the commands taken from the streams on the device, no host
 * synchronisation: a loop-top check, the first half of the iteration (as sf_step_begin), the fetch, the second half (as
 * sf_step_end_device) — two small launches more than the split step.  Per arena:
 *   - loop top: an arena whose game has ended (check_end, gameplay.hpp:1450) stands still as ever, state GAME_ENDED, the
 *     rest of its stream unread.  Otherwise, if the cursor has reached the stream's length, the arena stops exactly as a
 *     finished game without auto_reset does — done = 1, outcome = SF_SAMPLE_END, sf_done = 1, the state as the last
 *     iteration left it (sf_dump_arena / sf_state_digest give the replay's final world) — state SAMPLE_ENDED.  This is not
 *     an episode: sf_arena_hdr.episodes does not move, sf_results is not latched, the episode log gets no record.
 *     Otherwise the next line is the command of `ind`.
 *   - between the halves: every commanded human g != ind that sf_agent_alive would report (alive and still commanded; a
 *     dead player's slot re-used by a spawned NPC is not) takes the next line, slots ascending.  Where the stream ends in
 *     the middle of this, the humans without a line obey '+' (what the reference's failed read leaves in command[i],
 *     gameplay.hpp:1009), the state becomes TRUNCATED and the arena stops at the next loop top like SAMPLE_ENDED.
 * sf_replay_status: per arena 4 x int32: state (SF_REPLAY_*), cursor (lines taken), iterations played, 0.
 * sf_replay_commands_device: uint8 [arenas][n_agents], the line each commanded human took in the LAST iteration, 0 where
 * it took none (dead, gone, arena stopped).  With an sf_observe* call in front of sf_replay_step this is the
 * (observation, action) pair a replay_mode Agent of `ind` sees: bot() at the loop top (gameplay.hpp:955-958), update() in
 * human_action (gameplay.hpp:970-975).  The other players' mid-iteration observations are not part of this call: a caller
 * who wants them keeps to sf_step_begin / sf_observe / sf_step_end and feeds the lines itself.
 * SF_ERR_STATE: nothing loaded, before sf_reset, or between sf_step_begin and sf_step_end. */
enum { SF_REPLAY_RUNNING = 0, SF_REPLAY_GAME_ENDED = 1, SF_REPLAY_SAMPLE_ENDED = 2, SF_REPLAY_TRUNCATED = 3 };
int sf_replay_load(sf_env *env, const uint8_t *streams, const int64_t *offsets);
int sf_replay_step(sf_env *env);
int sf_replay_status(sf_env *env, int32_t *out_host);
int sf_replay_status_device(sf_env *env, int32_t *d_out);
int sf_replay_commands_device(sf_env *env, uint8_t *d_out);

/* ---- recording of games as command streams, on the device ------------------------------------------------------------
 * The reference writes a `.sf_sample` while a game is played: with `enable_logging`, human_action appends the command of
 * `ind` (`log_file << command[ind]`, gameplay.hpp:966-967) and then one line for every other human with mh[i] && remote[i],
 * slots ascending (gameplay.hpp:982-983, 990-991), behind the header load_data wrote (gameplay.hpp:1784-1794, 1836-1845,
 * 1867-1869, 1910-1914).  How many lines an iteration has depends on who is alive after its first half, so the stream is
 * written where the state is: sf_record_step is sf_replay_step's inverse.  A recorder belongs to one environment and owns,
 * per arena, a region of bytes_per_arena bytes for the streams and an index of games_per_arena game records.
 *
 * sf_record_step plays one iteration of every arena, bit for bit what sf_step_device(d_cmd, 1) does to the environment
 * (auto_reset, the result latch and the episode log included): a loop-top record launch, the first half (as
 * sf_step_begin), a record launch between the halves (not where n_agents == 1), the second half (as sf_step_end_device)
 * and a closing record launch: three small launches more than the split step, all on the environment's stream, no host
 * synchronisation.  d_cmd: device, [arenas][n_agents], as for sf_step_end_device.  Per arena — the game it is writing is
 * its open game:
 *   - loop top.  A done arena writes nothing.  An open game that the arena was restarted under (steps == 0 again:
 *     sf_reset_arenas, sf_reset) is closed as SF_RECORD_CUT — as SF_RECORD_BROKEN if sf_arena_hdr.episodes says that a game
 *     ended in between, behind the recorder's back.  An open game whose iteration count differs from sf_arena_hdr.steps
 *     (the arena was stepped through another entry point, or loaded from a snapshot), and one found open in a done arena
 *     (the closing launch below closes every game this call ends: another call ended this one), is SF_RECORD_BROKEN.  An arena
 *     without an open game opens one iff steps == 0: the record takes the arena, sf_arena_hdr.episodes and the running
 *     seed.  An arena with steps != 0 and no open game records nothing until its next steps == 0.  Where the index is full
 *     the game is not opened and counted as lost.  Then the command of `ind` is appended; this needs n_agents free bytes
 *     in the region (a whole iteration), otherwise the game is closed as SF_RECORD_OVERFLOW with nothing of this iteration
 *     written: a stream only ever holds whole iterations and never replays as SF_REPLAY_TRUNCATED.
 *   - between the halves.  Every commanded human g != ind that sf_agent_alive would report (sf_replay_step's own
 *     predicate: a dead player's slot re-used by a spawned NPC is not) appends its byte of d_cmd, slots ascending.
 *   - closing.  A game that check_end ended in this iteration (gameplay.hpp:1450) is closed as SF_RECORD_GAME_ENDED with
 *     its outcome (sf_arena_hdr.outcome; under auto_reset the latched result's).  GAME_ENDED is reported exactly then.
 *   - a command byte <= 0x20 or >= 0x7f cannot stand in a sample (`operator>>` reads one token per command) and is
 *     written as '+' and counted.  Every such byte acts as '+' in the step itself (obey, gameplay.hpp:695-821, knows its
 *     command chars and ignores every other byte), so the stream still replays to the same game.
 * sf_record_flush closes every open game as SF_RECORD_CUT (one launch); the arena records again from its next steps == 0.
 *
 * sf_record_collect_device delivers every CLOSED game, arena ascending and game ascending within an arena: d_games gets
 * SF_RECORD_GAME_WORDS int32 per game — arena, episode, tb lo, hi, serial lo, hi, lines, iterations, end (SF_RECORD_*),
 * outcome (SF_*; SF_RUNNING unless GAME_ENDED), byte offset lo, hi into d_bytes — and d_bytes the streams back to back:
 * offsets and lines are what sf_replay_load takes as `offsets` / `streams`.  Delivery stops at the first game that does not
 * fit max_bytes / max_games; it and every later game stay pending, the order is never broken.  The space of delivered
 * games is free again; an open game goes on uninterrupted.  d_counts, int64 [6]: games delivered, bytes delivered, games
 * pending, bytes pending, games lost to a full index and bytes substituted since the last collect.  Two launches on the
 * environment's stream, no host synchronisation.  sf_record_collect is the same into host memory and synchronises.
 * create and destroy synchronise.  Destroy a recorder before its environment.  While no recorder exists nothing is
 * allocated and no other entry point behaves differently.
 * Not recorded: iterations inside sf_step_device (any k) or sf_step / sf_step_begin; the continuation of a forked or loaded
 * game (BROKEN).  The character records of a sample's header are the configuration's, not the recorder's.
 * SF_ERR_STATE: before the first sf_reset, between sf_step_begin and sf_step_end, while a replay is loaded.  SF_ERR_ARG: null
 * handles, a recorder of another environment, a null d_cmd, bytes_per_arena < n_agents or >= 2^31, games_per_arena < 1,
 * max_bytes / max_games < 1, an output that is not device memory of the environment's device, is not aligned (d_games 4,
 * d_counts 8) or shorter than max_bytes / max_games say; nothing is launched then. */
#define SF_RECORD_GAME_WORDS 12
#define SF_RECORD_COUNT_WORDS 6
enum { SF_RECORD_GAME_ENDED = 1, SF_RECORD_CUT = 2, SF_RECORD_OVERFLOW = 3, SF_RECORD_BROKEN = 4 };
typedef struct sf_recorder sf_recorder;        /* opaque; belongs to one env */
int sf_record_create(sf_env *env, int64_t bytes_per_arena, int32_t games_per_arena, sf_recorder **out);
int sf_record_destroy(sf_recorder *r);         /* before its env */
int sf_record_step(sf_env *env, sf_recorder *r, const uint8_t *d_cmd);
int sf_record_flush(sf_env *env, sf_recorder *r);
int sf_record_collect_device(sf_recorder *r, uint8_t *d_bytes, int64_t max_bytes, int32_t *d_games, int32_t max_games,
                             int64_t *d_counts);
int sf_record_collect(sf_recorder *r, uint8_t *bytes_host, int64_t max_bytes, int32_t *games_host, int32_t max_games,
                      int64_t *counts_host);

/* ---- multi-GPU: the one exchange step ------------------------------------------
 * Arenas are sharded over one sf_env per GPU with no data-path collective.  The result records of all shards are
 * exchanged with an RCCL all-gather over xGMI.  The reference has no counterpart (its only inter-process traffic is the
 * TCP command relay, gameplay.hpp:113-118,170-193); what this replaces is every client simulating every arena.
 * RCCL is loaded on first use; the communicator is the library's own.  Bootstrap: rank 0 calls sf_comm_unique_id and
 * hands the SF_COMM_ID_BYTES bytes to the other ranks by any means (torch.distributed, MPI, a file); every rank then
 * calls sf_comm_init on its env. */
#define SF_COMM_ID_BYTES 128
int sf_comm_unique_id(uint8_t *id);
int sf_comm_init(sf_env *env, const uint8_t *id, int32_t rank, int32_t world);
/* ncclCommCount of the library's communicator: the number of ranks RCCL itself reports (bench.py prints it) */
int sf_comm_ranks(sf_env *env, int32_t *ranks);
/* Snapshot this env's result records on its stream and all-gather the snapshots of all ranks into d_out
 * ([world][arenas][n_agents][8] int32, device memory) on a side stream owned by the library: the call returns at
 * once and the gather runs beside the launches that follow.  d_out is complete after sf_comm_wait. */
int sf_results_allgather(sf_env *env, int32_t *d_out);
/* The same for the episode log: snapshot the raw rings (sf_episode_ring's layout) and all-gather them into d_out
 * ([world][arenas][depth][record] int32, device memory) on the side stream; staging is allocated on first use.  The
 * cursors are not touched: a consumer keeps its own per (rank, arena) and takes the records whose episode is newer. */
int sf_episodes_allgather(sf_env *env, int32_t *d_out);
/* Make the env's stream (and, with host_too != 0, the calling thread) wait for every gather issued so far. */
int sf_comm_wait(sf_env *env, int32_t host_too);

/* Replaces the loop exit test `if(check_end()) break;` gameplay.hpp:1450.  Without auto_reset: 1 once the arena's
 * episode has ended (the arena then stands still).  With auto_reset: the number of episodes (saturating at 255) that
 * ended during the LAST sf_step / sf_step_device call, over all of its k iterations; the arena has already restarted.
 * The result record (sf_results) is the one of the last episode that ended; a caller that gathers records after
 * multi-step launches tells fresh from stale ones by this count or by sf_arena_hdr.episodes, and the episode log
 * (sf_episode_log, sf_episodes_device) hands over every ended episode's record, not only the last. */
int sf_done(sf_env *env, uint8_t *out_host);
/* The same flag on the device, one byte per (arena, agent) (every agent of an arena gets its arena's flag), in the
 * layout the policy library's reset_memory entry (strikeforce_policy.h) takes: with auto_reset it marks the agents whose game just restarted, i.e. where the
 * reference would have built a new Agent in prepare() (gameplay.hpp:481). */
int sf_done_device(sf_env *env, uint8_t *d_out);
/* The same flags where the environment keeps them: arena a's is the int32 at (*d_words)[a * *stride_words], and each of
 * its *agents_per_arena agents takes it (device memory owned by env, valid until sf_destroy, rewritten by every step) —
 * for a consumer on the same stream that can read them in place (sf_policy_predict_sparse) instead of a copy. */
int sf_done_view_device(sf_env *env, const int32_t **d_words, int32_t *stride_words, int32_t *agents_per_arena);

/* ---- parity / tooling ---------------------------------------------------------------------- */
int sf_state_digest(sf_env *env, uint64_t *out_host); /* one 64-bit digest per arena */
/* Generator draws (random.hpp:54-62 `_rand()`) of every arena's LAST iteration by phase, out[arenas][6]: zombie_action
 * (gameplay.hpp:654-693), the first update_bull (:1059-1100: always 1), human_action (:965-1012: the NPC commands + the
 * sweep direction), the second update_bull (1), the next loop top's spawns (:1444-1449), everything else (0:
 * portal_damage, update_tmp and the hits draw nothing).  The state digest pins the TOTAL (jomle); this pins the order in
 * which the phases draw (SURVEY.md §8c golden item 5).  After sf_step_begin: the first two entries are of the running
 * iteration, the others still of the one before. */
int sf_phase_draws(sf_env *env, int32_t *out_host);
int sf_dump_arena(sf_env *env, int32_t arena, sf_arena_hdr *hdr, sf_human_rec *humans,
                  sf_zombie_rec *zombies, sf_bullet_rec *bullets, sf_portal_rec *portals,
                  uint8_t *cell_flags, int32_t *cell_dmg, int32_t *cell_portal);

/* ---- whole-arena state records and digests, on the device ------------------------------------------------------------
 * sf_dump_arena shows one arena per call through a host copy of every arena's state.  sf_state_device decodes the same
 * records where the state lives: for every arena (or the arenas an id list names) at once, in stream order, into device
 * buffers the caller owns.  Every output is optional; a NULL one costs nothing.
 *   Records.  Row i's sf_arena_hdr [gameplay.hpp:461, random.hpp:29-31], sf_human_rec [Character.hpp:65,286-294, the
 *     mh / remote bitsets gameplay.hpp:55], sf_zombie_rec, sf_bullet_rec [gameplay.hpp:814-816,1087-1089], sf_portal_rec
 *     and the three per-cell tables equal, word for word, what sf_dump_arena writes for that arena at that point of the
 *     stream: the all-zero record of a slot that is not alive (zombies, bullets) or not active (exits), the all-zero
 *     position / vec / ind / portal_ind of a human slot never used, the generator words masked to 20 bits, cell_dmg 0 off
 *     a player-built (SF_CELL_TEMP) cell, and cell_portal -1 off an entrance, the side table's exit number on a
 *     player-built entrance and the map's on a map entrance.
 *   Cuts.  humans / zombies / bullets / portals say how many slots per row the four tables hold, 0 .. the
 *     configuration's cap; a table cut below the cap shows the first that many slots, and nothing behind a row's last
 *     requested slot is written.
 *   d_counts, SF_STATE_COUNT_WORDS x int32 per row: alive humans, alive zombies, alive bullets, active exits | per table
 *     the highest alive / active slot + 1, 0 if none.  Counted over the configuration's whole pools whatever the cuts: a
 *     caller that sees extent > zombies knows the cut lost something, and sizes its tables by the extents, not the cap.
 *   d_digest: sf_state_digest's value of that arena, bit for bit, always over the whole pools.
 *   d_arena_ids: row i shows arena d_arena_ids[i]; duplicates are fine.  An id outside [0, arenas) never becomes an
 *     address: every requested output of its row is zero, its eight counts are -1 and its digest is 0.
 * The call writes nothing of the environment: digests, dumps and the next step are as without it.  It is allowed wherever
 * sf_dump_arena is, also between sf_step_begin and sf_step_end.  It is one kernel launch on the environment's stream, two
 * when d_counts or d_digest is asked for (their rows are zeroed first), in stream order: no allocation, no copy, no host
 * synchronisation; the struct travels in the kernel arguments (it may be a temporary) and the call may be captured in a
 * graph behind sf_step_device.  All outputs NULL: SF_OK, nothing launched.
 * sf_state_bytes: the bytes each of the ten outputs must hold for this struct (d_hdr, d_humans, d_zombies, d_bullets,
 * d_portals, d_cell_flags, d_cell_dmg, d_cell_portal, d_counts, d_digest, whether or not the pointer is set); no launch.
 * SF_ERR_STATE: before the first sf_reset.  SF_ERR_ARG: null handles, rows < 1 with ids, a cut below 0 or above its cap,
 * or a non-NULL pointer that is not device memory of the environment's device, is not aligned (8 bytes d_hdr and
 * d_digest, 1 d_cell_flags, 4 the others) or whose extent reaches past its allocation; nothing is launched then. */
#define SF_STATE_COUNT_WORDS 8
typedef struct sf_state_io {
  const int32_t *d_arena_ids;   /* optional, device, [rows]: row i shows arena d_arena_ids[i]; NULL: rows == arenas, row i = arena i */
  int32_t rows;                 /* ignored when d_arena_ids == NULL */
  int32_t humans, zombies, bullets, portals;  /* slots per row in the four tables below: 0 .. the configuration's cap */
  sf_arena_hdr  *d_hdr;         /* optional, [rows] */
  sf_human_rec  *d_humans;      /* optional, [rows][humans]  */
  sf_zombie_rec *d_zombies;     /* optional, [rows][zombies] */
  sf_bullet_rec *d_bullets;     /* optional, [rows][bullets] */
  sf_portal_rec *d_portals;     /* optional, [rows][portals] */
  uint8_t *d_cell_flags;        /* optional, [rows][floors*rows*cols] */
  int32_t *d_cell_dmg;          /* optional, same shape */
  int32_t *d_cell_portal;       /* optional, same shape */
  int32_t *d_counts;            /* optional, [rows][SF_STATE_COUNT_WORDS] */
  uint64_t *d_digest;           /* optional, [rows] */
} sf_state_io;
int sf_state_device(sf_env *env, const sf_state_io *io);
int sf_state_bytes(sf_env *env, const sf_state_io *io, int64_t bytes_out[10]);

/* ---- write arenas from state records, on the device --------------------------------------------------------------------
 * The inverse of sf_state_device.  The reference can set a world up in one way only, replaying a logged game from tick 0
 * (gameplay.hpp:968-986); sf_reset builds one from a seed and sf_snapshot_load reloads an opaque state of this library.
 * sf_state_put_device packs the canonical records — a state the caller designed, edited, or took from sf_state_device,
 * sf_dump_arena or the oracle's dump — into the arenas a row map names, in stream order, from device buffers the caller
 * owns.  Arena a takes row d_row_of_arena[a]; many arenas may name one row (the fork); -1: no word of the arena is written.
 *   The core property.  Take an environment B of the same configuration as A and put into arena y of B everything
 *     sf_state_device wrote for arena x of A (whole pools, all three cell tables).  Then y of B cannot be told from x of A by
 *     any reader or any later step: all ten outputs of sf_state_device and sf_state_digest are equal; observations, action
 *     masks, sf_done* and the results of later games are equal; under equal commands the digest after every later step is
 *     equal, across game ends under auto_reset too.
 *   What the destination keeps, by sf_snapshot_load's rule: sf_arena_hdr.episodes (the record's value is ignored), the
 *     result latch, the episode-log ring and its cursor, the cursors of replays, rollout buffers and networks.  The per-step
 *     restart flag of a written arena (what sf_done reports under auto_reset) is cleared and sf_phase_draws of it is 0
 *     until its next step.  The put is announced through d_selected as sf_reset_arenas announces a restart; pass it as
 *     sf_signals_step's d_rebase, to sf_policy_reset_memory and to sf_rollout_record.  The signals' rule 1 and the recorder
 *     (BROKEN) detect a loaded arena on their own as they detect sf_snapshot_load: neither needed a change.
 *   State the records do not show is derived: which humans are commanded, which occupy their cell and which agent record
 *     they were built from (from the slot, the configuration and `alive`: a dead `ind` keeps its cell and its command, every
 *     other dead human loses both); the generator's seed digits (the decimal digits of hdr.serial and hdr.tb); the next
 *     episode's generator under auto_reset, armed as after a restart with the seed hdr.tb + reseed_stride (the restart
 *     that adopts it draws whatever is missing: the trajectory is the one of an arena that warmed it up on the way); the
 *     draw count jomle - 1042, the population the launch order uses and the words of the large pools in use.  Slots that
 *     are not alive / active are written in one form: all-zero words, a human slot never used (way 0) as sf_reset leaves it.
 *   Parts.  Every part is optional: with d_hdr NULL the scalars, the seeds and both generators stay; a table that is NULL
 *     stays, with its derived scalars (the population only changes when humans and zombies are both given); the three cell
 *     tables come all or none.  A table that is given is written over its whole pool: humans / zombies / bullets / portals
 *     say how many slots per row the caller's table holds, 0 .. the cap, and the slots behind the cut become empty.
 *   Validation, per row, before any word of any arena is written.  No field becomes an address or a table index
 *     unchecked: every placed position inside floors x rows x cols; way 1..4 (a human's 0 only on an all-zero slot); the
 *     0 / 1 fields; team 0..255; vec -1..2, ind -1..14 and, where vec selects a table, inside it (consumables and
 *     throwables 4, weapons 8); item counts 0..65535, blocks / portals 0..255, portal_ind -1..cap_portals-1 (254 at most);
 *     a bullet's owner 0..cap_humans, range / traveled 0..65535, effect an int16; generator words 0..65536, jomle 1042 ..
 *     2^32-1, frame and steps 0..2^31-1, the counters int32 values, done 0 / 1, outcome 0..6; the consumable type of a cell
 *     only under SF_CELL_CHEST, cell_dmg 0 off a player-built cell, cell_portal -1 off an entrance, in [0, cap_portals) on a
 *     player-built entrance and the map's own number on a map entrance.  A row that fails writes nothing to any arena that
 *     names it: d_status has the SF_PUT_BAD_* bits of its failed parts and the library counts the arena as refused.  A row
 *     index outside [-1, rows) never becomes an address: SF_PUT_BAD_ROW, counted apart.
 *     Consistency of the game is the caller's: two occupants of one cell, an occupant in a wall, a `ref` bit that
 *     disagrees with its neighbours are played as they stand; the guarantees for those are memory safety and determinism.
 *   d_status, int32 [arenas]: -1 not named, 0 written, > 0 refused.  d_selected, uint8 [arenas][n_agents]: 1 for every
 *     agent of an arena that was written, else 0.  sf_state_put_status: arenas written, refused, named a row out of range,
 *     0, since the last call; it synchronises and clears.
 * Three launches on the environment's stream (the verdict rows zeroed, the check over the rows, the write over the
 * arenas), no copy and no host synchronisation; the struct travels in the kernel arguments and the call may be captured
 * in a graph.  The verdict rows (32 bytes a row) are the library's, allocated by the first call that needs more rows than
 * any call before it (outside a capture); later calls allocate nothing.
 * sf_load_arena is the host mirror of sf_dump_arena: whole pools from host memory, any of them NULL (the cell tables all
 * or none), through the same launches; it synchronises, and a refused state is SF_ERR_ARG with the reason in sf_last_error.
 * SF_ERR_STATE: before the first sf_reset, between sf_step_begin and sf_step_end, while a replay is loaded, on a runtime
 * without the launches.  SF_ERR_ARG: null handles or a null d_row_of_arena, rows < 1, a cut below 0 or above its cap, every
 * part NULL, one or two of the three cell tables, a pointer that is not device memory of the environment's device, is not
 * aligned (8 bytes d_hdr, 1 d_cell_flags and d_selected, 4 the others) or whose extent reaches past its allocation;
 * nothing is launched then. */
enum { SF_PUT_BAD_HDR = 1, SF_PUT_BAD_HUMAN = 2, SF_PUT_BAD_ZOMBIE = 4, SF_PUT_BAD_BULLET = 8, SF_PUT_BAD_PORTAL = 16,
       SF_PUT_BAD_CELL = 32, SF_PUT_BAD_ROW = 64 };
typedef struct sf_state_put_io {
  const int32_t *d_row_of_arena; /* device int32 [arenas]: arena a takes row d_row_of_arena[a]; -1: no word of it is written */
  int32_t rows;
  int32_t humans, zombies, bullets, portals; /* slots per row in the four tables, 0 .. cap; slots behind the cut become empty */
  const sf_arena_hdr *d_hdr;        /* each part optional, [rows]; NULL: that part of the destination stays as it is */
  const sf_human_rec *d_humans;     /* [rows][humans]  */
  const sf_zombie_rec *d_zombies;   /* [rows][zombies] */
  const sf_bullet_rec *d_bullets;   /* [rows][bullets] */
  const sf_portal_rec *d_portals;   /* [rows][portals] */
  const uint8_t *d_cell_flags;      /* the three cell tables: all or none; [rows][floors*rows*cols] */
  const int32_t *d_cell_dmg, *d_cell_portal;
  int32_t *d_status;                /* optional out, [arenas] */
  uint8_t *d_selected;              /* optional out, [arenas][n_agents] */
} sf_state_put_io;
int sf_state_put_device(sf_env *env, const sf_state_put_io *io);
int sf_state_put_status(sf_env *env, int64_t out_host[4]);
int sf_load_arena(sf_env *env, int32_t arena, const sf_arena_hdr *hdr, const sf_human_rec *humans, const sf_zombie_rec *zombies,
                  const sf_bullet_rec *bullets, const sf_portal_rec *portals, const uint8_t *cell_flags, const int32_t *cell_dmg,
                  const int32_t *cell_portal);

/* Stream control: the library launches on this hipStream_t (passed as void*); NULL = default stream. */
int sf_set_stream(sf_env *env, void *hip_stream);
int sf_synchronize(sf_env *env);

/* Device time of the step kernels launched since the last call, measured with HIP events on the
 * library's stream: *ms = sum of kernel durations, *launches = number of launches. */
int sf_kernel_time(sf_env *env, int32_t enable, float *ms, int32_t *launches);

/* Which step kernel the last sf_step / sf_step_device launch ran: *fixed_shape = the index of the built fixed shape
 * (a kernel compiled for one listed configuration; the library picks it at sf_create where every fixed field of the
 * configuration equals the shape's, unless SF_STEP_GENERIC=1 is set in the environment), -1 = a generic instance
 * (also: no launch yet, and every launch while the episode log is on). */
int sf_step_kernel(sf_env *env, int32_t *fixed_shape);

const char *sf_last_error(void);
int sf_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* STRIKEFORCE_H */
