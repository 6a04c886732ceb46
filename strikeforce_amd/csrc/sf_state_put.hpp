// sf_state_put.hpp — the inverse of sf_state_records.hpp: the canonical state records of strikeforce.h (sf_arena_hdr,
// sf_human_rec, sf_zombie_rec, sf_bullet_rec, sf_portal_rec, the three per-cell tables) packed into the state words of
// sf_types.hpp.  One text for three users:
//   - k_put_check / k_put_write (sf_api.hip), behind sf_state_put_device and sf_load_arena;
//   - the host side of sf_host.hpp (the struct, the sizes);
//   - the tests' stand-alone program (tests/state_put/put_main.cpp), which calls the lane functions for lanes 0..63 in a loop.
// The encoders and the check predicates are SF_HD and sit beside the decoders they invert: decode(encode(record)) is the
// record, and every bit the decoder does not read follows a rule stated here (DESIGN.md §4 "State put").
//
// Nothing a record holds becomes an address or a table index before its check_* has passed: the check kernel reads the
// caller's rows and writes verdicts only; the write kernel reads the verdicts first and touches an arena only for a row
// whose every check passed.
#pragma once
#include "sf_state_records.hpp"

namespace sf {

// what the encoders and checks need of the configuration
struct PutCfg {
  int32_t F, N, M, H, Z, B, P, cells;
  int32_t mode, n_agents, ind, npc_block, auto_reset, reseed;
};

// ---- check predicates: true = the record may be packed --------------------------------------------------------------------
SF_HD inline bool put_in_map(const PutCfg &c, int32_t f, int32_t r, int32_t cc) {
  return f >= 0 && f < c.F && f < 4 && r >= 0 && r < c.N && r < 1024 && cc >= 0 && cc < c.M && cc < 1024;
}
SF_HD inline bool put_bit(int32_t v) { return v == 0 || v == 1; }
SF_HD inline bool put_u16(int32_t v) { return v >= 0 && v <= 65535; }
// the table `vec` selects bounds `ind`: consumables and throwables 4, weapons 8 (sf_core.hpp:1410,1433,1449); with no
// table selected (vec -1) `ind` is the last selection kept and is never an index
SF_HD inline bool check_human(const PutCfg &c, const sf_human_rec &o) {
  if (o.way == 0) {  // a slot never used: every word zero
    int32_t w[REC_H_WORDS];
    __builtin_memcpy(w, &o, sizeof o);
    bool zero = true;
    for (int j = 0; j < REC_H_WORDS; ++j) zero = zero && w[j] == 0;
    return zero;
  }
  bool ok = o.way >= 1 && o.way <= 4 && put_bit(o.alive) && put_bit(o.remote) && put_bit(o.rnpc) && put_bit(o.profile);
  ok = ok && put_in_map(c, o.f, o.r, o.c) && o.team >= 0 && o.team <= 255;
  ok = ok && o.vec >= -1 && o.vec <= 2 && o.ind >= -1 && o.ind <= 14;
  if (o.vec == 0 || o.vec == 1) ok = ok && o.ind >= 0 && o.ind < 4;
  if (o.vec == 2) ok = ok && o.ind >= 0 && o.ind < 8;
  for (int j = 0; j < 4; ++j) ok = ok && put_u16(o.cons[j]) && put_u16(o.throw_cnt[j]);
  ok = ok && o.blocks >= 0 && o.blocks <= 255 && o.portals >= 0 && o.portals <= 255;
  ok = ok && o.portal_ind >= -1 && o.portal_ind < c.P && o.portal_ind <= 254;
  return ok;
}
SF_HD inline bool check_zombie(const PutCfg &c, const sf_zombie_rec &o) {
  if (!put_bit(o.alive)) return false;
  return !o.alive || (put_in_map(c, o.f, o.r, o.c) && put_bit(o.super_));
}
SF_HD inline bool check_bullet(const PutCfg &c, const sf_bullet_rec &o) {
  if (!put_bit(o.alive)) return false;
  if (!o.alive) return true;
  return put_in_map(c, o.f, o.r, o.c) && o.way >= 1 && o.way <= 4 && put_u16(o.traveled) && put_u16(o.range) &&
         o.effect >= -32768 && o.effect <= 32767 && o.owner >= 0 && o.owner <= c.H && put_bit(o.ref);
}
SF_HD inline bool check_portal(const PutCfg &c, const sf_portal_rec &o) {
  if (!put_bit(o.active)) return false;
  return !o.active || put_in_map(c, o.f, o.r, o.c);
}
// one cell of the three tables.  map_pidx: the map's own exit number of the cell (-1 off a map entrance)
SF_HD inline bool check_cell(const PutCfg &c, uint32_t fl, int32_t cd, int32_t cp, int32_t map_pidx) {
  if ((fl >> SF_CELL_CONS_SHIFT) && !(fl & SF_CELL_CHEST)) return false;  // (all eight bits of the byte are defined)
  const bool temp = (fl & SF_CELL_TEMP) != 0u, pin = (fl & (SF_CELL_PIN_UP | SF_CELL_PIN_DN)) != 0u;
  if (!temp && cd != 0) return false;
  if (!pin) return cp == -1;
  if (temp) return cp >= 0 && cp < c.P;
  return cp == map_pidx;
}
// the header's REC_HDR_WORDS words.  episodes (words 18, 19) is ignored: the destination keeps its own
template <class WP>
SF_HD inline bool check_hdr(WP hw) {
  auto small = [&](int f) { return hw[2 * f + 1] == 0 && hw[2 * f] >= 0; };          // 0 .. 2^31 - 1
  auto i32 = [&](int f) { return hw[2 * f + 1] == (hw[2 * f] >> 31); };              // an int32 value
  bool ok = small(0) && i32(1) && i32(2) && i32(3) && i32(4) && small(8);
  ok = ok && hw[11] == 0 && (uint32_t)hw[10] >= 1042u;                               // jomle: 18 + 1024 warm-up draws at least
  for (int j = 0; j < RNG_WORDS; ++j) ok = ok && hw[20 + j] >= 0 && hw[20 + j] <= 65536;
  return ok && put_bit(hw[38]) && hw[39] >= 0 && hw[39] <= SF_SAMPLE_END;
}

// ---- the encoders: one record -> packed words --------------------------------------------------------------------------
// Dead and empty slots have one form: a human slot never used is POS_NONE and twelve zero words (reset_state,
// sf_core.hpp:1946-1947); a zombie, bullet or exit that is not alive / active is all-zero words (:1949,1952,1125,1089).
//
// The bits of HW_FLAGS no record shows, from the slot, the configuration and `alive`:
//   commanded (HF_CTRL)  as reset_state sets it (sf_core.hpp:1981-1994): Solo / Timer slot 0, Battle the slots below
//                        n_agents, Squad slot 0 and the slots below min(n_agents, 10); never a spawned NPC (rnpc, :549)
//   HF_OCC, HF_CTRL      kept while alive, and by a dead `ind`; cleared for every other dead human (:1108, :1140)
//   HF_AGP_SH            the slot, where every commanded human has a record of its own (Battle, npc_block > 1, :1994), else 0
SF_HD inline uint32_t put_human_hidden(const PutCfg &c, int slot, const sf_human_rec &o) {
  const bool keep = o.alive || slot == c.ind;
  const bool seat = c.mode == SF_MODE_BATTLE ? slot < c.n_agents
                    : c.mode == SF_MODE_SQUAD ? (slot == 0 || (slot < c.n_agents && slot < 10))
                                              : slot == 0;
  uint32_t fl = 0u;
  if (keep) fl |= HF_OCC;
  if (keep && seat && !o.rnpc) fl |= HF_CTRL;
  if (!o.profile && c.mode == SF_MODE_BATTLE && c.npc_block > 1 && slot < c.n_agents) fl |= (uint32_t)slot << HF_AGP_SH;
  return fl;
}
SF_HD inline void encode_human(const PutCfg &c, int slot, const sf_human_rec &o, uint32_t *w) {
  for (int f = 0; f < HW_WORDS; ++f) w[f] = 0u;
  w[HW_POS] = POS_NONE;
  if (o.way == 0) return;
  w[HW_POS] = pos_pack(o.f, o.r, o.c);
  w[HW_FLAGS] = (uint32_t)o.way | ((uint32_t)o.team << HF_TEAM_SH) | (o.alive ? HF_ALIVE : 0u) | (o.remote ? HF_REMOTE : 0u) |
                (o.rnpc ? HF_RNPC : 0u) | (o.profile ? HF_PROF : 0u) | ((uint32_t)(o.vec + 1) << HF_VEC_SH) |
                ((uint32_t)(o.ind + 1) << HF_IND_SH) | put_human_hidden(c, slot, o);
  w[HW_HP] = (uint32_t)o.hp, w[HW_STAMINA] = (uint32_t)o.stamina, w[HW_MINDAMAGE] = (uint32_t)o.mindamage;
  w[HW_KILLS] = (uint32_t)o.kills, w[HW_DAMAGE] = (uint32_t)o.damage, w[HW_EFFECT] = (uint32_t)o.effect;
  w[HW_CONS01] = (uint32_t)o.cons[0] | ((uint32_t)o.cons[1] << 16), w[HW_CONS23] = (uint32_t)o.cons[2] | ((uint32_t)o.cons[3] << 16);
  w[HW_THR01] = (uint32_t)o.throw_cnt[0] | ((uint32_t)o.throw_cnt[1] << 16);
  w[HW_THR23] = (uint32_t)o.throw_cnt[2] | ((uint32_t)o.throw_cnt[3] << 16);
  w[HW_BPK] = (uint32_t)o.blocks | ((uint32_t)o.portals << 8) | ((uint32_t)(o.portal_ind + 1) << 16);
}
SF_HD inline void encode_zombie(const sf_zombie_rec &o, uint32_t *w) {
  w[ZW_POS] = w[ZW_HP] = w[ZW_MINDAMAGE] = 0u;
  if (!o.alive) return;
  w[ZW_POS] = pos_pack(o.f, o.r, o.c) | (o.super_ ? ZF_SUPER : 0u) | ZF_ALIVE;
  w[ZW_HP] = (uint32_t)o.hp, w[ZW_MINDAMAGE] = (uint32_t)o.mindamage;
}
SF_HD inline void encode_bullet(const sf_bullet_rec &o, uint32_t *w) {
  w[BW_A] = w[BW_DAMAGE] = w[BW_B] = w[BW_C] = 0u;
  if (!o.alive) return;
  w[BW_A] = pos_pack(o.f, o.r, o.c) | ((uint32_t)(o.way - 1) << BA_WAY_SH) | BA_ALIVE | (o.ref ? BA_REF : 0u);
  w[BW_DAMAGE] = (uint32_t)o.damage;
  w[BW_B] = ((uint32_t)o.effect & 0xffffu) | ((uint32_t)o.owner << 16);
  w[BW_C] = (uint32_t)o.range | ((uint32_t)o.traveled << 16);
}
SF_HD inline uint32_t encode_portal(const sf_portal_rec &o) { return o.active ? (pos_pack(o.f, o.r, o.c) | PF_ACTIVE) : 0u; }

// decimal digit i of x, plus one (seed_digits, sf_core.hpp:215)
SF_HD inline uint32_t put_digit(uint64_t x, int i) {
  for (int k = 0; k < i; ++k) x /= 10u;
  return (uint32_t)(x % 10u) + 1u;
}
SF_HD inline uint64_t put_u64(int32_t lo, int32_t hi) { return ((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo; }
// tap i of the running generator at rest: value | us << 20 | seed << 24 (sf_core.hpp:2171, :2253); us are the digits of
// hdr.serial, seed those of hdr.tb (srand_, :225-226)
template <class WP>
SF_HD inline uint32_t encode_rng_word(int i, WP hw) {
  return (uint32_t)hw[20 + i] | (put_digit(put_u64(hw[14], hw[15]), i) << 20) | (put_digit(put_u64(hw[12], hw[13]), i) << 24);
}
// tap i of the next episode's generator, armed as after a restart (sf_core.hpp:1973-1977, stored :2254): no draw made yet
// (RL_ZERO = 0x10000 in the log form), the seed digits of tb + reseed.  Without auto_reset nothing arms it (:2325)
template <class WP>
SF_HD inline uint32_t encode_rng2_word(const PutCfg &c, int i, WP hw) {
  if (!c.auto_reset) return 0x10000u;
  return 0x10000u | (put_digit(put_u64(hw[12], hw[13]) + (uint64_t)(uint32_t)c.reseed, i) << 24);
}
// word j of the scalar block.  hw: the header's words, or null (the scalar block stays but for what a put always sets);
// old: the destination's word; derived scalars: live humans + zombies (< 0: stays), 64-slot words of the zombie and exit
// tables in use (< 0: stays)
template <class WP>
SF_HD inline int32_t encode_hdr_word(int j, bool hdr, WP hw, int32_t old, int32_t load, int32_t zwn, int32_t pwn) {
  switch (j) {
    case SC_ENDED: case SC_PD01: case SC_PD23: case SC_PD45: return 0;  // no restart, no draw of a last step to report
    case SC_LOAD: return load >= 0 ? load : old;
    case SC_ZWN: return zwn >= 0 ? zwn : old;
    case SC_PWN: return pwn >= 0 ? pwn : old;
    default: break;
  }
  if (!hdr) return old;
  switch (j) {
    case SC_FRAME: case SC_KILLS: case SC_TKILLS: case SC_LOOT: case SC_CHESTS: case SC_JOMLE: return hw[2 * j];
    case SC_STEPS: return hw[16];
    case SC_DONE: return hw[38];
    case SC_OUTCOME: return hw[39];
    case SC_TB_LO: return hw[12];
    case SC_TB_HI: return hw[13];
    case SC_SR_LO: return hw[14];
    case SC_SR_HI: return hw[15];
    case SC_DRAWS: return (int32_t)((uint32_t)hw[10] - 1042u);  // store(), sf_core.hpp:2275
    case SC_WARM: return 0;
    default: return old;  // SC_EPISODES, and the block's unused word
  }
}
// a cell: the flag byte goes as it is; the side tables are written only where the flags make them valid
SF_HD inline bool encode_cell_has_dmg(uint32_t fl) { return (fl & SF_CELL_TEMP) != 0u; }
SF_HD inline bool encode_cell_has_pidx(uint32_t fl) { return (fl & SF_CELL_TEMP) && (fl & (SF_CELL_PIN_UP | SF_CELL_PIN_DN)); }

// ---- sf_state_put_device: what the two kernels take, by value in the kernel arguments ------------------------------------
enum { PUT_V_BITS = 0, PUT_V_HALIVE, PUT_V_ZALIVE, PUT_V_ZEXT, PUT_V_PEXT, PUT_ROW_WORDS = 8 };  // a row's verdict and extents
enum { PUT_N_WRITTEN = 0, PUT_N_REFUSED, PUT_N_RANGE, PUT_COUNTERS = 4 };                        // sf_state_put_status
struct StatePut {
  uint32_t *hum, *zom, *bul, *por, *rng, *rng2;
  int32_t *scal;
  uint8_t *flags;
  int32_t *aux_dmg;
  int16_t *aux_pidx;
  const int16_t *map_pidx;
  int32_t *verdict;               // [rows][PUT_ROW_WORDS], library-owned
  unsigned long long *counters;   // [PUT_COUNTERS], library-owned
  int32_t A, cells_pad;
  PutCfg c;
  sf_state_put_io io;
};
struct PutUnits {
  int32_t h, z, b, p, c;
  SF_HD int total() const { return 1 + h + z + b + p + c; }
};
// the header unit is always there (it carries the verdict, the status and the derived scalars); a table that is given is
// walked over its whole pool, so that slots behind the cut become empty
SF_HD inline PutUnits put_units(const StatePut &k) {
  PutUnits u;
  u.h = k.io.d_humans ? (k.c.H + 63) / 64 : 0, u.z = k.io.d_zombies ? (k.c.Z + 63) / 64 : 0;
  u.b = k.io.d_bullets ? (k.c.B + 63) / 64 : 0, u.p = k.io.d_portals ? (k.c.P + 63) / 64 : 0;
  u.c = k.io.d_cell_flags ? (k.c.cells + STATE_CELL_CHUNK - 1) / STATE_CELL_CHUNK : 0;
  return u;
}

#if defined(__HIP_DEVICE_COMPILE__)
SF_ST_FN void put_load16(const int32_t *p, int32_t &x, int32_t &y, int32_t &z, int32_t &w) {
  const st_i32x4 v = *reinterpret_cast<const SF_ST_G st_i32x4 *>(st_g(p));
  x = v.x, y = v.y, z = v.z, w = v.w;
}
#else
SF_ST_FN void put_load16(const int32_t *p, int32_t &x, int32_t &y, int32_t &z, int32_t &w) { x = p[0], y = p[1], z = p[2], w = p[3]; }
#endif

// the three tables that come through LDS, with sf_state_records.hpp's strides (29 / 7 / 11 words, odd)
struct PutHumans {
  typedef sf_human_rec Rec;
  enum { W = REC_H_WORDS, S = StHumans::S, FIELDS = HW_WORDS, BIT = SF_PUT_BAD_HUMAN };
  SF_ST_FN uint32_t *dst(const StatePut &k) { return k.hum; }
  SF_ST_FN int pool(const StatePut &k) { return k.c.H; }
  SF_ST_FN int cut(const StatePut &k) { return k.io.humans; }
  SF_ST_FN const int32_t *in(const StatePut &k) { return reinterpret_cast<const int32_t *>(k.io.d_humans); }
  SF_ST_FN bool check(const PutCfg &c, const Rec &o) { return check_human(c, o); }
  SF_ST_FN void encode(const PutCfg &c, int slot, const Rec &o, uint32_t *w) { encode_human(c, slot, o, w); }
};
struct PutZombies {
  typedef sf_zombie_rec Rec;
  enum { W = REC_Z_WORDS, S = StZombies::S, FIELDS = ZW_WORDS, BIT = SF_PUT_BAD_ZOMBIE };
  SF_ST_FN uint32_t *dst(const StatePut &k) { return k.zom; }
  SF_ST_FN int pool(const StatePut &k) { return k.c.Z; }
  SF_ST_FN int cut(const StatePut &k) { return k.io.zombies; }
  SF_ST_FN const int32_t *in(const StatePut &k) { return reinterpret_cast<const int32_t *>(k.io.d_zombies); }
  SF_ST_FN bool check(const PutCfg &c, const Rec &o) { return check_zombie(c, o); }
  SF_ST_FN void encode(const PutCfg &, int, const Rec &o, uint32_t *w) { encode_zombie(o, w); }
};
struct PutBullets {
  typedef sf_bullet_rec Rec;
  enum { W = REC_B_WORDS, S = StBullets::S, FIELDS = BW_WORDS, BIT = SF_PUT_BAD_BULLET };
  SF_ST_FN uint32_t *dst(const StatePut &k) { return k.bul; }
  SF_ST_FN int pool(const StatePut &k) { return k.c.B; }
  SF_ST_FN int cut(const StatePut &k) { return k.io.bullets; }
  SF_ST_FN const int32_t *in(const StatePut &k) { return reinterpret_cast<const int32_t *>(k.io.d_bullets); }
  SF_ST_FN bool check(const PutCfg &c, const Rec &o) { return check_bullet(c, o); }
  SF_ST_FN void encode(const PutCfg &, int, const Rec &o, uint32_t *w) { encode_bullet(o, w); }
};
constexpr int PUT_LDS_WORDS = 64 * PutHumans::S;

// ---- the traversal, one lane at a time (the kernel puts a barrier between the phases) ------------------------------------
// the row an arena takes: -1 not named, >= 0 a row in range; `range` = named a row outside [-1, rows)
struct PutArena {
  int32_t row;
  bool range;
};
SF_ST_FN PutArena put_arena(const StatePut &k, int a) {
  const int32_t r = st_g(k.io.d_row_of_arena)[a];
  PutArena x;
  x.range = r < -1 || r >= k.io.rows, x.row = x.range ? -1 : r;
  return x;
}
// k_put_init: the verdict rows the check's wavefronts add into
SF_ST_FN void put_init_body(const StatePut &k, int i) {
#pragma unroll
  for (int j = 0; j < PUT_ROW_WORDS; ++j) st_g(k.verdict)[(size_t)i * PUT_ROW_WORDS + j] = 0;
}

// phase 1 of a table batch: records 64 v .. of `row` from the caller's table into LDS (record s at lds + s * S), coalesced:
// dwords up to the first 16-byte boundary, 16 bytes per lane from there, dwords for the tail.  Slots at and behind the cut
// are not in the caller's table and are not loaded
template <class T>
SF_ST_FN void put_lane_fill(const StatePut &k, int row, int v, int lane, int32_t *lds) {
  const int slot0 = v * 64, left = T::cut(k) - slot0, n = left < 64 ? left : 64, cnt = n * T::W;
  if (n <= 0) return;
  const int32_t *src = T::in(k) + ((size_t)row * (size_t)T::cut(k) + (size_t)slot0) * T::W;
  auto L = [&](int g) -> int32_t & { return lds[(g / T::W) * T::S + g % T::W]; };
  int head = (int)((4u - (unsigned)((uintptr_t)src >> 2)) & 3u);
  head = head < cnt ? head : cnt;
  if (lane < head) L(lane) = st_g(src)[lane];
  const int nvec = (cnt - head) >> 2;
  for (int q = lane; q < nvec; q += 64) {
    const int g = head + 4 * q;
    int32_t x, y, z, w;
    put_load16(src + g, x, y, z, w);
    L(g) = x, L(g + 1) = y, L(g + 2) = z, L(g + 3) = w;
  }
  const int t = head + 4 * nvec + lane;
  if (t < cnt) L(t) = st_g(src)[t];
}
// the lane's own record out of LDS: the empty record at and behind the cut
template <class T>
SF_ST_FN void put_lane_record(const StatePut &k, int v, int lane, const int32_t *lds, typename T::Rec &o) {
  int32_t w[T::W];
  const bool in = v * 64 + lane < T::cut(k);
#pragma unroll
  for (int j = 0; j < T::W; ++j) w[j] = in ? lds[lane * T::S + j] : 0;
  __builtin_memcpy(&o, w, sizeof o);
}
// phase 2, check: the reason bit of the lane's record; alive: whether it counts (only where the check passed)
template <class T>
SF_ST_FN uint32_t put_lane_check(const StatePut &k, int v, int lane, const int32_t *lds, bool &alive) {
  typename T::Rec o;
  put_lane_record<T>(k, v, lane, lds, o);
  const int slot = v * 64 + lane;
  const bool ok = slot >= T::pool(k) || T::check(k.c, o);
  int32_t first;
  __builtin_memcpy(&first, &o, 4);  // alive is every record's first word
  alive = ok && slot < T::pool(k) && first != 0;
  return ok ? 0u : (uint32_t)T::BIT;
}
// phase 2, write: field f of the lane's slot into [field][arena][slot], one coalesced store per field
template <class T>
SF_ST_FN void put_lane_write(const StatePut &k, int a, int v, int lane, const int32_t *lds) {
  typename T::Rec o;
  put_lane_record<T>(k, v, lane, lds, o);
  const int slot = v * 64 + lane;
  if (slot >= T::pool(k)) return;
  uint32_t w[T::FIELDS];
  T::encode(k.c, slot, o, w);
  SF_ST_G uint32_t *dst = st_g(T::dst(k)) + ((size_t)a * (size_t)T::pool(k) + (size_t)slot);
  const size_t field = (size_t)k.A * (size_t)T::pool(k);
#pragma unroll
  for (int f = 0; f < T::FIELDS; ++f, dst += field) *dst = w[f];
}

// exits: a record is 16 bytes, one load per lane
SF_ST_FN void put_lane_portal_rec(const StatePut &k, int row, int v, int lane, sf_portal_rec &o) {
  const int slot = v * 64 + lane;
  o = sf_portal_rec{};
  if (slot >= k.io.portals) return;
  const int32_t *src = reinterpret_cast<const int32_t *>(k.io.d_portals) + ((size_t)row * (size_t)k.io.portals + (size_t)slot) * REC_P_WORDS;
  if (((uintptr_t)k.io.d_portals & 15u) == 0u) put_load16(src, o.active, o.f, o.r, o.c);
  else o.active = st_g(src)[0], o.f = st_g(src)[1], o.r = st_g(src)[2], o.c = st_g(src)[3];
}
SF_ST_FN uint32_t put_lane_portal_check(const StatePut &k, int row, int v, int lane, bool &active) {
  sf_portal_rec o;
  put_lane_portal_rec(k, row, v, lane, o);
  const int slot = v * 64 + lane;
  const bool ok = slot >= k.c.P || check_portal(k.c, o);
  active = ok && slot < k.c.P && o.active != 0;
  return ok ? 0u : (uint32_t)SF_PUT_BAD_PORTAL;
}
SF_ST_FN void put_lane_portal_write(const StatePut &k, int a, int row, int v, int lane) {
  sf_portal_rec o;
  put_lane_portal_rec(k, row, v, lane, o);
  const int slot = v * 64 + lane;
  if (slot < k.c.P) st_g(k.por)[(size_t)a * (size_t)k.c.P + (size_t)slot] = encode_portal(o);
}

// cells: chunk v is cells STATE_CELL_CHUNK v .., lane + 64 j for j < 4
SF_ST_FN uint32_t put_lane_cells_check(const StatePut &k, int row, int v, int lane) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ci = v * STATE_CELL_CHUNK + 64 * j + lane;
    if (ci >= k.c.cells) continue;
    const size_t at = (size_t)row * (size_t)k.c.cells + (size_t)ci;
    ok = ok && check_cell(k.c, st_g(k.io.d_cell_flags)[at], st_g(k.io.d_cell_dmg)[at], st_g(k.io.d_cell_portal)[at], st_g(k.map_pidx)[ci]);
  }
  return ok ? 0u : (uint32_t)SF_PUT_BAD_CELL;
}
SF_ST_FN void put_lane_cells_write(const StatePut &k, int a, int row, int v, int lane) {
  uint32_t fl[4];
  int32_t cd[4], cp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {  // every load of the chunk before the first store
    const int ci = v * STATE_CELL_CHUNK + 64 * j + lane;
    const size_t at = (size_t)row * (size_t)k.c.cells + (size_t)ci;
    const bool in = ci < k.c.cells;
    fl[j] = in ? (uint32_t)st_g(k.io.d_cell_flags)[at] : 0u;
    cd[j] = in ? st_g(k.io.d_cell_dmg)[at] : 0, cp[j] = in ? st_g(k.io.d_cell_portal)[at] : 0;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ci = v * STATE_CELL_CHUNK + 64 * j + lane;
    if (ci >= k.c.cells) continue;
    st_g(k.flags)[(size_t)a * (size_t)k.cells_pad + (size_t)ci] = (uint8_t)fl[j];
    const size_t at = (size_t)a * (size_t)k.c.cells + (size_t)ci;
    if (encode_cell_has_dmg(fl[j])) st_g(k.aux_dmg)[at] = cd[j];
    if (encode_cell_has_pidx(fl[j])) st_g(k.aux_pidx)[at] = (int16_t)cp[j];
  }
}

// the header unit.  Phase 1: the record's words into LDS; the check is lane 0's
SF_ST_FN void put_hdr_fill(const StatePut &k, int row, int lane, int32_t *lds) {
  if (k.io.d_hdr && lane < REC_HDR_WORDS) lds[lane] = st_g(reinterpret_cast<const int32_t *>(k.io.d_hdr))[(size_t)row * REC_HDR_WORDS + lane];
}
SF_ST_FN uint32_t put_hdr_check(const StatePut &k, int lane, const int32_t *lds) {
  return (k.io.d_hdr && lane == 0 && !check_hdr(lds)) ? (uint32_t)SF_PUT_BAD_HDR : 0u;
}
// phase 2, write: the scalar block (lanes below SC_WORDS), both generators (lanes below RNG_WORDS, only with a header).
// vr: the row's verdict words
SF_ST_FN void put_hdr_write(const StatePut &k, int a, int lane, const int32_t *lds, const int32_t *vr) {
  if (lane < SC_WORDS) {
    SF_ST_G int32_t *sc = st_g(k.scal) + (size_t)a * SC_WORDS + lane;
    const int32_t load = (k.io.d_humans && k.io.d_zombies) ? vr[PUT_V_HALIVE] + vr[PUT_V_ZALIVE] : -1;
    const int32_t zwn = k.io.d_zombies ? zw_for(vr[PUT_V_ZEXT]) : -1, pwn = k.io.d_portals ? zw_for(vr[PUT_V_PEXT]) : -1;
    *sc = encode_hdr_word(lane, k.io.d_hdr != nullptr, lds, *sc, load, zwn, pwn);
  }
  if (k.io.d_hdr && lane < RNG_WORDS) {
    st_g(k.rng)[(size_t)a * RNG_WORDS + lane] = encode_rng_word(lane, lds);
    st_g(k.rng2)[(size_t)a * RNG_WORDS + lane] = encode_rng2_word(k.c, lane, lds);
  }
}
// what the arena's first wavefront reports: status and selected.  go: the arena is written
SF_ST_FN void put_lane_report(const StatePut &k, int a, int lane, const PutArena &x, int32_t bits) {
  const bool go = x.row >= 0 && bits == 0;
  if (k.io.d_status && lane == 0) st_g(k.io.d_status)[a] = x.range ? (int32_t)SF_PUT_BAD_ROW : x.row < 0 ? -1 : bits;
  if (k.io.d_selected && lane < k.c.n_agents) st_g(k.io.d_selected)[(size_t)a * (size_t)k.c.n_agents + (size_t)lane] = go ? 1 : 0;
}

#if defined(__HIPCC__)
// ---- the wavefronts: grid (rows, parts) for the check, (arenas, parts) for the write; 64 threads per workgroup -------------
// unit u of a row is done by wavefront u % parts, as in k_state_records
template <class T>
SF_ST_DEV void put_table_check(const StatePut &k, int row, int part, int parts, int base, int n, int32_t *lds, uint32_t &bits, int aword, int eword) {
  const int lane = (int)threadIdx.x;
  for (int v = state_first_unit(part, base, parts); v < n; v += parts) {
    put_lane_fill<T>(k, row, v, lane, lds);
    __syncthreads();
    bool alive;
    bits |= put_lane_check<T>(k, v, lane, lds, alive);
    __syncthreads();
    const unsigned long long m = __ballot(alive);
    if (m != 0ull && lane == 0) {  // one atomic add and one atomic max per batch
      SF_ST_G int32_t *vr = st_g(k.verdict) + (size_t)row * PUT_ROW_WORDS;
      if (aword >= 0) (void)__hip_atomic_fetch_add(vr + aword, (int32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (eword >= 0) (void)__hip_atomic_fetch_max(vr + eword, (int32_t)(v * 64 + 64 - __clzll((long long)m)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
SF_ST_DEV void state_put_check_body(const StatePut &k, int row, int part, int parts) {
  __shared__ int32_t lds[PUT_LDS_WORDS];
  const int lane = (int)threadIdx.x;
  const PutUnits nu = put_units(k);
  uint32_t bits = 0u;
  if (part == 0) {
    put_hdr_fill(k, row, lane, lds);
    __syncthreads();
    bits |= put_hdr_check(k, lane, lds);
    __syncthreads();
  }
  int base = 1;
  put_table_check<PutHumans>(k, row, part, parts, base, nu.h, lds, bits, PUT_V_HALIVE, -1);
  base += nu.h;
  put_table_check<PutZombies>(k, row, part, parts, base, nu.z, lds, bits, PUT_V_ZALIVE, PUT_V_ZEXT);
  base += nu.z;
  put_table_check<PutBullets>(k, row, part, parts, base, nu.b, lds, bits, -1, -1);
  base += nu.b;
  for (int v = state_first_unit(part, base, parts); v < nu.p; v += parts) {
    bool active;
    bits |= put_lane_portal_check(k, row, v, lane, active);
    const unsigned long long m = __ballot(active);
    if (m != 0ull && lane == 0)
      (void)__hip_atomic_fetch_max(st_g(k.verdict) + (size_t)row * PUT_ROW_WORDS + PUT_V_PEXT, (int32_t)(v * 64 + 64 - __clzll((long long)m)),
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  base += nu.p;
  for (int v = state_first_unit(part, base, parts); v < nu.c; v += parts) bits |= put_lane_cells_check(k, row, v, lane);
#pragma unroll
  for (int d = 32; d; d >>= 1) bits |= (uint32_t)__shfl_xor((int)bits, d, 64);
  if (lane == 0 && bits != 0u)
    (void)__hip_atomic_fetch_or(st_g(k.verdict) + (size_t)row * PUT_ROW_WORDS + PUT_V_BITS, (int32_t)bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <class T>
SF_ST_DEV void put_table_write(const StatePut &k, int a, int row, int part, int parts, int base, int n, int32_t *lds) {
  const int lane = (int)threadIdx.x;
  for (int v = state_first_unit(part, base, parts); v < n; v += parts) {
    put_lane_fill<T>(k, row, v, lane, lds);
    __syncthreads();
    put_lane_write<T>(k, a, v, lane, lds);
    __syncthreads();
  }
}
SF_ST_DEV void state_put_write_body(const StatePut &k, int a, int part, int parts) {
  __shared__ int32_t lds[PUT_LDS_WORDS];
  const int lane = (int)threadIdx.x;
  const PutArena x = put_arena(k, a);
  int32_t vr[PUT_ROW_WORDS];
#pragma unroll
  for (int j = 0; j < PUT_ROW_WORDS; ++j) vr[j] = x.row >= 0 ? st_g(k.verdict)[(size_t)x.row * PUT_ROW_WORDS + j] : 0;
  const bool go = x.row >= 0 && vr[PUT_V_BITS] == 0;
  if (part == 0) {
    put_lane_report(k, a, lane, x, vr[PUT_V_BITS]);
    if (lane == 0 && (go || x.row >= 0 || x.range))
      (void)__hip_atomic_fetch_add(st_g(k.counters) + (go ? PUT_N_WRITTEN : x.range ? PUT_N_RANGE : PUT_N_REFUSED), 1ull, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!go) return;  // (uniform over the workgroup)
  const int row = x.row;
  const PutUnits nu = put_units(k);
  if (part == 0) {
    put_hdr_fill(k, row, lane, lds);
    __syncthreads();
    put_hdr_write(k, a, lane, lds, vr);
    __syncthreads();
  }
  int base = 1;
  put_table_write<PutHumans>(k, a, row, part, parts, base, nu.h, lds);
  base += nu.h;
  put_table_write<PutZombies>(k, a, row, part, parts, base, nu.z, lds);
  base += nu.z;
  put_table_write<PutBullets>(k, a, row, part, parts, base, nu.b, lds);
  base += nu.b;
  for (int v = state_first_unit(part, base, parts); v < nu.p; v += parts) put_lane_portal_write(k, a, row, v, lane);
  base += nu.p;
  for (int v = state_first_unit(part, base, parts); v < nu.c; v += parts) put_lane_cells_write(k, a, row, v, lane);
}
#endif  // __HIPCC__

}  // namespace sf
