// sf_state_records.hpp — the canonical state records of strikeforce.h (sf_arena_hdr, sf_human_rec, sf_zombie_rec,
// sf_bullet_rec, sf_portal_rec, the three per-cell tables) and the state digest, decoded from the packed state words of
// sf_types.hpp.  One text for two users:
//   - the host's Env::decode() / Env::digest_of() (sf_host.hpp), behind sf_dump_arena and sf_state_digest: one arena at a
//     time from a host copy of the state;
//   - k_state_records (sf_api.hip), behind sf_state_device: every arena at once where the state lives.
// The per-record functions below are SF_HD and take the packed words by value, so both compile them; the existing dump and
// digest tests pin them to the oracle, and the kernel adds only the traversal and the stores (state_records_body, below).
//
// Nothing of the environment is written by anything in this file.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/strikeforce.h"
#include "sf_types.hpp"

namespace sf {

// splitmix64 finalizer; the digest is an order-independent sum of per-item hashes
SF_HD inline uint64_t mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ULL;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebULL;
  x ^= x >> 31;
  return x;
}
SF_HD inline uint64_t dg(uint64_t tag, uint64_t idx, int64_t v) {
  return mix64((tag << 56) ^ (idx << 32) ^ (uint64_t)(uint32_t)v ^ ((uint64_t)(v >> 32) << 40));
}

// the records as int32 words (every record but the header is int32 fields only; the header's int64 fields are two words
// each, low word first: gfx950 and every host this builds for are little-endian)
enum { REC_HDR_WORDS = 40, REC_H_WORDS = 28, REC_Z_WORDS = 7, REC_B_WORDS = 11, REC_P_WORDS = 4 };
static_assert(sizeof(sf_arena_hdr) == 4 * REC_HDR_WORDS && sizeof(sf_human_rec) == 4 * REC_H_WORDS, "record layout");
static_assert(sizeof(sf_zombie_rec) == 4 * REC_Z_WORDS && sizeof(sf_bullet_rec) == 4 * REC_B_WORDS, "record layout");
static_assert(sizeof(sf_portal_rec) == 4 * REC_P_WORDS, "record layout");
static_assert(offsetof(sf_arena_hdr, rng) == 80 && offsetof(sf_arena_hdr, done) == 152, "header layout");
static_assert(SC_FRAME == 0 && SC_KILLS == 1 && SC_TKILLS == 2 && SC_LOOT == 3 && SC_CHESTS == 4 && SC_JOMLE == 5,
              "hdr_word takes the first six header fields from the scalar block's first six words");

// ---- the decoders: packed words -> one record -------------------------------------------------------------------------
// word j of arena's sf_arena_hdr from its scalar block `sc` ([SC_WORDS]) and generator registers `rng` ([RNG_WORDS]).
// SP / RP: anything indexable (the kernel passes global-address-space pointers)
template <class SP, class RP>
SF_HD inline int32_t hdr_word(int j, SP sc, RP rng) {
  if (j >= 38) return (int32_t)sc[j == 38 ? SC_DONE : SC_OUTCOME];
  if (j >= 20) return (int32_t)((uint32_t)rng[j - 20] & 0xfffffu);
  const int f = j >> 1;  // frame, kills, teams_kills, loot, chests, jomle, tb, serial, steps, episodes
  const int lo = f < 6 ? f : f == 6 ? SC_TB_LO : f == 7 ? SC_SR_LO : f == 8 ? SC_STEPS : SC_EPISODES;
  if (!(j & 1)) return (int32_t)sc[lo];
  if (f == 6) return (int32_t)sc[SC_TB_HI];
  if (f == 7) return (int32_t)sc[SC_SR_HI];
  if (f == 5) return 0;                 // jomle is the unsigned 32-bit count (random.hpp:29)
  return (int32_t)sc[lo] >> 31;         // the others are int32 values in an int64 field
}

// w: the HW_WORDS packed words of one human slot
SF_HD inline void decode_human(const uint32_t *w, sf_human_rec &o) {
  o = sf_human_rec{};
  const uint32_t fl = w[HW_FLAGS], q = w[HW_POS], bp = w[HW_BPK];
  const bool placed = (fl & (HF_ALIVE | HF_OCC)) || w[HW_HP] || (fl & HF_WAY_MASK);
  o.alive = !!(fl & HF_ALIVE), o.remote = !!(fl & HF_REMOTE), o.rnpc = !!(fl & HF_RNPC), o.profile = !!(fl & HF_PROF);
  if (placed && q != POS_NONE) o.f = pos_f(q), o.r = pos_r(q), o.c = pos_c(q);
  o.way = (int)(fl & HF_WAY_MASK), o.team = (int)((fl >> HF_TEAM_SH) & 255u);
  o.hp = (int32_t)w[HW_HP], o.stamina = (int32_t)w[HW_STAMINA], o.mindamage = (int32_t)w[HW_MINDAMAGE];
  o.kills = (int32_t)w[HW_KILLS], o.damage = (int32_t)w[HW_DAMAGE], o.effect = (int32_t)w[HW_EFFECT];
  const bool made = (fl & HF_WAY_MASK) != 0;  // slots never used stay all-zero, like the oracle's memset
  o.vec = made ? (int)((fl >> HF_VEC_SH) & 3u) - 1 : 0, o.ind = made ? (int)((fl >> HF_IND_SH) & 15u) - 1 : 0;
  o.cons[0] = w[HW_CONS01] & 0xffff, o.cons[1] = w[HW_CONS01] >> 16, o.cons[2] = w[HW_CONS23] & 0xffff,
  o.cons[3] = w[HW_CONS23] >> 16;
  o.throw_cnt[0] = w[HW_THR01] & 0xffff, o.throw_cnt[1] = w[HW_THR01] >> 16, o.throw_cnt[2] = w[HW_THR23] & 0xffff,
  o.throw_cnt[3] = w[HW_THR23] >> 16;
  o.blocks = bp & 255u, o.portals = (bp >> 8) & 255u, o.portal_ind = made ? (int)((bp >> 16) & 255u) - 1 : 0;
}
SF_HD inline void decode_zombie(uint32_t zp, uint32_t hp, uint32_t mindamage, sf_zombie_rec &o) {
  o = sf_zombie_rec{};
  if (!(zp & ZF_ALIVE)) return;
  o.alive = 1, o.f = pos_f(zp), o.r = pos_r(zp), o.c = pos_c(zp);
  o.hp = (int32_t)hp, o.mindamage = (int32_t)mindamage, o.super_ = !!(zp & ZF_SUPER);
}
SF_HD inline void decode_bullet(uint32_t ba, uint32_t damage, uint32_t bb, uint32_t bc, sf_bullet_rec &o) {
  o = sf_bullet_rec{};
  if (!(ba & BA_ALIVE)) return;
  o.alive = 1, o.f = pos_f(ba), o.r = pos_r(ba), o.c = pos_c(ba);
  o.way = (int)((ba >> BA_WAY_SH) & 3u) + 1, o.traveled = (int)(bc >> 16);
  o.damage = (int32_t)damage, o.effect = (int32_t)(int16_t)(bb & 0xffffu);
  o.range = (int)(bc & 0xffffu), o.owner = (int)(bb >> 16), o.ref = !!(ba & BA_REF);
}
SF_HD inline void decode_portal(uint32_t pp, sf_portal_rec &o) {
  o = sf_portal_rec{};
  if (!(pp & PF_ACTIVE)) return;
  o.active = 1, o.f = pos_f(pp), o.r = pos_r(pp), o.c = pos_c(pp);
}
// the two derived per-cell tables.  aux_dmg / aux_pidx: the side tables' entries (valid only under SF_CELL_TEMP; pass
// anything elsewhere), map_pidx: the map's own exit number of the cell
SF_HD inline int32_t cell_dmg_of(uint32_t fl, int32_t aux_dmg) { return (fl & SF_CELL_TEMP) ? aux_dmg : 0; }
SF_HD inline int32_t cell_portal_of(uint32_t fl, int32_t aux_pidx, int32_t map_pidx) {
  int32_t v = -1;
  if (fl & (SF_CELL_PIN_UP | SF_CELL_PIN_DN)) v = (fl & SF_CELL_TEMP) ? aux_pidx : map_pidx;
  return v;
}

// ---- the digest's terms -----------------------------------------------------------------------------------------------
enum { DG_HDR_TERMS = 27 };  // nine header fields under tag 1, the eighteen generator words under tag 2
// term j of the header's share, from the header's REC_HDR_WORDS words `hw`
template <class WP>
SF_HD inline uint64_t digest_hdr_term(int j, WP hw) {
  if (j >= 9) return dg(2, (uint64_t)(j - 9), (int64_t)(int32_t)hw[20 + (j - 9)]);
  if (j >= 7) return dg(1, (uint64_t)j, (int64_t)(int32_t)hw[38 + (j - 7)]);  // done, outcome
  const int f = j < 6 ? j : 8;  // frame, kills, teams_kills, loot, chests, jomle | steps
  const int64_t v = (int64_t)(((uint64_t)(uint32_t)hw[2 * f + 1] << 32) | (uint64_t)(uint32_t)hw[2 * f]);
  return dg(1, (uint64_t)j, v);
}
// record i of a table: TAG 3 / 4 / 5 / 6 and index stride 32 / 8 / 16 / 4 for humans / zombies / bullets / exits; the zero
// words of an empty slot count like any other
template <int TAG, int STRIDE, int W, class WP>
SF_HD inline uint64_t digest_rec(int i, WP w) {
  uint64_t d = 0;
#pragma unroll
  for (int k = 0; k < W; ++k) d += dg((uint64_t)TAG, (uint64_t)(i * STRIDE + k), (int64_t)(int32_t)w[k]);
  return d;
}
SF_HD inline uint64_t digest_human(int i, const sf_human_rec &o) { return digest_rec<3, 32, REC_H_WORDS>(i, (const int32_t *)&o); }
SF_HD inline uint64_t digest_zombie(int i, const sf_zombie_rec &o) { return digest_rec<4, 8, REC_Z_WORDS>(i, (const int32_t *)&o); }
SF_HD inline uint64_t digest_bullet(int i, const sf_bullet_rec &o) { return digest_rec<5, 16, REC_B_WORDS>(i, (const int32_t *)&o); }
SF_HD inline uint64_t digest_portal(int i, const sf_portal_rec &o) { return digest_rec<6, 4, REC_P_WORDS>(i, (const int32_t *)&o); }
// cell ci of the three cell tables: zero flags, zero damage and "no entrance" add nothing
SF_HD inline uint64_t digest_cell(int ci, uint32_t cf, int32_t cd, int32_t cp) {
  uint64_t d = 0;
  if (cf) d += dg(7, (uint64_t)ci, (int64_t)cf);
  if (cd) d += dg(8, (uint64_t)ci, (int64_t)cd);
  if (cp != -1) d += dg(9, (uint64_t)ci, (int64_t)cp);
  return d;
}

// ---- sf_state_device: what k_state_records takes, by value in the kernel arguments ---------------------------------------
// A struct of its own, like ResetSel, Snap and Signals: Params stays as it is.  `io` is the caller's struct with rows
// resolved (arenas where d_arena_ids is null).
constexpr int STATE_CELL_CHUNK = 256;  // cells one work unit covers: four per lane
struct StateRec {
  const uint32_t *hum, *zom, *bul, *por, *rng;  // Params::hum, zom, bul, por, rng
  const int32_t *scal;                          // Params::scal
  const uint8_t *flags;                         // Params::flags [A][cells_pad]
  const int32_t *aux_dmg;                       // Params::aux_dmg [A][cells]
  const int16_t *aux_pidx, *map_pidx;           // Params::aux_pidx [A][cells], Params::map_pidx [cells]
  int32_t A, H, Z, B, P, cells, cells_pad;
  int32_t parts;                                // wavefronts per row (grid.y)
  sf_state_io io;
};

// Work units of one row, in this order: the header, then 64-slot batches of humans, zombies, bullets, exits, then chunks
// of STATE_CELL_CHUNK cells.  A table is walked over its whole pool when the digest or the counts are asked for (both are
// taken over the whole pools), else up to the caller's cut, else not at all.
struct StateUnits {
  int32_t h, z, b, p, c;  // batches / chunks
  SF_HD int total() const { return 1 + h + z + b + p + c; }
};
SF_HD inline StateUnits state_units(const StateRec &k) {
  const bool whole = k.io.d_digest || k.io.d_counts;
  auto batches = [&](int pool, const void *out, int cut) { return ((whole ? pool : out ? cut : 0) + 63) / 64; };
  StateUnits u;
  u.h = batches(k.H, k.io.d_humans, k.io.humans), u.z = batches(k.Z, k.io.d_zombies, k.io.zombies);
  u.b = batches(k.B, k.io.d_bullets, k.io.bullets), u.p = batches(k.P, k.io.d_portals, k.io.portals);
  u.c = (k.io.d_digest || k.io.d_cell_flags || k.io.d_cell_dmg || k.io.d_cell_portal) ? (k.cells + STATE_CELL_CHUNK - 1) / STATE_CELL_CHUNK : 0;
  return u;
}
// wavefronts per row: enough of them to fill the chip at a small row count, and at most 32 units each for the big worlds
// (the native one has 9000-slot pools: some 460 units), the way k_snapshot splits its rows (snap_parts_for).  Measured at
// 4096 rows of configs[2] (21 units a row): four times as many, shorter wavefronts are no faster
inline int state_parts_for(int units, int rows) {
  int n = (8192 + rows - 1) / rows;
  if (n < (units + 31) / 32) n = (units + 31) / 32;
  if (n > 64) n = 64;
  if (n > units) n = units;
  return n < 1 ? 1 : n;
}

// ---- the traversal, one lane at a time --------------------------------------------------------------------------------------
// What one lane of the wavefront does in each phase of a work unit, as plain functions of (row, unit, lane): the kernel
// calls them with its own lane and a barrier between the phases; the tests' stand-alone program
// (tests/state_records/state_main.cpp) calls them for lanes 0..63 in a loop, a phase at a time, over heap buffers of
// exactly the documented sizes.  Both compile this text.
#if defined(__HIPCC__)
#define SF_ST_FN static __host__ __device__ __forceinline__
#else
#define SF_ST_FN static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define SF_ST_G __attribute__((address_space(1)))
template <class T>
SF_ST_FN const SF_ST_G T *st_g(const T *p) { return (const SF_ST_G T *)p; }
template <class T>
SF_ST_FN SF_ST_G T *st_g(T *p) { return (SF_ST_G T *)p; }
typedef int32_t st_i32x4 __attribute__((ext_vector_type(4)));
// 16 bytes at a 16-byte aligned address
SF_ST_FN void st_store16(int32_t *p, int32_t x, int32_t y, int32_t z, int32_t w) {
  st_i32x4 v;
  v.x = x, v.y = y, v.z = z, v.w = w;
  *reinterpret_cast<SF_ST_G st_i32x4 *>(st_g(p)) = v;
}
#else
#define SF_ST_G
template <class T>
SF_ST_FN T *st_g(T *p) { return p; }
SF_ST_FN void st_store16(int32_t *p, int32_t x, int32_t y, int32_t z, int32_t w) { p[0] = x, p[1] = y, p[2] = z, p[3] = w; }
#endif

// The three tables that are transposed through LDS.  S: the LDS row stride in words, odd, so that the 64 lanes' ds_write of
// word j of their own record (address lane * S + j) fall into 32 different banks per 32-lane half; 7 and 11 are odd as
// they are, 28 becomes 29.
struct StHumans {
  typedef sf_human_rec Rec;
  enum { W = REC_H_WORDS, S = REC_H_WORDS + 1, FIELDS = HW_WORDS, COUNT = 0 };
  SF_ST_FN const uint32_t *src(const StateRec &k) { return k.hum; }
  SF_ST_FN int pool(const StateRec &k) { return k.H; }
  SF_ST_FN int cut(const StateRec &k) { return k.io.humans; }
  SF_ST_FN int32_t *out(const StateRec &k) { return reinterpret_cast<int32_t *>(k.io.d_humans); }
  SF_ST_FN void decode(const uint32_t *w, Rec &o) { decode_human(w, o); }
  SF_ST_FN uint64_t digest(int i, const Rec &o) { return digest_human(i, o); }
};
struct StZombies {
  typedef sf_zombie_rec Rec;
  enum { W = REC_Z_WORDS, S = REC_Z_WORDS, FIELDS = ZW_WORDS, COUNT = 1 };
  SF_ST_FN const uint32_t *src(const StateRec &k) { return k.zom; }
  SF_ST_FN int pool(const StateRec &k) { return k.Z; }
  SF_ST_FN int cut(const StateRec &k) { return k.io.zombies; }
  SF_ST_FN int32_t *out(const StateRec &k) { return reinterpret_cast<int32_t *>(k.io.d_zombies); }
  SF_ST_FN void decode(const uint32_t *w, Rec &o) { decode_zombie(w[ZW_POS], w[ZW_HP], w[ZW_MINDAMAGE], o); }
  SF_ST_FN uint64_t digest(int i, const Rec &o) { return digest_zombie(i, o); }
};
struct StBullets {
  typedef sf_bullet_rec Rec;
  enum { W = REC_B_WORDS, S = REC_B_WORDS, FIELDS = BW_WORDS, COUNT = 2 };
  SF_ST_FN const uint32_t *src(const StateRec &k) { return k.bul; }
  SF_ST_FN int pool(const StateRec &k) { return k.B; }
  SF_ST_FN int cut(const StateRec &k) { return k.io.bullets; }
  SF_ST_FN int32_t *out(const StateRec &k) { return reinterpret_cast<int32_t *>(k.io.d_bullets); }
  SF_ST_FN void decode(const uint32_t *w, Rec &o) { decode_bullet(w[BW_A], w[BW_DAMAGE], w[BW_B], w[BW_C], o); }
  SF_ST_FN uint64_t digest(int i, const Rec &o) { return digest_bullet(i, o); }
};
constexpr int ST_LDS_WORDS = 64 * StHumans::S;

// the row a wavefront works on: the arena it shows and whether its id is in range.  An id out of range never becomes an
// address: the row reads arena 0 and stores zeros
struct StateRow {
  size_t a;
  int32_t row;
  bool ok;
};
SF_ST_FN StateRow state_row(const StateRec &k, int row) {
  const int id = k.io.d_arena_ids ? st_g(k.io.d_arena_ids)[row] : row;
  StateRow r;
  r.ok = id >= 0 && id < k.A, r.a = r.ok ? (size_t)id : 0u, r.row = row;
  return r;
}
// the first unit of a kind that is wavefront `part`'s: units are numbered over all kinds (base: the kind's first), and
// unit u is done by wavefront u % parts
SF_ST_FN int state_first_unit(int part, int base, int parts) {
  const int v = (part - base) % parts;
  return v < 0 ? v + parts : v;
}

// k_state_init: the rows the wavefronts of k_state_records add into
SF_ST_FN void state_init_body(const sf_state_io &io, int i) {
  if (io.d_digest) st_g(io.d_digest)[i] = 0ull;
  if (io.d_counts) {
#pragma unroll
    for (int j = 0; j < SF_STATE_COUNT_WORDS; ++j) st_g(io.d_counts)[(size_t)i * SF_STATE_COUNT_WORDS + j] = 0;
  }
}

// ---- the header: phase 1 puts the record's words into LDS, phase 2 takes the digest terms and stores
SF_ST_FN void st_hdr_words(const StateRec &k, const StateRow &r, int lane, int32_t *lds) {
  if (lane < REC_HDR_WORDS) lds[lane] = hdr_word(lane, st_g(k.scal) + r.a * SC_WORDS, st_g(k.rng) + r.a * RNG_WORDS);
}
SF_ST_FN void st_hdr_out(const StateRec &k, const StateRow &r, int lane, const int32_t *lds, uint64_t &sum) {
  if (k.io.d_digest && r.ok && lane < DG_HDR_TERMS) sum += digest_hdr_term(lane, lds);
  if (k.io.d_hdr && lane < REC_HDR_WORDS)
    st_g(reinterpret_cast<int32_t *>(k.io.d_hdr))[(size_t)r.row * REC_HDR_WORDS + lane] = r.ok ? lds[lane] : 0;
  if (k.io.d_counts && !r.ok && lane < SF_STATE_COUNT_WORDS) st_g(k.io.d_counts)[(size_t)r.row * SF_STATE_COUNT_WORDS + lane] = -1;
}

// ---- humans, zombies, bullets: batch v is slots 64 v .. 64 v + 63, one per lane.
// whether batch v of table T goes to the caller's buffer
template <class T>
SF_ST_FN bool st_batch_stored(const StateRec &k, int v) { return T::out(k) != nullptr && v * 64 < T::cut(k); }
// phase 1: the slot's packed words (every load issued before the first use), its record, its digest terms, the record
// into LDS for the transpose; returns whether the slot is alive
template <class T>
SF_ST_FN bool st_lane_decode(const StateRec &k, const StateRow &r, int v, int lane, int32_t *lds, uint64_t &sum) {
  const int slot = v * 64 + lane;
  const bool in = slot < T::pool(k);
  uint32_t w[T::FIELDS];
  // (a running per-lane address with one field stride, not one base per field: fewer scalar registers)
  const SF_ST_G uint32_t *src = st_g(T::src(k)) + (r.a * (size_t)T::pool(k) + (size_t)slot);
  const size_t field = (size_t)k.A * (size_t)T::pool(k);
#pragma unroll
  for (int f = 0; f < T::FIELDS; ++f, src += field) w[f] = in ? *src : 0u;
  typename T::Rec o;
  T::decode(w, o);
  if (k.io.d_digest && r.ok && in) sum += T::digest(slot, o);
  if (st_batch_stored<T>(k, v)) {
    int32_t ow[T::W];
    __builtin_memcpy(ow, &o, sizeof o);
#pragma unroll
    for (int j = 0; j < T::W; ++j) lds[lane * T::S + j] = ow[j];
  }
  return in && o.alive != 0;
}
// phase 2: the batch's records out of LDS (record s at lds + s * S) to the caller's table, coalesced: dwords up to the
// first 16-byte boundary, 16 bytes per lane from there, dwords for the tail
template <class T>
SF_ST_FN void st_lane_store(const StateRec &k, const StateRow &r, int v, int lane, const int32_t *lds) {
  if (!st_batch_stored<T>(k, v)) return;
  const int slot0 = v * 64, n = T::cut(k) - slot0 < 64 ? T::cut(k) - slot0 : 64, cnt = n * T::W;
  int32_t *out = T::out(k) + ((size_t)r.row * (size_t)T::cut(k) + (size_t)slot0) * T::W;
  auto L = [&](int g) { return r.ok ? lds[(g / T::W) * T::S + g % T::W] : 0; };
  int head = (int)((4u - (unsigned)((uintptr_t)out >> 2)) & 3u);
  head = head < cnt ? head : cnt;
  if (lane < head) st_g(out)[lane] = L(lane);
  const int nvec = (cnt - head) >> 2;
  for (int q = lane; q < nvec; q += 64) {
    const int g = head + 4 * q;
    st_store16(out + g, L(g), L(g + 1), L(g + 2), L(g + 3));
  }
  const int t = head + 4 * nvec + lane;
  if (t < cnt) st_g(out)[t] = L(t);
}

// ---- exits: a record is exactly 16 bytes, one per lane, no transpose; returns whether the slot is active
SF_ST_FN bool st_lane_portal(const StateRec &k, const StateRow &r, int v, int lane, uint64_t &sum) {
  const int slot = v * 64 + lane;
  const bool in = slot < k.P;
  const uint32_t pp = in ? st_g(k.por)[r.a * (size_t)k.P + (size_t)slot] : 0u;
  sf_portal_rec o;
  decode_portal(pp, o);
  if (k.io.d_digest && r.ok && in) sum += digest_portal(slot, o);
  if (k.io.d_portals && slot < k.io.portals) {
    int32_t *dst = reinterpret_cast<int32_t *>(k.io.d_portals) + ((size_t)r.row * (size_t)k.io.portals + (size_t)slot) * REC_P_WORDS;
    const int32_t x = r.ok ? o.active : 0, y = r.ok ? o.f : 0, z = r.ok ? o.r : 0, w = r.ok ? o.c : 0;
    if (((uintptr_t)k.io.d_portals & 15u) == 0u) st_store16(dst, x, y, z, w);
    else st_g(dst)[0] = x, st_g(dst)[1] = y, st_g(dst)[2] = z, st_g(dst)[3] = w;
  }
  return in && o.active != 0;
}

// ---- cells: chunk v is cells STATE_CELL_CHUNK v .., lane + 64 j for j < 4; byte and dword streams, every load of the
// chunk issued before the first use.  The side tables are read only where the flags say they are valid
SF_ST_FN void st_lane_cells(const StateRec &k, const StateRow &r, int v, int lane, uint64_t &sum) {
  const int c0 = v * STATE_CELL_CHUNK;
  uint32_t fl[4];
  int32_t dm[4], ax[4], mp[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ci = c0 + 64 * j + lane;
    fl[j] = ci < k.cells ? (uint32_t)st_g(k.flags)[r.a * (size_t)k.cells_pad + (size_t)ci] : 0u;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ci = c0 + 64 * j + lane;  // (fl is 0 beyond the last cell: nothing below loads there)
    const bool temp = (fl[j] & SF_CELL_TEMP) != 0u, pin = (fl[j] & (SF_CELL_PIN_UP | SF_CELL_PIN_DN)) != 0u;
    dm[j] = temp ? st_g(k.aux_dmg)[r.a * (size_t)k.cells + (size_t)ci] : 0;
    ax[j] = temp && pin ? (int32_t)st_g(k.aux_pidx)[r.a * (size_t)k.cells + (size_t)ci] : 0;
    mp[j] = !temp && pin ? (int32_t)st_g(k.map_pidx)[ci] : 0;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ci = c0 + 64 * j + lane;
    if (ci >= k.cells) continue;
    const int32_t cd = cell_dmg_of(fl[j], dm[j]), cp = cell_portal_of(fl[j], ax[j], mp[j]);
    if (k.io.d_digest && r.ok) sum += digest_cell(ci, fl[j], cd, cp);
    const size_t at = (size_t)r.row * (size_t)k.cells + (size_t)ci;
    if (k.io.d_cell_flags) st_g(k.io.d_cell_flags)[at] = r.ok ? (uint8_t)fl[j] : (uint8_t)0;
    if (k.io.d_cell_dmg) st_g(k.io.d_cell_dmg)[at] = r.ok ? cd : 0;
    if (k.io.d_cell_portal) st_g(k.io.d_cell_portal)[at] = r.ok ? cp : 0;
  }
}

#if defined(__HIPCC__)
#define SF_ST_DEV static __device__ __forceinline__
// ---- the wavefront: the units `part`, `part + parts`, ... of row `row`.  64 threads per workgroup -----------------------
// alive count and extent of one 64-slot batch, from the lanes' alive bits: one atomic add and one atomic max per batch
SF_ST_DEV void st_count(const StateRec &k, const StateRow &r, int word, bool alive, int slot0) {
  const unsigned long long m = __ballot(alive);
  if (k.io.d_counts && r.ok && m != 0ull && threadIdx.x == 0) {
    SF_ST_G int32_t *c = st_g(k.io.d_counts) + (size_t)r.row * SF_STATE_COUNT_WORDS;
    (void)__hip_atomic_fetch_add(c + word, (int32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    (void)__hip_atomic_fetch_max(c + 4 + word, (int32_t)(slot0 + 64 - __clzll((long long)m)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
template <class T>
SF_ST_DEV void st_table(const StateRec &k, const StateRow &r, int part, int base, int n, int32_t *lds, uint64_t &sum) {
  const int lane = (int)threadIdx.x;
  for (int v = state_first_unit(part, base, k.parts); v < n; v += k.parts) {
    const bool alive = st_lane_decode<T>(k, r, v, lane, lds, sum);
    st_count(k, r, T::COUNT, alive, v * 64);
    if (st_batch_stored<T>(k, v)) {
      __syncthreads();
      st_lane_store<T>(k, r, v, lane, lds);
      __syncthreads();
    }
  }
}
// One loop per kind, so that only that kind's pointers are live in it
SF_ST_DEV void state_records_body(const StateRec &k, int row, int part) {
  __shared__ int32_t lds[ST_LDS_WORDS];
  const int lane = (int)threadIdx.x;
  const StateRow r = state_row(k, row);
  const StateUnits nu = state_units(k);
  uint64_t sum = 0;
  if (part == 0) {  // unit 0
    st_hdr_words(k, r, lane, lds);
    __syncthreads();
    st_hdr_out(k, r, lane, lds, sum);
    __syncthreads();
  }
  int base = 1;
  st_table<StHumans>(k, r, part, base, nu.h, lds, sum);
  base += nu.h;
  st_table<StZombies>(k, r, part, base, nu.z, lds, sum);
  base += nu.z;
  st_table<StBullets>(k, r, part, base, nu.b, lds, sum);
  base += nu.b;
  for (int v = state_first_unit(part, base, k.parts); v < nu.p; v += k.parts)
    st_count(k, r, 3, st_lane_portal(k, r, v, lane, sum), v * 64);
  base += nu.p;
  for (int v = state_first_unit(part, base, k.parts); v < nu.c; v += k.parts) st_lane_cells(k, r, v, lane, sum);
  if (k.io.d_digest && r.ok) {  // per-lane sums -> one sum per wavefront -> one 64-bit add into the row k_state_init zeroed
#pragma unroll
    for (int d = 32; d; d >>= 1) sum += (uint64_t)__shfl_xor((unsigned long long)sum, d, 64);
    if (lane == 0 && sum != 0ull)
      (void)__hip_atomic_fetch_add(st_g(reinterpret_cast<unsigned long long *>(k.io.d_digest)) + row, (unsigned long long)sum, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
  }
}
#endif  // __HIPCC__

}  // namespace sf
