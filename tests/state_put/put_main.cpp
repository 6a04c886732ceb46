// put_main.cpp — the lane functions of csrc/sf_state_put.hpp (the text k_put_check / k_put_write compile) on the
// CPU, as a stand-alone program: tests/test_state_put_cpu.py builds it plain and with -fsanitize=address,undefined.
//
//   put_main <records file> <packed state out>
//
// The file holds rows of canonical records and the configuration (layout: test_state_put_cpu.py write_rows).  Row i is put
// into arena i of a destination that is filled with a pattern first.  The program walks the work units as the kernels do
// — wavefront `part` of `parts` takes the units u % parts == part, the lanes 0..63 of a phase in a loop, LDS refilled with
// garbage between units — over heap buffers of exactly the documented sizes, for every subset of the parts x cuts
// 0 / 1 / cap-1 / cap x 1 / 3 / 64 wavefronts per row.  After each run it decodes the destination with the decoders of
// sf_state_records.hpp and compares with the input (cut applied); parts that were not given must still hold the pattern.
// It also holds every check predicate at its last good and first bad value.  The full put's packed state goes to the output
// file for the comparison with state_records_ref.encode().  Last line: "put_main ok <runs>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../strikeforce_amd/csrc/sf_state_put.hpp"

using namespace sf;

#define REQUIRE(c)                                                       \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::printf("put_main: line %d: %s\n", __LINE__, #c);              \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

template <class T>
struct Heap {  // exactly n elements on the heap: a sanitized build sees the first byte outside
  std::unique_ptr<T[]> p;
  size_t n = 0;
  void make(size_t count, int pattern) {
    n = count, p.reset(new T[count ? count : 1]);
    std::memset(p.get(), pattern, (count ? count : 1) * sizeof(T));
  }
  T *get() { return n ? p.get() : nullptr; }
};

struct Rows {
  int32_t A;
  PutCfg c;
  int32_t cells_pad;
  std::vector<int32_t> hdr, hum, zom, bul, por, dmg, pidx;
  std::vector<uint8_t> fl;
  std::vector<int16_t> map_pidx;
};
static Rows read_rows(const char *path) {
  FILE *f = std::fopen(path, "rb");
  REQUIRE(f);
  int32_t h[16];
  REQUIRE(std::fread(h, 4, 16, f) == 16);
  Rows r;
  r.A = h[0], r.cells_pad = h[6];
  r.c = PutCfg{h[7], h[8], h[9], h[1], h[2], h[3], h[4], h[5], h[10], h[11], h[12], h[13], h[14], h[15]};
  auto rd = [&](auto &v, size_t n) {
    v.resize(n);
    REQUIRE(n == 0 || std::fread(v.data(), sizeof v[0], n, f) == n);
  };
  const size_t A = (size_t)r.A, C = (size_t)r.c.cells;
  rd(r.hdr, A * 40), rd(r.hum, A * r.c.H * 28), rd(r.zom, A * r.c.Z * 7), rd(r.bul, A * r.c.B * 11), rd(r.por, A * r.c.P * 4);
  rd(r.fl, A * C), rd(r.dmg, A * C), rd(r.pidx, A * C), rd(r.map_pidx, C);
  std::fclose(f);
  return r;
}

struct Dest {
  Heap<uint32_t> hum, zom, bul, por, rng, rng2;
  Heap<int32_t> scal, aux_dmg, verdict, status;
  Heap<uint8_t> flags, selected;
  Heap<int16_t> aux_pidx;
  Heap<unsigned long long> counters;
};
static const int PATTERN = 0x5B;
static const uint32_t PW = 0x5B5B5B5Bu;

static void garbage(int32_t *lds, unsigned &seed) {
  for (int i = 0; i < PUT_LDS_WORDS; ++i) lds[i] = (int32_t)(seed = seed * 1664525u + 1013904223u);
}

// one call as the three kernels make it
template <class T>
static void table_check(const StatePut &k, int row, int part, int parts, int base, int n, int32_t *lds, uint32_t &bits, int aword, int eword, unsigned &seed) {
  for (int v = state_first_unit(part, base, parts); v < n; v += parts) {
    garbage(lds, seed);
    for (int l = 0; l < 64; ++l) put_lane_fill<T>(k, row, v, l, lds);
    int count = 0, ext = 0;
    for (int l = 0; l < 64; ++l) {
      bool alive;
      bits |= put_lane_check<T>(k, v, l, lds, alive);
      if (alive) ++count, ext = v * 64 + l + 1;
    }
    int32_t *vr = k.verdict + (size_t)row * PUT_ROW_WORDS;
    if (aword >= 0) vr[aword] += count;
    if (eword >= 0 && ext > vr[eword]) vr[eword] = ext;
  }
}
template <class T>
static void table_write(const StatePut &k, int a, int row, int part, int parts, int base, int n, int32_t *lds, unsigned &seed) {
  for (int v = state_first_unit(part, base, parts); v < n; v += parts) {
    garbage(lds, seed);
    for (int l = 0; l < 64; ++l) put_lane_fill<T>(k, row, v, l, lds);
    for (int l = 0; l < 64; ++l) put_lane_write<T>(k, a, v, l, lds);
  }
}
static void put_call(const StatePut &k, int parts) {
  static int32_t lds[PUT_LDS_WORDS];
  unsigned seed = 12345u;
  const PutUnits nu = put_units(k);
  for (int i = 0; i < k.io.rows; ++i) put_init_body(k, i);
  for (int row = 0; row < k.io.rows; ++row)
    for (int part = 0; part < parts; ++part) {
      uint32_t bits = 0u;
      if (part == 0) {
        garbage(lds, seed);
        for (int l = 0; l < 64; ++l) put_hdr_fill(k, row, l, lds);
        for (int l = 0; l < 64; ++l) bits |= put_hdr_check(k, l, lds);
      }
      int base = 1;
      table_check<PutHumans>(k, row, part, parts, base, nu.h, lds, bits, PUT_V_HALIVE, -1, seed);
      base += nu.h;
      table_check<PutZombies>(k, row, part, parts, base, nu.z, lds, bits, PUT_V_ZALIVE, PUT_V_ZEXT, seed);
      base += nu.z;
      table_check<PutBullets>(k, row, part, parts, base, nu.b, lds, bits, -1, -1, seed);
      base += nu.b;
      for (int v = state_first_unit(part, base, parts); v < nu.p; v += parts)
        for (int l = 0; l < 64; ++l) {
          bool active;
          bits |= put_lane_portal_check(k, row, v, l, active);
          int32_t &e = k.verdict[(size_t)row * PUT_ROW_WORDS + PUT_V_PEXT];
          if (active && v * 64 + l + 1 > e) e = v * 64 + l + 1;
        }
      base += nu.p;
      for (int v = state_first_unit(part, base, parts); v < nu.c; v += parts)
        for (int l = 0; l < 64; ++l) bits |= put_lane_cells_check(k, row, v, l);
      k.verdict[(size_t)row * PUT_ROW_WORDS + PUT_V_BITS] |= (int32_t)bits;
    }
  for (int a = 0; a < k.A; ++a)
    for (int part = 0; part < parts; ++part) {
      const PutArena x = put_arena(k, a);
      int32_t vr[PUT_ROW_WORDS] = {0};
      if (x.row >= 0) std::memcpy(vr, k.verdict + (size_t)x.row * PUT_ROW_WORDS, sizeof vr);
      const bool go = x.row >= 0 && vr[PUT_V_BITS] == 0;
      if (part == 0) {
        for (int l = 0; l < 64; ++l) put_lane_report(k, a, l, x, vr[PUT_V_BITS]);
        if (go || x.row >= 0 || x.range) ++k.counters[go ? PUT_N_WRITTEN : x.range ? PUT_N_RANGE : PUT_N_REFUSED];
      }
      if (!go) continue;
      if (part == 0) {
        garbage(lds, seed);
        for (int l = 0; l < 64; ++l) put_hdr_fill(k, x.row, l, lds);
        for (int l = 0; l < 64; ++l) put_hdr_write(k, a, l, lds, vr);
      }
      int base = 1;
      table_write<PutHumans>(k, a, x.row, part, parts, base, nu.h, lds, seed);
      base += nu.h;
      table_write<PutZombies>(k, a, x.row, part, parts, base, nu.z, lds, seed);
      base += nu.z;
      table_write<PutBullets>(k, a, x.row, part, parts, base, nu.b, lds, seed);
      base += nu.b;
      for (int v = state_first_unit(part, base, parts); v < nu.p; v += parts)
        for (int l = 0; l < 64; ++l) put_lane_portal_write(k, a, x.row, v, l);
      base += nu.p;
      for (int v = state_first_unit(part, base, parts); v < nu.c; v += parts)
        for (int l = 0; l < 64; ++l) put_lane_cells_write(k, a, x.row, v, l);
    }
}

// subset bits: 1 hdr, 2 humans, 4 zombies, 8 bullets, 16 exits, 32 cells.  cut: slots of every table given
static void run(const Rows &r, int subset, int cutsel, int parts, Dest &d, bool verify = true) {
  const PutCfg &c = r.c;
  const size_t A = (size_t)r.A, C = (size_t)c.cells;
  d.hum.make(HW_WORDS * A * c.H, PATTERN), d.zom.make(ZW_WORDS * A * c.Z, PATTERN), d.bul.make(BW_WORDS * A * c.B, PATTERN);
  d.por.make(A * c.P, PATTERN), d.rng.make(A * RNG_WORDS, PATTERN), d.rng2.make(A * RNG_WORDS, PATTERN), d.scal.make(A * SC_WORDS, PATTERN);
  d.flags.make(A * (size_t)r.cells_pad, PATTERN), d.aux_dmg.make(A * C, PATTERN), d.aux_pidx.make(A * C, PATTERN);
  d.verdict.make(A * PUT_ROW_WORDS, 0x77), d.status.make(A, 0x77), d.selected.make(A * c.n_agents, 0x77), d.counters.make(PUT_COUNTERS, 0);
  auto cut = [&](int cap) { return cutsel == 0 ? 0 : cutsel == 1 ? (cap < 1 ? cap : 1) : cutsel == 2 ? (cap > 0 ? cap - 1 : 0) : cap; };
  const int ch = cut(c.H), cz = cut(c.Z), cb = cut(c.B), cp = cut(c.P);
  // the caller's tables cut to [rows][cut], exact size
  auto slice = [&](const std::vector<int32_t> &all, int cap, int n, int W, Heap<int32_t> &out) {
    out.make(A * (size_t)n * W + 1, 0);  // (+ 1: a table of 0 slots still has an address)
    for (size_t a = 0; a < A; ++a)
      for (int s = 0; s < n; ++s) std::memcpy(out.p.get() + (a * n + s) * W, all.data() + (a * cap + s) * W, (size_t)W * 4);
  };
  Heap<int32_t> th, tz, tb, tp, map;
  slice(r.hum, c.H, ch, 28, th), slice(r.zom, c.Z, cz, 7, tz), slice(r.bul, c.B, cb, 11, tb), slice(r.por, c.P, cp, 4, tp);
  map.make(A, 0);
  for (size_t a = 0; a < A; ++a) map.p[a] = (int32_t)a;
  StatePut k;
  std::memset(&k, 0, sizeof k);
  k.hum = d.hum.get(), k.zom = d.zom.get(), k.bul = d.bul.get(), k.por = d.por.get(), k.rng = d.rng.get(), k.rng2 = d.rng2.get();
  k.scal = d.scal.get(), k.flags = d.flags.get(), k.aux_dmg = d.aux_dmg.get(), k.aux_pidx = d.aux_pidx.get(), k.map_pidx = r.map_pidx.data();
  k.verdict = d.verdict.get(), k.counters = d.counters.get();
  k.A = r.A, k.cells_pad = r.cells_pad, k.c = c;
  k.io.d_row_of_arena = map.get(), k.io.rows = r.A, k.io.humans = ch, k.io.zombies = cz, k.io.bullets = cb, k.io.portals = cp;
  if (subset & 1) k.io.d_hdr = reinterpret_cast<const sf_arena_hdr *>(r.hdr.data());
  if (subset & 2) k.io.d_humans = reinterpret_cast<const sf_human_rec *>(th.p.get());
  if (subset & 4) k.io.d_zombies = reinterpret_cast<const sf_zombie_rec *>(tz.p.get());
  if (subset & 8) k.io.d_bullets = reinterpret_cast<const sf_bullet_rec *>(tb.p.get());
  if (subset & 16) k.io.d_portals = reinterpret_cast<const sf_portal_rec *>(tp.p.get());
  if (subset & 32) k.io.d_cell_flags = r.fl.data(), k.io.d_cell_dmg = r.dmg.data(), k.io.d_cell_portal = r.pidx.data();
  k.io.d_status = d.status.get(), k.io.d_selected = d.selected.get();
  put_call(k, parts);
  if (!verify) return;
  REQUIRE(d.counters.p[PUT_N_WRITTEN] == (unsigned long long)r.A && d.counters.p[PUT_N_REFUSED] == 0 && d.counters.p[PUT_N_RANGE] == 0);
  for (size_t a = 0; a < A; ++a) {
    REQUIRE(d.status.p[a] == 0);
    for (int g = 0; g < c.n_agents; ++g) REQUIRE(d.selected.p[a * c.n_agents + g] == 1);
    const int32_t *sc = d.scal.p.get() + a * SC_WORDS;
    if (subset & 1) {
      for (int j = 0; j < REC_HDR_WORDS; ++j)
        if (j != 18 && j != 19) REQUIRE(hdr_word(j, sc, d.rng.p.get() + a * RNG_WORDS) == r.hdr[a * 40 + j]);
      REQUIRE(sc[SC_EPISODES] == (int32_t)PW && sc[SC_WARM] == 0 && sc[SC_DRAWS] == (int32_t)((uint32_t)r.hdr[a * 40 + 10] - 1042u));
    } else {
      for (int j = 0; j < SC_WORDS; ++j)
        if (j != SC_ENDED && j != SC_PD01 && j != SC_PD23 && j != SC_PD45 && j != SC_LOAD && j != SC_ZWN && j != SC_PWN) REQUIRE(sc[j] == (int32_t)PW);
      for (int j = 0; j < RNG_WORDS; ++j) REQUIRE(d.rng.p[a * RNG_WORDS + j] == PW && d.rng2.p[a * RNG_WORDS + j] == PW);
    }
    REQUIRE(sc[SC_ENDED] == 0 && sc[SC_PD01] == 0 && sc[SC_PD23] == 0 && sc[SC_PD45] == 0);
    int halive = 0, zalive = 0, zext = 0, pext = 0;
    for (int i = 0; i < c.H; ++i) {
      uint32_t w[HW_WORDS];
      for (int f = 0; f < HW_WORDS; ++f) w[f] = d.hum.p[((size_t)f * A + a) * c.H + i];
      if (!(subset & 2)) {
        for (int f = 0; f < HW_WORDS; ++f) REQUIRE(w[f] == PW);
        continue;
      }
      sf_human_rec o, e{};
      decode_human(w, o);
      if (i < ch) std::memcpy(&e, r.hum.data() + (a * c.H + i) * 28, sizeof e);
      REQUIRE(std::memcmp(&o, &e, sizeof o) == 0);
      halive += e.alive;
      if (e.way == 0) REQUIRE(w[HW_POS] == POS_NONE && w[HW_FLAGS] == 0u);
    }
    for (int i = 0; i < c.Z; ++i) {
      uint32_t w[ZW_WORDS];
      for (int f = 0; f < ZW_WORDS; ++f) w[f] = d.zom.p[((size_t)f * A + a) * c.Z + i];
      if (!(subset & 4)) {
        for (int f = 0; f < ZW_WORDS; ++f) REQUIRE(w[f] == PW);
        continue;
      }
      sf_zombie_rec o, e{};
      decode_zombie(w[0], w[1], w[2], o);
      if (i < cz) std::memcpy(&e, r.zom.data() + (a * c.Z + i) * 7, sizeof e);
      REQUIRE(std::memcmp(&o, &e, sizeof o) == 0);
      if (e.alive) ++zalive, zext = i + 1;
      else REQUIRE(w[0] == 0u && w[1] == 0u && w[2] == 0u);
    }
    for (int i = 0; i < c.B; ++i) {
      uint32_t w[BW_WORDS];
      for (int f = 0; f < BW_WORDS; ++f) w[f] = d.bul.p[((size_t)f * A + a) * c.B + i];
      if (!(subset & 8)) {
        for (int f = 0; f < BW_WORDS; ++f) REQUIRE(w[f] == PW);
        continue;
      }
      sf_bullet_rec o, e{};
      decode_bullet(w[0], w[1], w[2], w[3], o);
      if (i < cb) std::memcpy(&e, r.bul.data() + (a * c.B + i) * 11, sizeof e);
      REQUIRE(std::memcmp(&o, &e, sizeof o) == 0);
      if (!e.alive) REQUIRE(w[0] == 0u && w[1] == 0u && w[2] == 0u && w[3] == 0u);
    }
    for (int i = 0; i < c.P; ++i) {
      const uint32_t w = d.por.p[a * c.P + i];
      if (!(subset & 16)) {
        REQUIRE(w == PW);
        continue;
      }
      sf_portal_rec o, e{};
      decode_portal(w, o);
      if (i < cp) std::memcpy(&e, r.por.data() + (a * c.P + i) * 4, sizeof e);
      REQUIRE(std::memcmp(&o, &e, sizeof o) == 0);
      if (e.active) pext = i + 1;
      else REQUIRE(w == 0u);
    }
    REQUIRE(sc[SC_LOAD] == (((subset & 6) == 6) ? halive + zalive : (int32_t)PW));
    REQUIRE(sc[SC_ZWN] == ((subset & 4) ? zw_for(zext) : (int32_t)PW) && sc[SC_PWN] == ((subset & 16) ? zw_for(pext) : (int32_t)PW));
    for (int ci = 0; ci < r.cells_pad; ++ci) {
      const uint8_t f = d.flags.p[a * r.cells_pad + ci];
      if (!(subset & 32) || ci >= c.cells) {
        REQUIRE(f == PATTERN);
        if (ci < c.cells) REQUIRE(d.aux_dmg.p[a * C + ci] == (int32_t)PW && d.aux_pidx.p[a * C + ci] == (int16_t)0x5B5B);
        continue;
      }
      REQUIRE(f == r.fl[a * C + ci]);
      REQUIRE(cell_dmg_of(f, d.aux_dmg.p[a * C + ci]) == r.dmg[a * C + ci]);
      REQUIRE(cell_portal_of(f, d.aux_pidx.p[a * C + ci], r.map_pidx[ci]) == r.pidx[a * C + ci]);
      if (!encode_cell_has_dmg(f)) REQUIRE(d.aux_dmg.p[a * C + ci] == (int32_t)PW);
      if (!encode_cell_has_pidx(f)) REQUIRE(d.aux_pidx.p[a * C + ci] == (int16_t)0x5B5B);
    }
  }
}

// every predicate at its last good and first bad value
static void predicates() {
  const PutCfg c = {3, 20, 30, 22, 200, 128, 109, 1800, SF_MODE_SQUAD, 3, 0, 1, 0, 3};
  sf_human_rec h{};
  REQUIRE(check_human(c, h));
  h.hp = 1;
  REQUIRE(!check_human(c, h));  // way 0 only on an all-zero slot
  h = sf_human_rec{};
  h.alive = 1, h.way = 4, h.f = 2, h.r = 19, h.c = 29, h.team = 255, h.vec = 2, h.ind = 7, h.blocks = 255, h.portals = 255, h.portal_ind = 108;
  h.hp = -5, h.effect = -7;
  for (int j = 0; j < 4; ++j) h.cons[j] = h.throw_cnt[j] = 65535;
  REQUIRE(check_human(c, h));
  auto bad = [&](auto edit) {
    sf_human_rec x = h;
    edit(x);
    return !check_human(c, x);
  };
  REQUIRE(bad([](sf_human_rec &x) { x.way = 5; }) && bad([](sf_human_rec &x) { x.f = 3; }) && bad([](sf_human_rec &x) { x.r = 20; }));
  REQUIRE(bad([](sf_human_rec &x) { x.c = 30; }) && bad([](sf_human_rec &x) { x.c = -1; }) && bad([](sf_human_rec &x) { x.team = 256; }));
  REQUIRE(bad([](sf_human_rec &x) { x.team = -1; }) && bad([](sf_human_rec &x) { x.vec = 3; }) && bad([](sf_human_rec &x) { x.vec = -2; }));
  REQUIRE(bad([](sf_human_rec &x) { x.ind = 8; }) && bad([](sf_human_rec &x) { x.ind = -1; }) && bad([](sf_human_rec &x) { x.alive = 2; }));
  REQUIRE(bad([](sf_human_rec &x) { x.vec = 0, x.ind = 4; }) && !bad([](sf_human_rec &x) { x.vec = 1, x.ind = 3; }));
  REQUIRE(!bad([](sf_human_rec &x) { x.vec = -1, x.ind = 14; }) && bad([](sf_human_rec &x) { x.vec = -1, x.ind = 15; }));
  REQUIRE(!bad([](sf_human_rec &x) { x.vec = -1, x.ind = -1; }) && bad([](sf_human_rec &x) { x.ind = -2; }));
  REQUIRE(bad([](sf_human_rec &x) { x.cons[3] = 65536; }) && bad([](sf_human_rec &x) { x.throw_cnt[0] = -1; }));
  REQUIRE(bad([](sf_human_rec &x) { x.blocks = 256; }) && bad([](sf_human_rec &x) { x.portals = -1; }));
  REQUIRE(bad([](sf_human_rec &x) { x.portal_ind = 109; }) && bad([](sf_human_rec &x) { x.portal_ind = -2; }) && !bad([](sf_human_rec &x) { x.portal_ind = -1; }));
  REQUIRE(bad([](sf_human_rec &x) { x.remote = 2; }) && bad([](sf_human_rec &x) { x.rnpc = -1; }) && bad([](sf_human_rec &x) { x.profile = 2; }));
  PutCfg big = c;
  big.P = 9000;
  h.portal_ind = 254;
  REQUIRE(check_human(big, h));
  h.portal_ind = 255;
  REQUIRE(!check_human(big, h));  // (the field has eight bits)
  sf_zombie_rec z = {1, 2, 19, 29, -1, -9, 1};
  REQUIRE(check_zombie(c, z));
  z.super_ = 2;
  REQUIRE(!check_zombie(c, z));
  z.super_ = 0, z.f = 3;
  REQUIRE(!check_zombie(c, z));
  z.alive = 0;
  REQUIRE(check_zombie(c, z));  // a dead slot's leftovers are not read
  z.alive = 2;
  REQUIRE(!check_zombie(c, z));
  sf_bullet_rec b = {1, 2, 19, 29, 4, 65535, -3, -32768, 65535, 22, 1};
  REQUIRE(check_bullet(c, b));
  auto badb = [&](auto edit) {
    sf_bullet_rec x = b;
    edit(x);
    return !check_bullet(c, x);
  };
  REQUIRE(badb([](sf_bullet_rec &x) { x.way = 0; }) && badb([](sf_bullet_rec &x) { x.way = 5; }) && badb([](sf_bullet_rec &x) { x.traveled = 65536; }));
  REQUIRE(badb([](sf_bullet_rec &x) { x.range = -1; }) && badb([](sf_bullet_rec &x) { x.effect = -32769; }) && badb([](sf_bullet_rec &x) { x.effect = 32768; }));
  REQUIRE(!badb([](sf_bullet_rec &x) { x.effect = 32767; }) && badb([](sf_bullet_rec &x) { x.owner = 23; }) && badb([](sf_bullet_rec &x) { x.owner = -1; }));
  REQUIRE(badb([](sf_bullet_rec &x) { x.ref = 2; }) && badb([](sf_bullet_rec &x) { x.r = 20; }) && !badb([](sf_bullet_rec &x) { x.owner = 0; }));
  sf_portal_rec p = {1, 2, 19, 29};
  REQUIRE(check_portal(c, p));
  p.c = 30;
  REQUIRE(!check_portal(c, p));
  p.active = 0;
  REQUIRE(check_portal(c, p));
  p.active = -1;
  REQUIRE(!check_portal(c, p));
  REQUIRE(check_cell(c, 0, 0, -1, -1) && !check_cell(c, 0, 1, -1, -1) && !check_cell(c, 0, 0, 0, -1));
  REQUIRE(check_cell(c, SF_CELL_CHEST | 0xC0, 0, -1, -1) && !check_cell(c, 0x40, 0, -1, -1) && !check_cell(c, 0x80 | SF_CELL_WALL, 0, -1, -1));
  REQUIRE(check_cell(c, SF_CELL_TEMP | SF_CELL_WALL, -77, -1, -1));
  REQUIRE(check_cell(c, SF_CELL_TEMP | SF_CELL_PIN_UP, 0, 108, -1) && !check_cell(c, SF_CELL_TEMP | SF_CELL_PIN_UP, 0, 109, -1));
  REQUIRE(check_cell(c, SF_CELL_TEMP | SF_CELL_PIN_UP, 0, 0, -1) && !check_cell(c, SF_CELL_TEMP | SF_CELL_PIN_UP, 0, -1, -1));
  REQUIRE(check_cell(c, SF_CELL_PIN_DN, 0, 5, 5) && !check_cell(c, SF_CELL_PIN_DN, 0, 4, 5) && !check_cell(c, SF_CELL_PIN_DN, 0, -1, 5));
  int32_t hw[40] = {0};
  hw[10] = 1042, hw[20] = 65536, hw[38] = 1, hw[39] = 6, hw[0] = 0x7fffffff, hw[16] = 0x7fffffff, hw[2] = -1, hw[3] = -1;
  hw[18] = -5, hw[19] = 12345;  // (episodes: ignored)
  REQUIRE(check_hdr(hw));
  auto badh = [&](int j, int32_t v) {
    int32_t x[40];
    std::memcpy(x, hw, sizeof x);
    x[j] = v;
    return !check_hdr(x);
  };
  REQUIRE(badh(10, 1041) && badh(11, 1) && badh(20, 65537) && badh(37, -1) && badh(38, 2) && badh(38, -1) && badh(39, 7) && badh(39, -1));
  REQUIRE(badh(0, -1) && badh(1, 1) && badh(16, -1) && badh(17, 1) && badh(3, 0) && badh(5, 1) && !badh(10, -1) && !badh(12, -1));
}

int main(int argc, char **argv) {
  REQUIRE(argc == 3);
  predicates();
  const Rows r = read_rows(argv[1]);
  int runs = 0;
  Dest d;
  static const int parts[3] = {1, 3, 64};
  for (int subset = 1; subset < 64; ++subset)
    for (int cutsel = 0; cutsel < 4; ++cutsel) {
      // above 512 cells: each part alone, and all of them
      if (r.c.cells > 512 && subset != 63 && (subset & (subset - 1))) continue;
      for (int pi = 0; pi < 3; ++pi) run(r, subset, cutsel, parts[pi], d), ++runs;
    }
  run(r, 63, 3, 1, d), ++runs;
  FILE *f = std::fopen(argv[2], "wb");
  REQUIRE(f);
  auto wr = [&](auto &h) { REQUIRE(h.n == 0 || std::fwrite(h.p.get(), sizeof h.p[0], h.n, f) == h.n); };
  wr(d.hum), wr(d.zom), wr(d.bul), wr(d.por), wr(d.rng), wr(d.rng2), wr(d.scal), wr(d.flags), wr(d.aux_dmg), wr(d.aux_pidx);
  std::fclose(f);
  std::printf("put_main ok %d\n", runs);
  return 0;
}
