// state_main.cpp — the lane functions of strikeforce_amd/csrc/sf_state_records.hpp (the text k_state_records compiles) in a
// stand-alone program: tests/test_state_records_cpu.py builds it plain and with -fsanitize=address,undefined and runs both.
//
//   state_main <state file> <output file>
//
// The state file holds the packed state of A arenas (layout below).  The program runs what sf_state_device runs — the init
// body, then for every (row, wavefront) the phases of every work unit, lanes 0..63 in a loop per phase — over heap buffers
// of exactly the sizes sf_state_bytes documents, so that the sanitizer sees every access out of bounds.  What the device does
// with wave intrinsics (the ballot behind the counts, the reduction of the lanes' digest sums, the atomic adds) is done here
// in plain loops; everything else is the header's text.  LDS is a heap buffer refilled with garbage before every unit.
//   - The full request (all outputs, all arenas, whole tables) is written to the output file, the ten outputs back to back:
//     the test compares it with the records the state was packed from and with the digest.  It is run with 1, 3 and 64
//     wavefronts per row besides the host's own choice: the outputs must be the same bytes.
//   - Every subset of the ten outputs x the cuts 0 / 1 / cap - 1 / cap x the id lists {none, one with a duplicate, one with
//     -1 and `arenas`} is compared with the slice of the full request it must equal (small states: at most 512 cells and
//     256 slots per pool; larger ones take every output alone, all, and none).
// Prints "state_main ok <requests run>" or the first mismatch.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../strikeforce_amd/csrc/sf_state_records.hpp"

using namespace sf;

struct State {
  int32_t A, H, Z, B, P, cells, cells_pad;
  std::vector<uint32_t> hum, zom, bul, por, rng;
  std::vector<int32_t> scal, aux_dmg;
  std::vector<uint8_t> flags;
  std::vector<int16_t> aux_pidx, map_pidx;
};

template <class T>
static void take(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) {
    fprintf(stderr, "state file too short\n");
    exit(2);
  }
}

// the ten outputs of one request, each a heap buffer of exactly its documented size (a zero-size one still has an address)
struct Outputs {
  std::vector<uint8_t *> buf = std::vector<uint8_t *>(10, nullptr);
  std::vector<size_t> bytes = std::vector<size_t>(10, 0);
  ~Outputs() {
    for (uint8_t *p : buf) free(p);
  }
};
static void sizes_of(const State &s, int rows, const int cut[4], size_t out[10]) {
  const size_t R = (size_t)rows, C = (size_t)s.cells;
  const size_t b[10] = {R * sizeof(sf_arena_hdr), R * cut[0] * sizeof(sf_human_rec), R * cut[1] * sizeof(sf_zombie_rec),
                        R * cut[2] * sizeof(sf_bullet_rec), R * cut[3] * sizeof(sf_portal_rec), R * C, R * C * 4, R * C * 4,
                        R * SF_STATE_COUNT_WORDS * 4, R * 8};
  memcpy(out, b, sizeof b);
}

static void fill(const State &s, StateRec &k, const int32_t *ids, int rows, const int cut[4], unsigned mask, Outputs &o) {
  memset(&k, 0, sizeof k);
  k.hum = s.hum.data(), k.zom = s.zom.data(), k.bul = s.bul.data(), k.por = s.por.data(), k.rng = s.rng.data();
  k.scal = s.scal.data(), k.flags = s.flags.data(), k.aux_dmg = s.aux_dmg.data(), k.aux_pidx = s.aux_pidx.data();
  k.map_pidx = s.map_pidx.data();
  k.A = s.A, k.H = s.H, k.Z = s.Z, k.B = s.B, k.P = s.P, k.cells = s.cells, k.cells_pad = s.cells_pad;
  k.io.d_arena_ids = ids, k.io.rows = ids ? rows : s.A;
  k.io.humans = cut[0], k.io.zombies = cut[1], k.io.bullets = cut[2], k.io.portals = cut[3];
  size_t b[10];
  sizes_of(s, k.io.rows, cut, b);
  for (int j = 0; j < 10; ++j) {
    if (!(mask >> j & 1u)) continue;
    o.bytes[j] = b[j];
    o.buf[j] = (uint8_t *)malloc(b[j] ? b[j] : 1);  // (exactly the size: the sanitizer's red zone starts behind it)
    memset(o.buf[j], 0xA5, b[j] ? b[j] : 1);
  }
  k.io.d_hdr = (sf_arena_hdr *)o.buf[0], k.io.d_humans = (sf_human_rec *)o.buf[1], k.io.d_zombies = (sf_zombie_rec *)o.buf[2];
  k.io.d_bullets = (sf_bullet_rec *)o.buf[3], k.io.d_portals = (sf_portal_rec *)o.buf[4], k.io.d_cell_flags = o.buf[5];
  k.io.d_cell_dmg = (int32_t *)o.buf[6], k.io.d_cell_portal = (int32_t *)o.buf[7], k.io.d_counts = (int32_t *)o.buf[8];
  k.io.d_digest = (uint64_t *)o.buf[9];
  k.parts = state_parts_for(state_units(k).total(), k.io.rows);
}

// ---- what the wavefront does around the lane functions (sf_state_records.hpp state_records_body) ----
struct Wave {
  std::vector<int32_t> lds = std::vector<int32_t>(ST_LDS_WORDS);
  uint64_t sum[64];
  void garbage() {
    for (int32_t &w : lds) w = 0x7f7f7f7f;
  }
};
static void count(const StateRec &k, const StateRow &r, int word, const bool alive[64], int slot0) {
  int n = 0, top = -1;
  for (int lane = 0; lane < 64; ++lane)
    if (alive[lane]) ++n, top = lane;
  if (k.io.d_counts && r.ok && n) {
    int32_t *c = k.io.d_counts + (size_t)r.row * SF_STATE_COUNT_WORDS;
    c[word] += n;
    if (c[4 + word] < slot0 + top + 1) c[4 + word] = slot0 + top + 1;
  }
}
template <class T>
static void table(const StateRec &k, const StateRow &r, int part, int base, int n, Wave &w) {
  for (int v = state_first_unit(part, base, k.parts); v < n; v += k.parts) {
    bool alive[64];
    w.garbage();
    for (int lane = 0; lane < 64; ++lane) alive[lane] = st_lane_decode<T>(k, r, v, lane, w.lds.data(), w.sum[lane]);
    count(k, r, T::COUNT, alive, v * 64);
    for (int lane = 0; lane < 64; ++lane) st_lane_store<T>(k, r, v, lane, w.lds.data());
  }
}
static void run(const StateRec &k) {
  const sf_state_io &io = k.io;
  if (!(io.d_hdr || io.d_humans || io.d_zombies || io.d_bullets || io.d_portals || io.d_cell_flags || io.d_cell_dmg ||
        io.d_cell_portal || io.d_counts || io.d_digest))
    return;
  if (io.d_counts || io.d_digest)
    for (int i = 0; i < io.rows; ++i) state_init_body(io, i);
  const StateUnits nu = state_units(k);
  Wave w;
  for (int row = 0; row < io.rows; ++row)
    for (int part = 0; part < k.parts; ++part) {
      const StateRow r = state_row(k, row);
      memset(w.sum, 0, sizeof w.sum);
      if (part == 0) {
        w.garbage();
        for (int lane = 0; lane < 64; ++lane) st_hdr_words(k, r, lane, w.lds.data());
        for (int lane = 0; lane < 64; ++lane) st_hdr_out(k, r, lane, w.lds.data(), w.sum[lane]);
      }
      int base = 1;
      table<StHumans>(k, r, part, base, nu.h, w);
      base += nu.h;
      table<StZombies>(k, r, part, base, nu.z, w);
      base += nu.z;
      table<StBullets>(k, r, part, base, nu.b, w);
      base += nu.b;
      for (int v = state_first_unit(part, base, k.parts); v < nu.p; v += k.parts) {
        bool alive[64];
        for (int lane = 0; lane < 64; ++lane) alive[lane] = st_lane_portal(k, r, v, lane, w.sum[lane]);
        count(k, r, 3, alive, v * 64);
      }
      base += nu.p;
      for (int v = state_first_unit(part, base, k.parts); v < nu.c; v += k.parts)
        for (int lane = 0; lane < 64; ++lane) st_lane_cells(k, r, v, lane, w.sum[lane]);
      if (io.d_digest && r.ok) {
        uint64_t total = 0;
        for (int lane = 0; lane < 64; ++lane) total += w.sum[lane];
        io.d_digest[row] += total;
      }
    }
}

// what output j of a request must hold, from the full request's: row i is arena ids[i]'s row with the tables cut, or the
// all-zero row (counts -1) of an id out of range
static bool matches(const State &s, const Outputs &full, const Outputs &got, int j, const int32_t *ids, int rows, const int cut[4]) {
  const int cap[4] = {s.H, s.Z, s.B, s.P};
  const size_t rec[4] = {sizeof(sf_human_rec), sizeof(sf_zombie_rec), sizeof(sf_bullet_rec), sizeof(sf_portal_rec)};
  const size_t got_row = rows ? got.bytes[j] / rows : 0, full_row = full.bytes[j] / s.A;
  for (int i = 0; i < rows && got_row; ++i) {
    const int id = ids ? ids[i] : i;
    const uint8_t *g = got.buf[j] + i * got_row;
    const bool ok = id >= 0 && id < s.A;
    std::vector<uint8_t> want(got_row, j == 8 && !ok ? 0xFF : 0);
    if (ok) {
      const uint8_t *f = full.buf[j] + (size_t)id * full_row;
      if (j >= 1 && j <= 4) {
        if (full_row != cap[j - 1] * rec[j - 1] || got_row != cut[j - 1] * rec[j - 1]) return false;
        memcpy(want.data(), f, got_row);  // the first `cut` slots
      } else {
        if (full_row != got_row) return false;
        memcpy(want.data(), f, got_row);
      }
    }
    if (memcmp(g, want.data(), got_row)) {
      printf("mismatch: output %d row %d (arena %d)\n", j, i, id);
      return false;
    }
  }
  return true;
}

int main(int argc, char **argv) {
  if (argc != 3) return fprintf(stderr, "usage: state_main <state file> <output file>\n"), 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  State s;
  int32_t h[7];
  if (fread(h, 4, 7, f) != 7) return fprintf(stderr, "state file too short\n"), 2;
  s.A = h[0], s.H = h[1], s.Z = h[2], s.B = h[3], s.P = h[4], s.cells = h[5], s.cells_pad = h[6];
  const size_t A = (size_t)s.A;
  take(f, s.hum, HW_WORDS * A * s.H), take(f, s.zom, ZW_WORDS * A * s.Z), take(f, s.bul, BW_WORDS * A * s.B);
  take(f, s.por, A * s.P), take(f, s.rng, A * RNG_WORDS), take(f, s.scal, A * SC_WORDS), take(f, s.flags, A * s.cells_pad);
  take(f, s.aux_dmg, A * s.cells), take(f, s.aux_pidx, A * s.cells), take(f, s.map_pidx, (size_t)s.cells);
  fclose(f);

  const int cap[4] = {s.H, s.Z, s.B, s.P};
  int requests = 0;
  // ---- the full request, with the host's choice of wavefronts per row and with 1, 3 and 64
  Outputs full;
  StateRec k;
  fill(s, k, nullptr, 0, cap, 0x3FFu, full);
  run(k), ++requests;
  for (int parts : {1, 3, 64}) {
    Outputs o;
    StateRec q;
    fill(s, q, nullptr, 0, cap, 0x3FFu, o);
    q.parts = parts < state_units(q).total() ? parts : state_units(q).total();
    run(q), ++requests;
    for (int j = 0; j < 10; ++j)
      if (memcmp(o.buf[j], full.buf[j], full.bytes[j])) return printf("mismatch: output %d with %d wavefronts per row\n", j, parts), 1;
  }
  FILE *out = fopen(argv[2], "wb");
  if (!out) return fprintf(stderr, "cannot write %s\n", argv[2]), 2;
  for (int j = 0; j < 10; ++j)
    if (full.bytes[j] && fwrite(full.buf[j], 1, full.bytes[j], out) != full.bytes[j]) return 2;
  fclose(out);

  // ---- subsets x cuts x id lists against slices of the full request
  const bool small = s.cells <= 512 && s.H <= 256 && s.Z <= 256 && s.B <= 256 && s.P <= 256;
  std::vector<unsigned> masks;
  if (small)
    for (unsigned m = 0; m < 1024u; ++m) masks.push_back(m);
  else {
    masks = {0u, 0x3FFu};
    for (int j = 0; j < 10; ++j) masks.push_back(1u << j);
  }
  const std::vector<int32_t> dup = {s.A - 1, 0, 0}, wild = {s.A, 0, -1, s.A - 1, INT32_MAX, INT32_MIN};
  const std::vector<int32_t> *lists[3] = {nullptr, &dup, &wild};
  for (int level = 0; level < 4; ++level) {
    int cut[4];
    for (int t = 0; t < 4; ++t) cut[t] = level == 0 ? 0 : level == 1 ? 1 : level == 2 ? cap[t] - 1 : cap[t];
    for (const std::vector<int32_t> *ids : lists)
      for (unsigned m : masks) {
        // heap copies of exactly their size: the id list too
        const int rows = ids ? (int)ids->size() : s.A;
        int32_t *d_ids = nullptr;
        if (ids) {
          d_ids = (int32_t *)malloc(ids->size() * 4);
          memcpy(d_ids, ids->data(), ids->size() * 4);
        }
        Outputs o;
        StateRec q;
        fill(s, q, d_ids, rows, cut, m, o);
        run(q), ++requests;
        bool good = true;
        for (int j = 0; j < 10 && good; ++j)
          if (m >> j & 1u) good = matches(s, full, o, j, d_ids, rows, cut);
        free(d_ids);
        if (!good) return printf("  in request: outputs %03x, cut level %d, id list %d\n", m, level, ids == lists[1] ? 1 : ids ? 2 : 0), 1;
      }
  }
  printf("state_main ok %d\n", requests);
  return 0;
}
