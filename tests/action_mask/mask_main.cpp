// mask_main.cpp — the body of strikeforce_amd/csrc/sf_action_mask.hpp (the text k_action_mask compiles) against the truth, in a
// stand-alone program: tests/test_action_mask_cpu.py builds it plain and with -fsanitize=address,undefined and runs both.
//
//   mask_main <state file> <output file>
//
// The state file holds the configuration and the packed state of A arenas (layout in main()).  The tables are built with
// sf_host.hpp's own derive_profile / finish_derived / fill_hatab, as Env::create builds them.
//   (a) The mask: ActionMaskCore<WaveEmu>::body for every arena over heap buffers of exactly the documented sizes, so that the
//       sanitizer sees every access out of bounds — the command words alone, the action words alone for three action strings,
//       and both together, which must agree.
//   (b) The truth: for every arena, every present commanded human and every command of SF_COMMANDS, the product's own
//       Core<WaveEmu, ..>::load -> obey -> store (the instance Env::create would pick) on a copy of the state; the bit is set
//       when any of the arena's rows in any buffer of the copy differs, byte by byte, from what load -> store without a
//       command leaves.  (That run is obey('+'); whether it reproduced the state file's bytes exactly is printed, not required: a packed dump carries words
//       no record shows, and store() rewrites them.)
// (a) must equal (b) for all 30 commands, the '+' rule aside: bit 0 is set for every present agent, and an agent that is not
// present has the word 0.  Both are written to the output file, [A][n_agents] uint32 each, the mask first.
// Prints "mask_main ok <agents present> <bits compared>" or every mismatch.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../emu/wave_emu.hpp"
#include "../../strikeforce_amd/csrc/sf_core.hpp"
#include "../../strikeforce_amd/csrc/sf_host.hpp"
#include "../../strikeforce_amd/csrc/sf_action_mask.hpp"

using namespace sf;

struct State {
  std::vector<uint32_t> hum, zom, bul, por, rng, rng2;
  std::vector<int32_t> scal, aux_dmg;
  std::vector<uint8_t> flags;
  std::vector<int16_t> aux_pidx;
  bool operator==(const State &o) const {
    return hum == o.hum && zom == o.zom && bul == o.bul && por == o.por && rng == o.rng && rng2 == o.rng2 && scal == o.scal &&
           aux_dmg == o.aux_dmg && flags == o.flags && aux_pidx == o.aux_pidx;
  }
  void into(Params &p) {
    p.hum = hum.data(), p.zom = zom.data(), p.bul = bul.data(), p.por = por.data(), p.rng = rng.data(), p.rng2 = rng2.data();
    p.scal = scal.data(), p.aux_dmg = aux_dmg.data(), p.flags = flags.data(), p.aux_pidx = aux_pidx.data();
  }
};

template <class T>
static void take(FILE *f, T *v, size_t n) {
  if (n && fread(v, sizeof(T), n, f) != n) {
    fprintf(stderr, "state file too short\n");
    exit(2);
  }
}
template <class T>
static void take(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  take(f, v.data(), n);
}
// a heap copy of exactly the vector's bytes (the sanitizer's red zone starts right behind it)
template <class T>
static T *exact(const std::vector<T> &v) {
  const size_t bytes = v.size() * sizeof(T);
  T *p = (T *)malloc(bytes ? bytes : 1);
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

// whether arena a's rows of every buffer hold the same bytes in x and y
template <class T>
static bool same_rows(const std::vector<T> &x, const std::vector<T> &y, size_t fields, size_t A, size_t a, size_t row) {
  for (size_t f = 0; f < fields; ++f)
    if (row && memcmp(x.data() + (f * A + a) * row, y.data() + (f * A + a) * row, row * sizeof(T))) return false;
  return true;
}
static bool same_arena(const State &x, const State &y, const Params &p, int a) {
  const size_t A = (size_t)p.A;
  return same_rows(x.hum, y.hum, HW_WORDS, A, a, p.H) && same_rows(x.zom, y.zom, ZW_WORDS, A, a, p.Z) &&
         same_rows(x.bul, y.bul, BW_WORDS, A, a, p.B) && same_rows(x.por, y.por, 1, A, a, p.P) &&
         same_rows(x.rng, y.rng, 1, A, a, RNG_WORDS) && same_rows(x.rng2, y.rng2, 1, A, a, RNG_WORDS) &&
         same_rows(x.scal, y.scal, 1, A, a, SC_WORDS) && same_rows(x.aux_dmg, y.aux_dmg, 1, A, a, p.cells) &&
         same_rows(x.flags, y.flags, 1, A, a, p.cells_pad) && same_rows(x.aux_pidx, y.aux_pidx, 1, A, a, p.cells);
}

// load -> obey(c) -> store of arena a on the buffers `p` points at; c == 0: no command
static void play(const Params &p, int NB, int a, uint32_t c, uint32_t slot) {
  with_variant(p, NB, [&](auto v) {
    using K = Core<WaveEmu, decltype(v)::NB, decltype(v)::HP, decltype(v)::BM, decltype(v)::ZL>;
    std::vector<uint8_t> lds(lds_bytes_for(p.cells_pad, p.lds_tab, p.Z, p.P) + 64, 0x7f);
    typename K::Arena S;
    uint8_t *plane = K::tables(S, lds.data(), p, a);
    K::load(S, plane, p, a);
    if (c) K::obey(S, plane, p, a, c, slot);
    K::store(S, plane, p, a);
    return 0;
  });
}

int main(int argc, char **argv) {
  if (argc != 3) return fprintf(stderr, "usage: mask_main <state file> <output file>\n"), 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
  // header: A H Z B P F N M cells_pad n_agents mode ind level n_agent_profiles 0 0; player, npc, items, agent_profile[16]
  int32_t h[16];
  take(f, h, 16);
  sf_config cfg;
  memset(&cfg, 0, sizeof cfg);
  take(f, &cfg.player, 1), take(f, &cfg.npc, 1), take(f, &cfg.items, 1), take(f, cfg.agent_profile, SF_MAX_AGENTS);
  cfg.level = h[12], cfg.n_agent_profiles = h[13];
  Params p;
  memset(&p, 0, sizeof p);
  p.A = h[0], p.H = h[1], p.Z = h[2], p.B = h[3], p.P = h[4], p.F = h[5], p.N = h[6], p.M = h[7], p.cells_pad = h[8];
  p.n_agents = h[9], p.mode = h[10], p.ind = h[11], p.level = h[12];
  p.cells = p.F * p.N * p.M, p.bm_words = bm_words_for(p.cells_pad);
  const int NB = large_pools(p.Z, p.P) ? 4 : nb_for(p.B);
  // the tables, as Env::create builds them
  static Tables tab;
  memset(&tab, 0, sizeof tab);
  p.npc_block = cfg.n_agent_profiles > 0 ? MAX_PROFILE_BLOCKS - 1 : 1;
  p.ht_bytes = ht_bytes_for(p.npc_block + 1), p.lds_tab = lds_tab_for(p.npc_block + 1);
  for (int i = 0; i < p.npc_block; ++i)
    derive_profile(cfg, (cfg.n_agent_profiles > 0 && i < cfg.n_agent_profiles) ? cfg.agent_profile[i] : cfg.player, tab.der[i]);
  derive_profile(cfg, cfg.npc, tab.der[p.npc_block]);
  tab.der[p.npc_block].mindamage_def += 15 * (cfg.level - 1);
  for (int i = 0; i <= p.npc_block; ++i) finish_derived(tab.der[i]);
  for (int i = 0; i < 4; ++i)
    for (int k = 0; k < 3; ++k) tab.cons_items[i][k] = cfg.items.cons[i][k];
  fill_hatab(tab, p.npc_block + 1);
  p.tab = &tab;
  std::vector<uint16_t> logt(LOGT_ENTRIES, 0);
  std::vector<uint32_t> exptab(512);
  build_rng_tables(logt.data(), exptab.data());
  p.logt = logt.data(), p.exptab = exptab.data();

  State s;
  const size_t A = (size_t)p.A;
  take(f, s.hum, HW_WORDS * A * p.H), take(f, s.zom, ZW_WORDS * A * p.Z), take(f, s.bul, BW_WORDS * A * p.B);
  take(f, s.por, A * p.P), take(f, s.rng, A * RNG_WORDS), take(f, s.scal, A * SC_WORDS), take(f, s.flags, A * p.cells_pad);
  take(f, s.aux_dmg, A * p.cells), take(f, s.aux_pidx, A * p.cells);
  s.rng2.assign(A * RNG_WORDS, 0u);
  fclose(f);
  const size_t n = A * (size_t)p.n_agents;

  // ---- (a) the mask ----
  ActionMask k;
  memset(&k, 0, sizeof k);
  uint32_t *hum = exact(s.hum), *zom = exact(s.zom), *bul = exact(s.bul), *por = exact(s.por);
  int32_t *scal = exact(s.scal);
  uint8_t *flags = exact(s.flags);
  Tables *tabx = (Tables *)malloc(sizeof tab);
  memcpy(tabx, &tab, sizeof tab);
  k.hum = hum, k.zom = zom, k.bul = bul, k.por = por, k.scal = scal, k.flags = flags, k.tab = tabx;
  k.A = p.A, k.F = p.F, k.N = p.N, k.M = p.M, k.cells_pad = p.cells_pad, k.H = p.H, k.Z = p.Z, k.B = p.B, k.P = p.P;
  k.n_agents = p.n_agents, k.npc_block = p.npc_block;
  const char *strings[3] = {"+xzqeawsd", SF_COMMANDS, "__+xzqeawsd[]uu3fghjkl;'cvbnm,./"};  // the last: 32 chars, repeats
  std::vector<uint32_t> mask(n);
  int bad = 0;
  for (int round = 0; round < 7; ++round) {  // commands alone; per string: actions alone, both
    const char *str = round ? strings[(round - 1) / 2] : nullptr;
    const bool both = round && (round - 1) % 2;
    uint32_t *cm = (!round || both) ? (uint32_t *)malloc(n * 4) : nullptr, *ac = round ? (uint32_t *)malloc(n * 4) : nullptr;
    if (cm) memset(cm, 0xA5, n * 4);
    if (ac) memset(ac, 0xA5, n * 4);
    memset(k.action_bit, 31, sizeof k.action_bit);
    k.n_actions = str ? (int32_t)strlen(str) : 0;
    if (k.n_actions > 32) return fprintf(stderr, "action string too long\n"), 2;
    for (int j = 0; j < k.n_actions; ++j) k.action_bit[j] = (uint8_t)(strchr(SF_COMMANDS, str[j]) - SF_COMMANDS);
    k.commands = cm, k.actions = ac;
    for (int a = 0; a < p.A; ++a) ActionMaskCore<WaveEmu>::body(k, a);
    if (!round) memcpy(mask.data(), cm, n * 4);
    for (size_t i = 0; i < n; ++i) {
      if (cm && cm[i] != mask[i]) ++bad, printf("mismatch: commands differ between requests, round %d, agent %zu\n", round, i);
      if (ac) {
        uint32_t want = 0;
        for (int j = 0; j < k.n_actions; ++j) want |= ((mask[i] >> k.action_bit[j]) & 1u) << j;
        if (ac[i] != want) ++bad, printf("mismatch: actions of \"%s\", agent %zu: %08x, expected %08x\n", str, i, ac[i], want);
      }
    }
    free(cm), free(ac);
  }
  free(hum), free(zom), free(bul), free(por), free(scal), free(flags), free(tabx);

  // ---- (b) the truth ----
  State base = s;
  base.into(p);
  for (int a = 0; a < p.A; ++a) play(p, NB, a, 0u, 0u);
  printf("load -> store %s the state file's bytes\n", base == s ? "reproduces" : "does not reproduce");
  std::vector<uint32_t> truth(n, 0u);
  long present = 0, bits = 0;
  for (int a = 0; a < p.A; ++a)
    for (int g = 0; g < p.n_agents; ++g) {
      const uint32_t fl = s.hum[HW_FLAGS * A * p.H + (size_t)a * p.H + g];
      if ((fl & (HF_ALIVE | HF_CTRL)) != (HF_ALIVE | HF_CTRL)) continue;
      ++present;
      uint32_t w = 1u;
      for (int c = 1; c < SF_N_COMMANDS; ++c) {
        State work = s;
        work.into(p);
        play(p, NB, a, (uint32_t)(uint8_t)SF_COMMANDS[c], (uint32_t)g);
        if (!same_arena(work, base, p, a)) w |= 1u << c;
        ++bits;
      }
      truth[(size_t)a * p.n_agents + g] = w;
    }
  for (size_t i = 0; i < n; ++i)
    if (mask[i] != truth[i]) {
      ++bad;
      printf("mismatch: arena %zu agent %zu: mask %08x truth %08x:", i / p.n_agents, i % p.n_agents, mask[i], truth[i]);
      for (int c = 0; c < SF_N_COMMANDS; ++c)
        if ((mask[i] ^ truth[i]) >> c & 1u) printf(" '%c'", SF_COMMANDS[c]);
      printf("\n");
    }
  FILE *out = fopen(argv[2], "wb");
  if (!out) return fprintf(stderr, "cannot write %s\n", argv[2]), 2;
  if (fwrite(mask.data(), 4, n, out) != n || fwrite(truth.data(), 4, n, out) != n) return 2;
  fclose(out);
  if (bad) return printf("mask_main: %d mismatches\n", bad), 1;
  printf("mask_main ok %ld %ld\n", present, bits);
  return 0;
}
