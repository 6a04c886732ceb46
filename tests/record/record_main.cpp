// TEST INFRASTRUCTURE ONLY: the lane functions of strikeforce_amd/csrc/sf_record.hpp — the text k_record, k_record_plan and
// k_record_copy compile — run on the CPU with the lanes in loops, over heap buffers of exactly the documented sizes (a
// fresh allocation per launch for everything the launch only reads, and per collect for its outputs), so that a build with
// -fsanitize=address,undefined sees every access.  Driven by tests/test_record_cpu.py.
//
//   record_main <trace> <out>
// trace, int32 words: A H n_agents ind auto_reset G bpa, then events:
//   0 TOP    scal [A][SC_WORDS], cmd [A][n_agents] (one word per byte)                       k_record mode 0
//   1 MID    flags [A][H] (the HW_FLAGS plane), cmd [A][n_agents]                            k_record mode 1
//   2 END    scal [A][SC_WORDS], results [A][n_agents][8]                                    k_record mode 2
//   3 FLUSH                                                                                  k_record mode 3
//   4 COLLECT max_bytes max_games                                                            k_record_plan + k_record_copy
// out: per COLLECT int64 counts[6], then int32 games[counts[0]][12], then counts[1] bytes (padded to 8).
// Where the kernels exchange something between lanes, the loops here do it the way the wavefront does: the ballot of mode
// 1 is gathered over all lanes before any lane stores, and every pass of the copy loads on all 64 lanes before it stores.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../strikeforce_amd/csrc/sf_record.hpp"

using namespace sf;

static std::vector<int32_t> trace;
static size_t at = 0;
static int32_t next() {
  if (at >= trace.size()) fprintf(stderr, "record_main: trace ends early\n"), exit(2);
  return trace[at++];
}
template <class T>
static std::unique_ptr<T[]> take(size_t n) {  // exactly n elements on the heap
  std::unique_ptr<T[]> p(new T[n]);
  for (size_t i = 0; i < n; ++i) p[i] = (T)next();
  return p;
}

int main(int argc, char **argv) {
  if (argc != 3) return fprintf(stderr, "usage: record_main <trace> <out>\n"), 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  fseek(f, 0, SEEK_END);
  trace.resize((size_t)ftell(f) / 4);
  fseek(f, 0, SEEK_SET);
  if (fread(trace.data(), 4, trace.size(), f) != trace.size()) return fprintf(stderr, "short read\n"), 2;
  fclose(f);
  FILE *out = fopen(argv[2], "wb");
  if (!out) return perror(argv[2]), 2;

  Record k;
  memset(&k, 0, sizeof k);
  k.A = next(), k.H = next(), k.n_agents = next(), k.ind = next(), k.auto_reset = next(), k.G = next(), k.bpa = next();
  const size_t A = (size_t)k.A, na = (size_t)k.n_agents;
  std::unique_ptr<uint8_t[]> bytes(new uint8_t[A * (size_t)k.bpa]);
  std::unique_ptr<int32_t[]> games(new int32_t[A * (size_t)k.G * RG_WORDS]), st(new int32_t[A * RC_WORDS]()), plan(new int32_t[A * RPL_WORDS]);
  memset(bytes.get(), 0xEE, A * (size_t)k.bpa);
  k.bytes = bytes.get(), k.games = games.get(), k.st = st.get(), k.plan = plan.get();
  long events = 0, collects = 0;
  while (at < trace.size()) {
    const int32_t ev = next();
    ++events;
    if (ev == 0) {
      auto scal = take<int32_t>(A * SC_WORDS);
      auto cmd = take<uint8_t>(A * na);
      k.scal = scal.get(), k.cmd = cmd.get();
      for (int a = 0; a < k.A; ++a) record_top(k, a);
    } else if (ev == 1) {
      // the whole [HW_WORDS][A][H] buffer, as the kernel's index computes into it; only the flag plane is defined
      std::unique_ptr<uint32_t[]> hum(new uint32_t[(size_t)HW_WORDS * A * (size_t)k.H]);
      memset(hum.get(), 0xFF, (size_t)HW_WORDS * A * (size_t)k.H * 4);
      for (size_t i = 0; i < A * (size_t)k.H; ++i) hum[(size_t)HW_FLAGS * A * (size_t)k.H + i] = (uint32_t)next();
      auto cmd = take<uint8_t>(A * na);
      k.hum = hum.get(), k.cmd = cmd.get();
      for (int a = 0; a < k.A; ++a) {
        uint64_t bal = 0;
        for (int g = 0; g < 64; ++g)
          if (record_mid_takes(k, a, g)) bal |= 1ull << g;
        if (!bal) continue;
        int subs = 0;
        for (int g = 0; g < 64; ++g)
          if ((bal >> g) & 1ull) subs += record_mid_store(k, a, g, bal) ? 1 : 0;
        record_mid_finish(k, a, __builtin_popcountll(bal), subs);
      }
      k.hum = nullptr;
    } else if (ev == 2) {
      auto scal = take<int32_t>(A * SC_WORDS);
      auto res = take<int32_t>(A * na * 8);
      k.scal = scal.get(), k.results = res.get();
      for (int a = 0; a < k.A; ++a) record_end(k, a);
      k.results = nullptr;
    } else if (ev == 3) {
      for (int a = 0; a < k.A; ++a) record_flush(k, a);
    } else if (ev == 4) {
      const int64_t max_bytes = next(), max_games = next();
      std::unique_ptr<uint8_t[]> d_bytes(new uint8_t[(size_t)max_bytes]);
      std::unique_ptr<int32_t[]> d_games(new int32_t[(size_t)max_games * RG_WORDS]);
      int64_t gpre = 0, bpre = 0, tg = 0, tb = 0, lost = 0, subst = 0;
      for (int a = 0; a < k.A; ++a) {
        int64_t ga, ba;
        record_arena_totals(k, a, ga, ba);
        record_plan_arena(k, a, gpre, bpre, max_games, max_bytes, tg, tb, lost, subst);
        gpre += ga, bpre += ba;
      }
      const int64_t counts[6] = {tg, tb, gpre - tg, bpre - tb, lost, subst};
      for (int a = 0; a < k.A; ++a) {
        const RecordCopy c = record_copy_load(k, a);
        if (c.ntake == 0) continue;
        for (int32_t i = 0; i < c.ntake * RG_WORDS; ++i) record_copy_game_word(k, c, a, i, d_games.get());
        for (int32_t i = 0; i < c.tbytes; ++i) record_copy_byte(k, c, a, i, d_bytes.get());
        const int32_t rem_w = (c.ngames - c.ntake) * RG_WORDS, rem_b = c.used - c.tbytes;
        for (int32_t i0 = 0; i0 < rem_w; i0 += 64) {
          int32_t v[64];
          for (int l = 0; l < 64 && i0 + l < rem_w; ++l) v[l] = record_compact_word_load(k, c, a, i0 + l);
          for (int l = 0; l < 64 && i0 + l < rem_w; ++l) record_compact_word_store(k, a, i0 + l, v[l]);
        }
        if (c.tbytes)
          for (int32_t i0 = 0; i0 < rem_b; i0 += 64) {
            uint8_t v[64];
            for (int l = 0; l < 64 && i0 + l < rem_b; ++l) v[l] = record_compact_byte_load(k, c, a, i0 + l);
            for (int l = 0; l < 64 && i0 + l < rem_b; ++l) record_compact_byte_store(k, a, i0 + l, v[l]);
          }
        record_copy_finish(k, c, a);
      }
      fwrite(counts, 8, 6, out);
      if (tg) fwrite(d_games.get(), 4, (size_t)tg * RG_WORDS, out);
      std::vector<uint8_t> pad((size_t)((tb + 7) / 8 * 8), 0);
      if (tb) memcpy(pad.data(), d_bytes.get(), (size_t)tb), fwrite(pad.data(), 1, pad.size(), out);
      ++collects;
    } else {
      return fprintf(stderr, "record_main: unknown event %d\n", ev), 2;
    }
    k.scal = nullptr, k.cmd = nullptr;
  }
  fclose(out);
  printf("record_main ok %ld %ld\n", events, collects);
  return 0;
}
