// sf_record.hpp — the device side of sf_record_* (strikeforce.h): games played through sf_record_step written out as the
// command streams of `.sf_sample` files — the inverse of replay_fetch (sf_core.hpp).  Per iteration a stream holds the
// command of `ind`, then one byte for every other commanded human that is alive and still commanded when human_action
// runs (gameplay.hpp:966-967, 979-986), slots ascending.
//
// The bodies are plain SF_HD lane functions over pointers.  k_record / k_record_plan / k_record_copy (sf_api.hip) call
// them with one wavefront per arena; tests/record/record_main.cpp calls them with the lanes in loops; both compile this
// text.  Where lanes exchange something (the ballot of k_record's mode 1, the scan of k_record_plan, "every load of a
// pass before its stores" in k_record_copy) the exchange is the caller's and the functions here are its two sides.
//
// A recorder owns, per arena,
//   a region of `bpa` bytes: the streams of its closed games back to back from byte 0, then the open game's;
//   an index of `G` game records of SF_RECORD_GAME_WORDS words, the closed games in order (word 10 = the stream's first
//   byte in the region until a collect turns it into the offset in the caller's buffer);
//   RC_WORDS state words.
// Nothing of the environment is written.  No LDS, no scratch; lane 0 writes the cursor and the game words.
#pragma once
#include "../../include/strikeforce.h"
#include "sf_types.hpp"

namespace sf {

enum { RC_OPEN = 0,   // a game is being written
       RC_ACTIVE,     // ... and the line of `ind` of the running iteration was written at this loop top
       RC_ITERS,      // iterations of the open game
       RC_START,      // first byte of the open game in the region = end of the closed games
       RC_USED,       // first free byte of the region
       RC_NGAMES,     // closed games in the index
       RC_LOST,       // games not opened because the index was full, since the last collect
       RC_SUBST,      // bytes written as '+' because a sample cannot carry them, since the last collect
       RC_EPISODE, RC_TB_LO, RC_TB_HI, RC_SR_LO, RC_SR_HI,  // the open game's episode and seed
       RC_WORDS = 16 };
enum { RG_ARENA = 0, RG_EPISODE, RG_TB_LO, RG_TB_HI, RG_SR_LO, RG_SR_HI, RG_LINES, RG_ITERS, RG_END, RG_OUTCOME, RG_OFF_LO,
       RG_OFF_HI, RG_WORDS = SF_RECORD_GAME_WORDS };
enum { RPL_GBASE = 0, RPL_NTAKE, RPL_TBYTES, RPL_BB_LO, RPL_BB_HI, RPL_WORDS = 6 };  // k_record_plan's row of one arena

// What the record kernels take, by value in the kernel arguments.  A struct of its own, like Replay and Signals: Params
// stays as it is.
struct Record {
  const uint32_t *hum;     // Params::hum  [HW_WORDS][A][H]
  const int32_t *scal;     // Params::scal [A][SC_WORDS]
  const int32_t *results;  // Params::results [A][n_agents][8]
  const uint8_t *cmd;      // [A][n_agents]: the row k_step_half's second phase reads
  uint8_t *bytes;          // [A][bpa]
  int32_t *games;          // [A][G][RG_WORDS]
  int32_t *st;             // [A][RC_WORDS]
  int32_t *plan;           // [A][RPL_WORDS]
  int32_t A, H, n_agents, ind, auto_reset, G, bpa, pad;
};

#if defined(__HIP_DEVICE_COMPILE__)
#define SF_REC_G __attribute__((address_space(1)))
template <class T>
static __device__ __forceinline__ const SF_REC_G T *rec_g(const T *p) { return (const SF_REC_G T *)p; }
template <class T>
static __device__ __forceinline__ SF_REC_G T *rec_g(T *p) { return (SF_REC_G T *)p; }
#else
template <class T>
static inline T *rec_g(T *p) { return p; }
#endif

// `operator>>` reads one token per command: white space and control bytes cannot stand in a sample, and bytes of 0x7f and
// above are no reference command.  Every such byte acts exactly as '+' here: obey() (sf_core.hpp) tests for its command
// chars one by one and does nothing for any other, and the lane-parallel form looks the class up in a 128-entry table
// whose only non-zero entries are those chars (fill_hatab, sf_host.hpp), reading nothing for bytes >= 128.
SF_HD inline bool record_unwritable(uint32_t c) { return c <= 0x20u || c >= 0x7fu; }

// lane 0: the open game becomes the next closed one
SF_HD inline void record_close(const Record &k, int a, int32_t end, int32_t outcome) {
  auto *st = rec_g(k.st) + (size_t)a * RC_WORDS;
  const int32_t g = st[RC_NGAMES], start = st[RC_START], used = st[RC_USED];
  auto *r = rec_g(k.games) + ((size_t)a * (size_t)k.G + (size_t)g) * RG_WORDS;
  r[RG_ARENA] = a, r[RG_EPISODE] = st[RC_EPISODE];
  r[RG_TB_LO] = st[RC_TB_LO], r[RG_TB_HI] = st[RC_TB_HI], r[RG_SR_LO] = st[RC_SR_LO], r[RG_SR_HI] = st[RC_SR_HI];
  r[RG_LINES] = used - start, r[RG_ITERS] = st[RC_ITERS], r[RG_END] = end, r[RG_OUTCOME] = outcome;
  r[RG_OFF_LO] = start, r[RG_OFF_HI] = 0;
  st[RC_NGAMES] = g + 1, st[RC_OPEN] = 0, st[RC_ACTIVE] = 0, st[RC_START] = used;
}

// mode 0, lane 0, in front of the iteration's first half: the loop top as the recorder sees it (rules: strikeforce.h)
SF_HD inline void record_top(const Record &k, int a) {
  auto *st = rec_g(k.st) + (size_t)a * RC_WORDS;
  const auto *sc = rec_g(k.scal) + (size_t)a * SC_WORDS;
  const int32_t done = sc[SC_DONE], steps = sc[SC_STEPS], episodes = sc[SC_EPISODES];
  bool open = st[RC_OPEN] != 0;
  st[RC_ACTIVE] = 0;
  if (open) {
    if (!done && steps == 0) {  // the arena was restarted under the game: cut, or ended behind the recorder's back
      record_close(k, a, episodes > st[RC_EPISODE] ? SF_RECORD_BROKEN : SF_RECORD_CUT, SF_RUNNING);
      open = false;
    } else if (done || st[RC_ITERS] != steps) {  // stepped through another entry point, or loaded from a snapshot
      record_close(k, a, SF_RECORD_BROKEN, SF_RUNNING);
      open = false;
    }
  }
  if (done) return;
  if (!open) {
    if (steps != 0) return;  // (a game is recorded from its first iteration or not at all)
    if (st[RC_NGAMES] >= k.G) {
      st[RC_LOST] = st[RC_LOST] + 1;
      return;
    }
    st[RC_OPEN] = 1, st[RC_ITERS] = 0, st[RC_EPISODE] = episodes;
    st[RC_TB_LO] = sc[SC_TB_LO], st[RC_TB_HI] = sc[SC_TB_HI], st[RC_SR_LO] = sc[SC_SR_LO], st[RC_SR_HI] = sc[SC_SR_HI];
  }
  const int32_t used = st[RC_USED];
  if (k.bpa - used < k.n_agents) {  // no room for a whole iteration: nothing of it is written
    record_close(k, a, SF_RECORD_OVERFLOW, SF_RUNNING);
    return;
  }
  uint32_t c = rec_g(k.cmd)[(size_t)a * (size_t)k.n_agents + (size_t)k.ind];
  if (record_unwritable(c)) c = (uint32_t)'+', st[RC_SUBST] = st[RC_SUBST] + 1;
  rec_g(k.bytes)[(size_t)a * (size_t)k.bpa + (size_t)used] = (uint8_t)c;
  st[RC_USED] = used + 1, st[RC_ITERS] = st[RC_ITERS] + 1, st[RC_ACTIVE] = 1;
}

// mode 1, between the halves.  record_mid_takes: replay_fetch mode 1's predicate for lane g, 0 for an arena that wrote no
// line of `ind` at this loop top.  record_mid_store: lane g's byte at its rank in the ballot of those lanes; true if the
// byte was substituted.  record_mid_finish: lane 0, behind every lane's store.
SF_HD inline bool record_mid_takes(const Record &k, int a, int g) {
  if (!rec_g(k.st)[(size_t)a * RC_WORDS + RC_ACTIVE] || g >= k.n_agents || g == k.ind) return false;
  const uint32_t fl = rec_g(k.hum)[((size_t)HW_FLAGS * (size_t)k.A + (size_t)a) * (size_t)k.H + (size_t)g];
  return (fl & (HF_ALIVE | HF_CTRL)) == (HF_ALIVE | HF_CTRL);
}
SF_HD inline int record_rank(uint64_t ballot, int g) {
  const uint64_t below = ballot & ((1ull << g) - 1ull);
#if defined(__HIP_DEVICE_COMPILE__)
  return (int)__popcll(below);
#else
  return (int)__builtin_popcountll(below);
#endif
}
SF_HD inline bool record_mid_store(const Record &k, int a, int g, uint64_t ballot) {
  const int32_t used = rec_g(k.st)[(size_t)a * RC_WORDS + RC_USED];
  uint32_t c = rec_g(k.cmd)[(size_t)a * (size_t)k.n_agents + (size_t)g];
  const bool sub = record_unwritable(c);
  if (sub) c = (uint32_t)'+';
  rec_g(k.bytes)[(size_t)a * (size_t)k.bpa + (size_t)used + (size_t)record_rank(ballot, g)] = (uint8_t)c;
  return sub;
}
SF_HD inline void record_mid_finish(const Record &k, int a, int lines, int substituted) {
  auto *st = rec_g(k.st) + (size_t)a * RC_WORDS;
  st[RC_USED] = st[RC_USED] + lines, st[RC_SUBST] = st[RC_SUBST] + substituted;
}

// mode 2, lane 0, behind the second half (and k_ep_late): a game that check_end ended in this iteration is closed with its
// outcome.  The first half of every iteration clears SC_ENDED, so under auto_reset it says "ended in this iteration"
SF_HD inline void record_end(const Record &k, int a) {
  auto *st = rec_g(k.st) + (size_t)a * RC_WORDS;
  if (!st[RC_ACTIVE]) return;
  st[RC_ACTIVE] = 0;
  const auto *sc = rec_g(k.scal) + (size_t)a * SC_WORDS;
  if (k.auto_reset) {
    if (sc[SC_ENDED]) record_close(k, a, SF_RECORD_GAME_ENDED, rec_g(k.results)[(size_t)a * (size_t)k.n_agents * 8u + 7u]);
  } else if (sc[SC_DONE]) {
    record_close(k, a, SF_RECORD_GAME_ENDED, sc[SC_OUTCOME]);
  }
}

// mode 3, lane 0 (sf_record_flush)
SF_HD inline void record_flush(const Record &k, int a) {
  if (rec_g(k.st)[(size_t)a * RC_WORDS + RC_OPEN]) record_close(k, a, SF_RECORD_CUT, SF_RUNNING);
}

// ---- collection (sf_record_collect_device): k_record_plan, then k_record_copy ---------------------------------------------
// Output order is arena ascending, game ascending.  A game is delivered iff the games and bytes of everything in front
// of it in that order, plus its own, fit the limits: the delivered games are a prefix of the order, and a delivered
// game's place in the output is the sum over the games in front of it.
SF_HD inline void record_arena_totals(const Record &k, int a, int64_t &games, int64_t &bytes) {
  const auto *st = rec_g(k.st) + (size_t)a * RC_WORDS;
  games = st[RC_NGAMES], bytes = st[RC_START];
}
// gpre / bpre: the closed games / bytes of all arenas below a.  Writes the arena's plan row, adds what it delivers to
// tg / tb, moves its two since-the-last-collect counters into lost / subst.
SF_HD inline void record_plan_arena(const Record &k, int a, int64_t gpre, int64_t bpre, int64_t max_games, int64_t max_bytes,
                                    int64_t &tg, int64_t &tb, int64_t &lost, int64_t &subst) {
  auto *st = rec_g(k.st) + (size_t)a * RC_WORDS;
  const int32_t n = st[RC_NGAMES], closed = st[RC_START];
  const auto *r = rec_g(k.games) + (size_t)a * (size_t)k.G * RG_WORDS;
  int32_t take = 0, tbytes = 0;
  if (gpre + n <= max_games && bpre + closed <= max_bytes) {
    take = n, tbytes = closed;
  } else if (gpre < max_games && bpre <= max_bytes) {
    for (; take < n; ++take) {
      const int32_t end = r[(size_t)take * RG_WORDS + RG_OFF_LO] + r[(size_t)take * RG_WORDS + RG_LINES];
      if (gpre + take + 1 > max_games || bpre + end > max_bytes) break;
      tbytes = end;
    }
  }
  auto *pl = rec_g(k.plan) + (size_t)a * RPL_WORDS;
  pl[RPL_GBASE] = (int32_t)(take ? gpre : 0), pl[RPL_NTAKE] = take, pl[RPL_TBYTES] = tbytes;
  pl[RPL_BB_LO] = (int32_t)(uint32_t)(uint64_t)bpre, pl[RPL_BB_HI] = (int32_t)(uint32_t)((uint64_t)bpre >> 32);
  tg += take, tb += tbytes, lost += st[RC_LOST], subst += st[RC_SUBST];
  st[RC_LOST] = 0, st[RC_SUBST] = 0;
}

// k_record_copy, one wavefront per arena.  What a wave needs of the arena, loaded once in front of everything else:
struct RecordCopy {
  int32_t gbase, ntake, tbytes, ngames, used;
  int64_t bbase;
};
SF_HD inline RecordCopy record_copy_load(const Record &k, int a) {
  const auto *pl = rec_g(k.plan) + (size_t)a * RPL_WORDS;
  const auto *st = rec_g(k.st) + (size_t)a * RC_WORDS;
  RecordCopy c;
  c.gbase = pl[RPL_GBASE], c.ntake = pl[RPL_NTAKE], c.tbytes = pl[RPL_TBYTES];
  c.bbase = (int64_t)(((uint64_t)(uint32_t)pl[RPL_BB_HI] << 32) | (uint32_t)pl[RPL_BB_LO]);
  c.ngames = st[RC_NGAMES], c.used = st[RC_USED];
  return c;
}
// word i of the arena's delivered game records -> the dense list; the offset words become offsets in d_bytes
SF_HD inline void record_copy_game_word(const Record &k, const RecordCopy &c, int a, int32_t i, int32_t *d_games) {
  const auto *r = rec_g(k.games) + (size_t)a * (size_t)k.G * RG_WORDS;
  const int32_t w = i % RG_WORDS;
  int32_t v = r[i];
  if (w == RG_OFF_LO) v = (int32_t)(uint32_t)(uint64_t)(c.bbase + (int64_t)v);
  if (w == RG_OFF_HI) v = (int32_t)(uint32_t)((uint64_t)(c.bbase + (int64_t)r[i - 1]) >> 32);
  rec_g(d_games)[(size_t)c.gbase * RG_WORDS + (size_t)i] = v;
}
SF_HD inline void record_copy_byte(const Record &k, const RecordCopy &c, int a, int32_t i, uint8_t *d_bytes) {
  rec_g(d_bytes)[(size_t)c.bbase + (size_t)i] = rec_g(k.bytes)[(size_t)a * (size_t)k.bpa + (size_t)i];
}
// The compaction: what is left (pending games, the open game) moves to the front of the region and of the index, in
// ascending passes of 64.  A pass loads on every lane before any lane stores; the stores of a pass lie below every later
// load, so a move by fewer than 64 places is safe too.
SF_HD inline uint8_t record_compact_byte_load(const Record &k, const RecordCopy &c, int a, int32_t i) {
  return rec_g(k.bytes)[(size_t)a * (size_t)k.bpa + (size_t)c.tbytes + (size_t)i];
}
SF_HD inline void record_compact_byte_store(const Record &k, int a, int32_t i, uint8_t v) {
  rec_g(k.bytes)[(size_t)a * (size_t)k.bpa + (size_t)i] = v;
}
SF_HD inline int32_t record_compact_word_load(const Record &k, const RecordCopy &c, int a, int32_t i) {
  const int32_t v = rec_g(k.games)[((size_t)a * (size_t)k.G + (size_t)c.ntake) * RG_WORDS + (size_t)i];
  return i % RG_WORDS == RG_OFF_LO ? v - c.tbytes : v;
}
SF_HD inline void record_compact_word_store(const Record &k, int a, int32_t i, int32_t v) {
  rec_g(k.games)[(size_t)a * (size_t)k.G * RG_WORDS + (size_t)i] = v;
}
SF_HD inline void record_copy_finish(const Record &k, const RecordCopy &c, int a) {  // lane 0, behind everything else
  auto *st = rec_g(k.st) + (size_t)a * RC_WORDS;
  st[RC_NGAMES] = c.ngames - c.ntake, st[RC_USED] = c.used - c.tbytes, st[RC_START] = st[RC_START] - c.tbytes;
}

}  // namespace sf
