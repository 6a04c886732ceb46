// sf_sample.hpp — the reference's `.sf_sample` trajectory format for C++ hosts of the C-ABI (header-only).
//
// A `.sf_sample` file is what the reference client writes while a game is played with logging on
// (StrikeForce-client/gameplay.hpp:1784-1794 opens it and writes the header, :1910-1914 the player's blob,
// :966-967 one command per loop iteration) and reads back in replay mode (:1749-1782, :968-969).  The player's blob is
// Human::log_file (Character.hpp:619-648), read by Human::scan_file (:570-617): the name and the 32 integers of the
// character record, one per line.  Offline (Solo / Timer / Squad) files look like
//
//     <tb> <serial>
//     1 <ind> <team>
//     <name>
//     <def_Hp> ... 31 more integers, one per line
//     <one command char per loop iteration, one per line>
//
// Online files (a Battle match, players > 1) come in two layouts, because the reference's writer and reader disagree:
//   Layout::Logged  what the reference WRITES (gameplay.hpp:1836-1845): `tb serial` / `players ind team(ind)` / the blob
//                   of `ind` / the blob of every other player in slot order / the command lines.  No other team.
//   Layout::Replay  what the reference READS (gameplay.hpp:1762-1778,1796-1806): three leading tokens (ip, port,
//                   password, thrown away), `tb serial`, `players ind team`, the blob of `ind`, then for every other slot
//                   its blob FOLLOWED BY ITS TEAM, then the command lines.
// So the reference cannot replay its own online log as written; read here as Logged with the teams supplied and written
// as Replay, it can.  A match's command lines are, per iteration, the command of `ind`, then one for every other player
// alive and remote when human_action runs, slots ascending (gameplay.hpp:966-967,979-986).
//
// sf::read_sample / sf::write_sample read and write these layouts (a file written here replays in the reference, one
// the reference logged replays here: tests/test_cpp_sample.py does both against the reference's own build);
// sf::replay feeds a sample to an sf_env through sf_reset / sf_step / sf_done, a match through the split step
// (sf_step_begin / sf_agent_alive / sf_step_end); sf::replay_on_device through sf_replay_load / sf_replay_step, the lines
// fetched on the device; sf::samples_of_recording turns what a recorder collected (sf_record_collect: games played here,
// written out on the device as these command lines) into Samples.  Python twin: strikeforce_amd/replay.py.
#ifndef SF_SAMPLE_HPP
#define SF_SAMPLE_HPP

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <array>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "strikeforce.h"

namespace sf {

enum class Layout { Auto, Logged, Replay };

struct Sample {
  uint64_t tb = 0, serial = 0;  // the seed pair of the game: gameplay.hpp:1745-1746 (`_srand(tb, serial_number)`)
  int players = 1, ind = 0, team = 1;
  std::string name = "player";
  int32_t record[32] = {0};     // the character record of `ind`, Character.hpp:669-689 (33 tokens minus the name)
  std::string commands;         // the reference command chars in file order (gameplay.hpp:45 + '_')
  // a match (players > 1): every player's name, record and team by slot (the entries of `ind` repeat the fields above);
  // team -1 = the file does not say (Layout::Logged only holds the team of `ind`).  Empty for an offline sample
  std::vector<std::string> names;
  std::vector<std::array<int32_t, 32>> records;
  std::vector<int> teams;
  std::string ip = "0.0.0.0", port = "0", password = "-";  // the three tokens Layout::Replay starts with
};

// sf_profile is those 32 integers in file order (include/strikeforce.h)
static_assert(sizeof(sf_profile) == 32 * sizeof(int32_t), "sf_profile = the 32 integers of a character record");
inline sf_profile profile_of(const int32_t record[32]) {
  sf_profile p;
  memcpy(&p, record, sizeof p);
  return p;
}

namespace detail {
inline bool is_int(const std::string &t) {
  if (t.empty()) return false;
  char *end = nullptr;
  (void)strtoll(t.c_str(), &end, 10);
  return end && *end == 0;
}
// the tokens of one file in one explicit layout
inline bool parse(std::vector<std::string> tok, Layout layout, const std::vector<int> *teams, Sample &s, std::string &why) {
  auto fail = [&](const std::string &m) {
    why = m;
    return false;
  };
  s = Sample();
  if (layout == Layout::Replay && !(tok.size() > 2 && is_int(tok[0]) && is_int(tok[1]) && tok[2] == "1")) {
    if (tok.size() < 3) return fail("header: expected `tb serial` and `players ind team`");
    s.ip = tok[0], s.port = tok[1], s.password = tok[2];  // (an offline file has no such tokens: gameplay.hpp:1762)
    tok.erase(tok.begin(), tok.begin() + 3);
  }
  if (tok.size() < 5 + 33) return fail("header: expected `tb serial` and `players ind team`");
  for (int i = 0; i < 5; ++i)
    if (!is_int(tok[i])) return fail("header: expected `tb serial` and `players ind team`");
  s.tb = strtoull(tok[0].c_str(), nullptr, 10), s.serial = strtoull(tok[1].c_str(), nullptr, 10);
  s.players = atoi(tok[2].c_str()), s.ind = atoi(tok[3].c_str()), s.team = atoi(tok[4].c_str());
  if (s.players < 1 || s.players > SF_MAX_AGENTS || s.ind < 0 || s.ind >= s.players)
    return fail("header: players must be 1..16 and ind one of them");
  size_t pos = 5;
  s.names.assign(s.players, ""), s.records.assign(s.players, {}), s.teams.assign(s.players, -1);
  s.teams[s.ind] = s.team;
  for (int k = 0; k < s.players; ++k) {
    const int i = k == 0 ? s.ind : (k <= s.ind ? k - 1 : k);  // `ind` first, then the other slots ascending
    if (pos + 33 > tok.size()) return fail("character record: fewer than 32 integers");
    s.names[i] = tok[pos];
    for (int j = 0; j < 32; ++j) {
      if (!is_int(tok[pos + 1 + j])) return fail("character record: fewer than 32 integers");
      s.records[i][j] = atoi(tok[pos + 1 + j].c_str());
    }
    pos += 33;
    if (layout == Layout::Replay && i != s.ind) {
      if (pos >= tok.size() || !is_int(tok[pos])) return fail("layout Replay: the team of a player is missing behind its record");
      s.teams[i] = atoi(tok[pos++].c_str());
    }
  }
  s.name = s.names[s.ind];
  memcpy(s.record, s.records[s.ind].data(), sizeof s.record);
  if (s.players > 1 && layout == Layout::Logged) {
    if (!teams)
      return fail("a logged online sample holds only the team of `ind`: pass the teams, one per player (Layout::Logged, "
                  "gameplay.hpp:1836-1845)");
    if ((int)teams->size() != s.players || (*teams)[s.ind] != s.team)
      return fail("teams needs one entry per player, and teams[ind] must be the file's own");
    s.teams = *teams;
  }
  if (s.players == 1) s.names.clear(), s.records.clear(), s.teams.clear();
  // `replay_file >> command[i]` reads a char: a token "ab" is two commands
  for (; pos < tok.size(); ++pos) s.commands += tok[pos];
  return true;
}
}  // namespace detail

// Parses the way the reference does: whitespace-separated tokens (`operator>>`), commands one char at a time.  An
// explicit layout is taken as exactly that, never guessed.  Layout::Auto: the file is taken as Logged if it parses as
// such — five integers, then a name and 32 integers per player — and otherwise as Replay, i.e. the same behind three
// leading tokens (an IP address is no integer, so a Replay file never parses as Logged).  teams: the team of every
// player, for a Logged match file; reading one without them is an error that says so.  Offline files (players == 1)
// read the same in every layout.  Returns false (and says why) on a file that fits no layout asked for.
inline bool read_sample(const std::string &path, Sample &s, std::string *why = nullptr, Layout layout = Layout::Auto,
                        const std::vector<int> *teams = nullptr) {
  std::string w;
  auto done = [&](bool ok) {
    if (!ok && why) *why = w;
    return ok;
  };
  std::ifstream f(path.c_str());
  if (!f) return w = "cannot open the file", done(false);
  std::vector<std::string> tok;
  for (std::string t; f >> t;) tok.push_back(t);
  if (layout != Layout::Auto) return done(detail::parse(tok, layout, teams, s, w));
  if (detail::parse(tok, Layout::Logged, teams, s, w)) return true;
  if (!tok.empty() && detail::is_int(tok[0])) return done(false);  // it begins like a Logged file: that complaint is the useful one
  std::string w2;
  if (detail::parse(tok, Layout::Replay, teams, s, w2)) return true;
  w = "neither layout fits: as Logged: " + w + "; as Replay: " + w2;
  return done(false);
}

// The reference logger's byte layout: header, Human::log_file blob(s), then `command << '\n'` per line.  Layout::Logged
// (and Auto): what the reference writes; Layout::Replay: what its replay mode reads — every team must be known.  An
// offline sample is the same bytes whatever the layout.
inline bool write_sample(const std::string &path, const Sample &s, Layout layout = Layout::Logged) {
  const bool as_replay = s.players > 1 && layout == Layout::Replay;
  if (s.players > 1 && ((int)s.names.size() != s.players || (int)s.records.size() != s.players || (int)s.teams.size() != s.players))
    return false;
  if (as_replay)
    for (int t : s.teams)
      if (t < 0) return false;
  std::ofstream f(path.c_str());
  if (!f) return false;
  if (as_replay) f << s.ip << '\n' << s.port << '\n' << s.password << '\n';
  f << s.tb << ' ' << s.serial << '\n' << s.players << ' ' << s.ind << ' ' << s.team << '\n' << s.name << '\n';
  for (int i = 0; i < 32; ++i) f << s.record[i] << '\n';
  for (int p = 0; p < s.players; ++p) {
    if (p == s.ind) continue;
    f << s.names[p] << '\n';
    for (int i = 0; i < 32; ++i) f << s.records[p][i] << '\n';
    if (as_replay) f << s.teams[p] << '\n';
  }
  for (char c : s.commands) f << c << '\n';
  return (bool)f;
}

// The part of an sf_config a logged match fixes, as the logging client saw it: Battle mode, n_agents = players, `ind`,
// the teams and one character record per player from the file's blobs.  False if a team is unknown.
inline bool match_config(const Sample &s, sf_config &cfg) {
  if (s.players < 2) return false;
  for (int t : s.teams)
    if (t < 0) return false;
  cfg.mode = SF_MODE_BATTLE, cfg.level = 1, cfg.n_agents = s.players, cfg.ind = s.ind, cfg.auto_reset = 0;
  cfg.player = profile_of(s.record);
  cfg.n_agent_profiles = s.players;
  for (int i = 0; i < s.players; ++i) cfg.agent_team[i] = s.teams[i], cfg.agent_profile[i] = profile_of(s.records[i].data());
  return true;
}

// map/floor1.txt .. floor<floors>.txt of a reference checkout, read the way gameplay::setup() does
// (gameplay.hpp:1249-1274: `f >> c`, a '^' or 'v' is followed by the number of the exit it leads to; any character other
// than # . O ^ v is an empty cell): fills what sf_config::map / map_portal point at.
inline bool load_reference_maps(const std::string &dir, int floors, int rows, int cols, std::string &chars,
                                std::vector<int16_t> &portal) {
  chars.clear(), portal.clear();
  for (int k = 1; k <= floors; ++k) {
    std::ifstream f((dir + "/floor" + std::to_string(k) + ".txt").c_str());
    if (!f) return false;
    for (int i = 0; i < rows * cols; ++i) {
      char c;
      int idx = -1;
      if (!(f >> c)) return false;
      if (c == '^' || c == 'v') {
        if (!(f >> idx)) return false;
      } else if (c != '#' && c != 'O') {
        c = '.';
      }
      chars.push_back(c);
      portal.push_back((int16_t)idx);
    }
  }
  return true;
}

// How a replay ended (SF_REPLAY_* of strikeforce.h), the lines it took and the iterations it played
struct ReplayEnd {
  int state = SF_REPLAY_RUNNING;
  long cursor = 0, iterations = 0;
};

// Replays the sample on `env` — created for ONE arena with cfg.player = profile_of(sample.record) (a match:
// match_config), auto_reset off and the mode / level / map of the logged game — the way the reference's replay loop does.
// Offline: one command per iteration until the game ends (gameplay.hpp:1450 `if(check_end()) break;`) or the commands run
// out.  A match: the lines fetched on the host through the split step — the command of `ind` at the loop top, after
// sf_step_begin one line for every other commanded human sf_agent_alive reports, slots ascending, '+' for the rest —
// until the game ends, the lines run out at a loop top, or, a stream cut in mid-iteration, at the loop top after it
// (`end`, if given, says which).  Returns the number of iterations played, or a negative SF_ERR_* code.
inline long replay(sf_env *env, const Sample &s, ReplayEnd *end = nullptr) {
  const uint64_t tb = s.tb, serial = s.serial;
  int rc = sf_reset(env, &tb, &serial);
  if (rc != SF_OK) return rc;
  long n = 0;
  if (s.players <= 1) {
    for (char c : s.commands) {
      uint8_t done = 0;
      if ((rc = sf_done(env, &done)) != SF_OK) return rc;
      if (done) break;
      const uint8_t cmd = (uint8_t)c;
      if ((rc = sf_step(env, &cmd)) != SF_OK) return rc;
      ++n;
    }
    return n;
  }
  ReplayEnd e;
  size_t cur = 0;
  bool cut = false;
  for (;;) {
    uint8_t done = 0;
    if ((rc = sf_done(env, &done)) != SF_OK) return rc;
    if (cut) e.state = SF_REPLAY_TRUNCATED;
    else if (done) e.state = SF_REPLAY_GAME_ENDED;
    else if (cur == s.commands.size()) e.state = SF_REPLAY_SAMPLE_ENDED;
    if (e.state != SF_REPLAY_RUNNING) break;
    uint8_t cmd[SF_MAX_AGENTS], alive[SF_MAX_AGENTS];
    memset(cmd, '+', sizeof cmd);
    cmd[s.ind] = (uint8_t)s.commands[cur++];
    if ((rc = sf_step_begin(env)) != SF_OK || (rc = sf_agent_alive(env, alive)) != SF_OK) return rc;
    for (int g = 0; g < s.players; ++g) {
      if (g == s.ind || !alive[g]) continue;
      if (cur < s.commands.size())
        cmd[g] = (uint8_t)s.commands[cur++];
      else
        cut = true;
    }
    if ((rc = sf_step_end(env, cmd)) != SF_OK) return rc;
    ++n;
  }
  e.cursor = (long)cur, e.iterations = n;
  if (end) *end = e;
  return n;
}

// The same replay with the lines fetched on the device (sf_replay_load / sf_replay_step: no host round trip inside an
// iteration), for any number of players; steps until the arena has stopped.  Other than sf::replay it leaves an arena
// whose lines ran out stopped (done = 1, outcome = SF_SAMPLE_END).  Returns the iterations played or a negative code.
inline long replay_on_device(sf_env *env, const Sample &s, ReplayEnd *end = nullptr) {
  const uint64_t tb = s.tb, serial = s.serial;
  const int64_t off[2] = {0, (int64_t)s.commands.size()};
  int rc = sf_reset(env, &tb, &serial);
  if (rc != SF_OK || (rc = sf_replay_load(env, reinterpret_cast<const uint8_t *>(s.commands.data()), off)) != SF_OK) return rc;
  int32_t st[4] = {0, 0, 0, 0};
  for (;;) {
    uint8_t done = 0;
    if ((rc = sf_replay_status(env, st)) != SF_OK || (rc = sf_done(env, &done)) != SF_OK) return rc;
    if (st[0] != SF_REPLAY_RUNNING && done) break;
    for (int k = 0; k < 16; ++k)
      if ((rc = sf_replay_step(env)) != SF_OK) return rc;
  }
  if (end) end->state = st[0], end->cursor = st[1], end->iterations = st[2];
  return st[2];
}

// What a recorder says about one game beside its sample: the words of its game record that are no part of the file
struct RecordedGame {
  int32_t arena = 0, episode = 0, iterations = 0, end = 0 /* SF_RECORD_* */, outcome = SF_RUNNING;
};

// The games a recorder collected (sf_record_collect: `n_games` records of SF_RECORD_GAME_WORDS int32 and the streams back
// to back, `n_bytes` of them) as Samples, one per game in the order delivered: seed and command stream from the recording;
// players, `ind`, the teams, names and character records — which the recorder does not know — from `like` (a sample of a
// match these games resemble, or one filled in by hand).  write_sample then produces files the reference reads.  Returns
// false if a game's stream lies outside the bytes given.  Python twin: replay.samples_from_recording.
inline bool samples_of_recording(const int32_t *games, int64_t n_games, const uint8_t *bytes, int64_t n_bytes, const Sample &like,
                                 std::vector<Sample> &out, std::vector<RecordedGame> *info = nullptr) {
  out.clear();
  if (info) info->clear();
  for (int64_t i = 0; i < n_games; ++i) {
    const int32_t *g = games + i * SF_RECORD_GAME_WORDS;
    auto u64 = [&](int lo) { return ((uint64_t)(uint32_t)g[lo + 1] << 32) | (uint64_t)(uint32_t)g[lo]; };
    const int64_t off = (int64_t)u64(10), lines = g[6];
    if (off < 0 || lines < 0 || off > n_bytes || lines > n_bytes - off) return false;
    Sample s = like;
    s.tb = u64(2), s.serial = u64(4);
    s.commands.assign(reinterpret_cast<const char *>(bytes) + off, (size_t)lines);
    out.push_back(s);
    if (info) {
      RecordedGame r;
      r.arena = g[0], r.episode = g[1], r.iterations = g[7], r.end = g[8], r.outcome = g[9];
      info->push_back(r);
    }
  }
  return true;
}

}  // namespace sf
#endif  // SF_SAMPLE_HPP
