// examples/replay_sample.cpp — a game the reference client LOGGED (`.sf_sample`, gameplay.hpp:1784-1794,966-967) replayed
// through the C-ABI, with include/sf_sample.hpp: an offline game on the reference's own world (map/floor1-3.txt,
// 3 x 30 x 100), or a logged online match (Battle, several players) on the map it was played on.
//
//   g++ -std=c++17 -O2 -I include examples/replay_sample.cpp -L strikeforce_amd -lstrikeforce_amd
//       -Wl,-rpath,$PWD/strikeforce_amd -o /tmp/replay_sample
//   /tmp/replay_sample tests/golden/maps game.sf_sample <mode 0 Solo | 1 Timer | 2 Squad> <level> [copy.sf_sample]
//   /tmp/replay_sample <maps dir> match.sf_sample 3 1 <copy.sf_sample | -> <teams, e.g. 1,2,3> <floors> <rows> <cols>
//       <H> <Z> <B> <P>
//
// A match file as the reference logged it holds only the team of the logging player (sf_sample.hpp Layout::Logged), so
// the teams are an argument; <maps dir>/floor1.txt ... hold the match's map in the reference's text format; the copy is
// written in the layout the reference's own replay mode reads (Layout::Replay).  Built with -DSF_REPLAY_ON_DEVICE the
// lines are fetched on the device (sf_replay_load / sf_replay_step) instead of through sf_step / the split step.
//
// Prints the sample's header, the number of iterations played and the final state digest — for a match also how the
// replay ended and how many lines it took; with a fifth argument the sample is written out again (the reference's byte
// layout: the copy replays in the reference itself).
#include <cstdio>
#include <cstdlib>

#include "sf_sample.hpp"

int main(int argc, char **argv) {
  if (argc < 5) return fprintf(stderr, "usage: %s <maps dir> <sample> <mode> <level> [copy [teams floors rows cols H Z B P]]\n", argv[0]), 2;
  sf::Sample s;
  std::string why;
  std::vector<int> teams;
  if (argc > 6) {
    std::string list(argv[6]);
    for (char &c : list)
      if (c == ',') c = ' ';
    std::istringstream in(list);
    for (int t; in >> t;) teams.push_back(t);
  }
  if (!sf::read_sample(argv[2], s, &why, sf::Layout::Auto, teams.empty() ? nullptr : &teams))
    return fprintf(stderr, "%s: %s\n", argv[2], why.c_str()), 1;
  sf_config cfg;
  sf_config_defaults(&cfg);
  cfg.arenas = 1, cfg.floors = 3, cfg.rows = 30, cfg.cols = 100;  // gameplay.hpp:37
  // pools for a whole game of the reference (its own hold 9000): 1024 zombies and 512 exits live in the arena's LDS
  cfg.cap_humans = 64, cfg.cap_zombies = 1024, cfg.cap_bullets = 256, cfg.cap_portals = 512, cfg.cap_chests = 9000;
  cfg.mode = atoi(argv[3]), cfg.level = atoi(argv[4]), cfg.n_agents = 1, cfg.auto_reset = 0;
  cfg.timer_frames_per_level = 1 << 20;
  cfg.player = sf::profile_of(s.record);  // the record comes from the file (Human::scan_file, Character.hpp:570-617)
  if (s.players > 1) {  // a match: Battle, every player's record and team from the file (and the command line)
    if (argc < 14) return fprintf(stderr, "a match file needs: copy teams floors rows cols H Z B P\n"), 2;
    if (!sf::match_config(s, cfg)) return fprintf(stderr, "%s: a team is unknown\n", argv[2]), 1;
    cfg.floors = atoi(argv[7]), cfg.rows = atoi(argv[8]), cfg.cols = atoi(argv[9]);
    cfg.cap_humans = atoi(argv[10]), cfg.cap_zombies = atoi(argv[11]), cfg.cap_bullets = atoi(argv[12]), cfg.cap_portals = atoi(argv[13]);
  }
  std::string chars;
  std::vector<int16_t> portal;
  if (!sf::load_reference_maps(argv[1], cfg.floors, cfg.rows, cfg.cols, chars, portal)) return fprintf(stderr, "cannot read the maps in %s\n", argv[1]), 1;
  cfg.map = chars.data(), cfg.map_portal = portal.data();
  sf_env *env = nullptr;
  if (sf_create(&cfg, &env) != SF_OK) return fprintf(stderr, "sf_create: %s\n", sf_last_error()), 1;
  sf::ReplayEnd end;
#ifdef SF_REPLAY_ON_DEVICE
  const long n = sf::replay_on_device(env, s, &end);
#else
  const long n = sf::replay(env, s, &end);
#endif
  if (n < 0) return fprintf(stderr, "replay: %s\n", sf_last_error()), 1;
  uint64_t digest = 0;
  sf_state_digest(env, &digest);
  printf("sample tb %llu serial %llu ind %d team %d name %s commands %zu\n", (unsigned long long)s.tb, (unsigned long long)s.serial, s.ind,
         s.team, s.name.c_str(), s.commands.size());
  printf("iterations %ld\ndigest %016llx\n", n, (unsigned long long)digest);
  if (s.players > 1) {
    static const char *const states[] = {"running", "game ended", "sample ended", "truncated"};
    printf("players %d\nstate %s\ncursor %ld\n", s.players, states[end.state & 3], end.cursor);
  }
  const bool copy = argc > 5 && std::string(argv[5]) != "-";
  if (copy && !sf::write_sample(argv[5], s, s.players > 1 ? sf::Layout::Replay : sf::Layout::Logged)) return fprintf(stderr, "cannot write %s\n", argv[5]), 1;
  sf_destroy(env);
  return 0;
}
