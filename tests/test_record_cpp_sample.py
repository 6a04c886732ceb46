"""sf::samples_of_recording (include/sf_sample.hpp), the C++ twin of replay.samples_from_recording: a game record and a
stream put together by hand for a fixture match give, through sf::write_sample, the reference client's own file."""
import os
import subprocess

import online_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = r'''
#include <cstdio>
#include "sf_sample.hpp"
int main(int argc, char **argv) {
  if (argc != 4) return 2;
  sf::Sample like;
  std::string why;
  const std::vector<int> teams = {1, 2, 3};
  if (!sf::read_sample(argv[1], like, &why, sf::Layout::Logged, &teams)) return fprintf(stderr, "%s\n", why.c_str()), 3;
  // two games in one collection: five bytes of another game first, then the fixture's lines
  std::vector<uint8_t> bytes = {'w', 'a', 's', 'd', '+'};
  bytes.insert(bytes.end(), like.commands.begin(), like.commands.end());
  const int32_t lines = (int32_t)like.commands.size();
  const int32_t games[2 * SF_RECORD_GAME_WORDS] = {
      7, 3, -5, 1, 9, 0, 5, 2, SF_RECORD_BROKEN, SF_RUNNING, 0, 0,
      0, 0, (int32_t)(uint32_t)like.tb, (int32_t)(like.tb >> 32), (int32_t)(uint32_t)like.serial, (int32_t)(like.serial >> 32), lines, 120,
      SF_RECORD_CUT, SF_RUNNING, 5, 0};
  std::vector<sf::Sample> out;
  std::vector<sf::RecordedGame> info;
  if (!sf::samples_of_recording(games, 2, bytes.data(), (int64_t)bytes.size(), like, out, &info) || out.size() != 2) return 4;
  if (out[0].commands != "wasd+" || out[0].tb != ((1ull << 32) | 0xfffffffbull) || out[0].serial != 9 || info[0].arena != 7 ||
      info[0].episode != 3 || info[0].iterations != 2 || info[0].end != SF_RECORD_BROKEN || info[1].end != SF_RECORD_CUT)
    return 5;
  if (sf::samples_of_recording(games, 2, bytes.data(), (int64_t)bytes.size() - 1, like, out)) return 6;  // a stream past the end
  if (!sf::samples_of_recording(games, 2, bytes.data(), (int64_t)bytes.size(), like, out)) return 7;
  return sf::write_sample(argv[2], out[1], sf::Layout::Logged) && sf::write_sample(argv[3], out[0], sf::Layout::Replay) ? 0 : 8;
}
'''


def test_a_collection_becomes_the_reference_clients_file(tmp_path):
    src, exe = tmp_path / "rec.cpp", tmp_path / "rec"
    src.write_text(PROGRAM)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)])
    for name in oc.NAMES:
        out, other = tmp_path / (name + ".sf_sample"), tmp_path / (name + "_other.sf_sample")
        subprocess.check_call([str(exe), oc.path_of(name), str(out), str(other)])
        assert out.read_bytes() == open(oc.path_of(name), "rb").read()
        assert other.read_text().split()[-5:] == list("wasd+")
