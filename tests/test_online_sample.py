"""Online `.sf_sample` files: two matches that the reference's own client logged on the reference's own
server (tests/golden/online_plain.sf_sample, online_quit.sf_sample, committed as it wrote them; make_online_sample.py)
are read in Python and in C++, written back byte for byte in the layout the reference writes ("logged",
gameplay.hpp:1836-1845) and converted to the one its replay mode reads ("replay", :1762-1778,1796-1806), and replayed
with the lines fetched on the host (strikeforce_amd.replay.replay_lines) on the oracle and on the wave emulator to the
reference client's own state digest after every iteration.  No reference checkout needed."""
import os
import subprocess

import numpy as np
import pytest

import online_cases as oc
from emu_lib import Emu
from oracle_lib import Oracle, ROOT
from strikeforce_amd import abi, config, replay

HEADER, BLOB = 2 + 3, 33


def test_the_fixtures_hold_what_the_reference_logged():
    plain, fp = oc.load("online_plain")
    quit_, fq = oc.load("online_quit")
    for s, f in ((plain, fp), (quit_, fq)):
        assert (s.players, s.ind, s.team, s.teams) == (3, 1, 2, [1, 2, 3])
        assert (s.tb, s.serial) == (f["tb"], f["serial"])
        assert s.records == [oc.RECORD] * 3 and s.profile_tokens == oc.RECORD
        assert all(c in abi.ALL_COMMANDS for c in s.commands)
    # 120 iterations of three lines; with the quit 51 iterations of three, then 69 of two: the number of lines per
    # iteration depends on the game
    assert len(open(oc.path_of("online_plain")).read().split()) == HEADER + BLOB * 3 + 3 * 120 == 464
    assert len(open(oc.path_of("online_quit")).read().split()) == HEADER + BLOB * 3 + 3 * 51 + 2 * 69 == 395
    assert len(plain.commands) == 3 * 120 and len(quit_.commands) == 3 * 51 + 2 * 69
    assert len(fp["digests"]) == len(fq["digests"]) == 121


@pytest.mark.parametrize("name", oc.NAMES)
def test_layouts_round_trip_byte_for_byte(name, tmp_path):
    s, f = oc.load(name)
    original = open(oc.path_of(name), "rb").read()
    a, b, c = (str(tmp_path / n) for n in ("logged", "replay", "again"))
    replay.write_sample(a, s, layout="logged")
    assert open(a, "rb").read() == original
    # logged -> replay -> logged
    replay.write_sample(b, s, layout="replay")
    tok = open(b).read().split()
    assert len(tok) == len(original.split()) + 3 + 2  # ip, port, password in front; a team behind each other blob
    for how in ("replay", "auto"):
        r = replay.read_sample(b, layout=how)
        assert (r.tb, r.serial, r.players, r.ind, r.teams, r.names, r.records, r.commands) == (
            s.tb, s.serial, 3, 1, [1, 2, 3], s.names, s.records, s.commands)
        replay.write_sample(c, r, layout="logged")
        assert open(c, "rb").read() == original
    # "auto" takes the reference's own file as "logged"; an explicit layout never guesses
    assert replay.read_sample(oc.path_of(name), teams=f["teams"]).commands == s.commands
    with pytest.raises(ValueError):
        replay.read_sample(oc.path_of(name), layout="replay")
    with pytest.raises(ValueError):
        replay.read_sample(b, layout="logged", teams=f["teams"])


@pytest.mark.parametrize("layout", ["auto", "logged"])
def test_a_logged_match_without_the_teams_is_refused(layout):
    with pytest.raises(ValueError, match="holds only the team of `ind`: pass teams="):
        replay.read_sample(oc.path_of("online_quit"), layout=layout)
    with pytest.raises(ValueError, match="teams"):
        replay.read_sample(oc.path_of("online_quit"), layout=layout, teams=[1, 1, 3])  # not the file's own team of `ind`
    s, _ = oc.load("online_quit")
    s.teams[0] = None
    with pytest.raises(ValueError, match="team"):
        replay.write_sample(os.devnull, s, layout="replay")


def test_offline_samples_are_what_they_were(tmp_path):
    """The files of tests/test_replay.py: the same bytes in both directions whatever the layout says."""
    rng = np.random.RandomState(7)
    cmds = "".join(abi.BENCH_COMMANDS[i] for i in rng.randint(0, 28, size=400))
    s = replay.Sample(1771155561, 1073741823, config.HUMAN_ENEMY_TOKENS, cmds, name="1")
    want = "1771155561 1073741823\n1 0 1\n1\n" + "".join("%d\n" % t for t in config.HUMAN_ENEMY_TOKENS) + "".join(c + "\n" for c in cmds)
    for wl in replay.LAYOUTS:
        p = str(tmp_path / ("w_" + wl))
        replay.write_sample(p, s, layout=wl)
        assert open(p).read() == want
        for rl in replay.LAYOUTS:
            r = replay.read_sample(p, layout=rl)
            assert (r.tb, r.serial, r.players, r.ind, r.team, r.name, r.profile_tokens, r.commands) == (
                s.tb, s.serial, 1, 0, 1, "1", s.profile_tokens, cmds)
            q = str(tmp_path / "again")
            replay.write_sample(q, r, layout=rl)
            assert open(q).read() == want


def _expected_lines(name):
    s, f = oc.load(name)
    q = f["quit"]
    alive = [[g for g in range(3) if g != s.ind and not (q and g == q[0] and it > q[1])] for it in range(f["iterations"])]
    return oc.lines_per_iteration(s, alive)


@pytest.mark.parametrize("impl", [Oracle, Emu], ids=["oracle", "emulator"])
@pytest.mark.parametrize("name", oc.NAMES)
def test_the_replay_reproduces_the_reference_clients_digests(name, impl):
    """All 121 digests of the reference client's own dumps (after the placement and after every iteration), every line
    consumed, "sample ended"; the lines each iteration took are the file's, none for the player that has left."""
    s, f = oc.load(name)
    sim = impl(oc.workload(s, f))
    digests, taken = [], []

    def on_iteration(n, sim_, row):
        digests.append("%016x" % int(sim_.digest()[0]))
        if n:
            taken.append([int(x) for x in row])

    end = replay.replay_lines(s, sim, on_iteration)
    differing = [i for i, (a, b) in enumerate(zip(digests, f["digests"])) if a != b]
    assert len(digests) == 121 and differing == []
    assert end == (120, abi.REPLAY_SAMPLE_ENDED, len(s.commands))
    assert taken == _expected_lines(name)
    if f["quit"]:
        assert all(row[f["quit"][0]] == 0 for row in taken[f["quit"][1] + 1:]) and taken[f["quit"][1]][f["quit"][0]] == ord("_")
    assert replay.replay(s, impl(oc.workload(s, f))) == 120


def test_a_stream_cut_in_mid_iteration_ends_truncated():
    s, f = oc.load("online_plain")
    whole = s.commands
    s.commands = whole[:3 * 40 + 2]  # iteration 41 has the line of `ind` and of player 0, none for player 2
    a, b = Oracle(oc.workload(s, f)), Oracle(oc.workload(s, f))
    assert replay.replay_lines(s, a) == (41, abi.REPLAY_TRUNCATED, 3 * 40 + 2)
    s.commands = whole[:3 * 40 + 2] + "+"  # the same game: a human without a line obeys '+'
    assert replay.replay_lines(s, b) == (41, abi.REPLAY_SAMPLE_ENDED, 3 * 41)
    assert int(a.digest()[0]) == int(b.digest()[0])


def test_a_game_that_ends_leaves_the_rest_unread():
    s, f = oc.load("online_plain")
    s.commands = s.commands[:3 * 10] + "_" + s.commands[3 * 10 + 1:]  # `ind` gives up in iteration 11 (gameplay.hpp:696-699)
    sim = Oracle(oc.workload(s, f))
    end = replay.replay_lines(s, sim)
    assert end.state == abi.REPLAY_GAME_ENDED and end.iterations < 20 and end.cursor == 3 * end.iterations
    assert sim.done()[0]


# ---- include/sf_sample.hpp, through examples/replay_sample.cpp on the emulator-backed test library --------------------
def _build(tmp_path):
    d = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-s", "-C", d, "libsf_emu_abi.so"])
    exe = str(tmp_path / "replay_sample")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "replay_sample.cpp"), "-L", d, "-lsf_emu_abi", "-Wl,-rpath," + d,
                           "-o", exe])
    return exe


def match_args(f, maps_dir):
    chars, portal = oc.map_of(f)
    os.makedirs(maps_dir, exist_ok=True)
    with open(os.path.join(maps_dir, "floor1.txt"), "w") as fh:
        fh.write(config.format_floor_text(bytes(chars).decode("ascii"), list(portal), f["map"]["rows"], f["map"]["cols"]))
    p = f["pools"]
    return [",".join(map(str, f["teams"])), "1", str(f["map"]["rows"]), str(f["map"]["cols"]), str(p["H"]), str(p["Z"]),
            str(p["B"]), str(p["P"])]


@pytest.mark.parametrize("name", oc.NAMES)
def test_the_cpp_header_reads_replays_and_converts_the_fixtures(name, tmp_path):
    s, f = oc.load(name)
    exe = _build(tmp_path)
    maps, copy = str(tmp_path / "maps"), str(tmp_path / "copy.sf_sample")
    out = subprocess.check_output([exe, maps, oc.path_of(name), "3", "1", copy] + match_args(f, str(tmp_path / "maps")), text=True)
    lines = out.strip().split("\n")
    kv = dict(ln.split(" ", 1) for ln in lines[1:])
    assert lines[0] == "sample tb %d serial %d ind 1 team 2 name %s commands %d" % (s.tb, s.serial, s.name, len(s.commands))
    assert (kv["players"], kv["state"], int(kv["cursor"]), int(kv["iterations"])) == ("3", "sample ended", len(s.commands), 120)
    assert kv["digest"] == f["digests"][-1]
    # the copy: the layout the reference's replay mode reads, the bytes the Python twin writes
    twin = str(tmp_path / "twin.sf_sample")
    replay.write_sample(twin, s, layout="replay")
    assert open(copy, "rb").read() == open(twin, "rb").read()
    # and without the teams the C++ reader refuses the file, saying why
    r = subprocess.run([exe, maps, oc.path_of(name), "3", "1"], capture_output=True, text=True)
    assert r.returncode == 1 and "pass the teams" in r.stderr
