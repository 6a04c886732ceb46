"""include/sf_sample.hpp (the reference's `.sf_sample` format for C++ hosts of the C-ABI) through examples/replay_sample.cpp:
a game LOGGED by the reference itself (oracle/_ref/sf_ref_tick, gameplay.hpp:1784-1794,966-967) is read and replayed by
the C++ program to the reference's own replay of that file; the copy the program writes is byte-identical to what
strikeforce_amd.replay writes and is replayed by the reference in turn.  CPU: linked against the emulator-backed test
library (tests/emu/libsf_emu_abi.so); -m gpu: against libstrikeforce_amd.so, compared with the oracle's digest."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ref_cases
import reftick
from oracle_lib import Oracle
from strikeforce_amd import abi, config, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = os.path.join(ROOT, "tests", "golden", "maps")
RICH = ref_cases.RICH
STRONG1 = list(RICH[:3]) + [1, 1, 1] + list(RICH[6:])


def build(tmp_path, lib_dir, lib_name):
    exe = str(tmp_path / "replay_sample")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "replay_sample.cpp"), "-L", lib_dir, "-l" + lib_name,
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    return exe


def emu_lib():
    d = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-s", "-C", d, "libsf_emu_abi.so"])  # (a no-op when it is up to date)
    return d, "sf_emu_abi"


def run(exe, sample, mode, level, copy=None):
    out = subprocess.check_output([exe, MAPS, sample, str(mode), str(level)] + ([copy] if copy else []), text=True)
    kv = dict(ln.split(" ", 1) for ln in out.strip().split("\n")[1:])
    return out.split("\n")[0], int(kv["iterations"]), kv["digest"]


def commands(n, seed):
    rng = np.random.RandomState(seed)
    return "".join(abi.BENCH_COMMANDS[i] for i in rng.randint(0, 28, size=n))


@pytest.mark.skipif(not reftick.available(), reason="oracle/_ref/sf_ref_tick not built (no reference checkout)")
def test_a_game_logged_by_the_reference_replays_through_the_cpp_header(tmp_path):
    w = ref_cases.native(abi.MODE_SOLO, 3, STRONG1, maps="shipped")
    cmds = commands(400, 5)
    r = reftick.RefTick(w, STRONG1)
    r.logging(True)
    tb, serial = r.reset_native()
    for ch in cmds:
        r.step(ch)
    final_logged = r.dump()
    text = open(r.logclose()).read()
    r.close()
    sample = tmp_path / "logged.sf_sample"
    sample.write_text(text)
    exe = build(tmp_path, *emu_lib())
    copy = str(tmp_path / "copy.sf_sample")
    header, n, digest = run(exe, str(sample), abi.MODE_SOLO, 3, copy)
    assert header == "sample tb %d serial %d ind 0 team 1 name %s commands 400" % (tb, serial, header.split()[10])
    assert n == 400
    # the same file through the Python reader on the oracle: the state the reference itself ended the logged game in
    s = replay.read_sample(str(sample))
    o = Oracle(ref_cases.native(abi.MODE_SOLO, 3, s.profile_tokens, maps="shipped"))
    assert replay.replay(s, o) == 400
    assert reftick.first_difference(final_logged, reftick.arrays_of(o.dump(0))) is None
    assert digest == "%016x" % int(o.digest()[0])
    # the copy written by sf::write_sample: the bytes strikeforce_amd.replay writes, and the reference replays it
    twin = tmp_path / "twin.sf_sample"
    replay.write_sample(str(twin), s)
    assert open(copy, "rb").read() == twin.read_bytes()
    r2 = reftick.RefTick(w, config.HUMAN_TOKENS)  # (the record comes from the file)
    os.symlink(copy, os.path.join(r2.dir, "copy.sf_sample"))
    _tb2, serial2 = r2.reset_native(replay_path="copy.sf_sample")
    assert serial2 == serial
    for _ in cmds:
        r2.step("+")
    assert reftick.first_difference(r2.dump(), reftick.arrays_of(o.dump(0))) is None
    r2.close()


def _timer_sample(tmp_path):
    s = replay.Sample(1771155561, 1073741823, RICH, commands(900, 9), name="player")
    path = str(tmp_path / "ours.sf_sample")
    replay.write_sample(path, s)
    o = Oracle(ref_cases.native(abi.MODE_TIMER, 2, RICH, maps="shipped"))
    assert replay.replay(s, o) == 900
    return path, "%016x" % int(o.digest()[0])


def test_cpp_replay_on_the_emulator_equals_the_oracle(tmp_path):
    path, want = _timer_sample(tmp_path)
    _h, n, digest = run(build(tmp_path, *emu_lib()), path, abi.MODE_TIMER, 2)
    assert (n, digest) == (900, want)


@pytest.mark.gpu
def test_cpp_replay_on_the_device_equals_the_oracle(tmp_path):
    path, want = _timer_sample(tmp_path)
    _h, n, digest = run(build(tmp_path, os.path.join(ROOT, "strikeforce_amd"), "strikeforce_amd"), path, abi.MODE_TIMER, 2)
    assert (n, digest) == (900, want)
