"""The lane functions of csrc/sf_record.hpp — the text k_record, k_record_plan and k_record_copy compile — on the CPU, in the
stand-alone program tests/record/record_main.cpp, built once plain and once with -fsanitize=address,undefined.  Nothing
sanitized is loaded into Python.

The games are played on the oracle through the split step (tests/record_cases.py), which dumps what the kernels read per
iteration: the scalar words, the humans' flag words, the command row.  Expected bytes: the oracle-side logger
online_cases.play_and_log for the 24-match batch, the reference client's own files for the two fixture matches
(tests/golden/online_*.sf_sample), and record_cases.play's own bookkeeping for the cases; the collection is checked on
synthetic layouts whose streams are known by construction."""
import os
import subprocess

import numpy as np
import pytest

import online_cases as oc
import record_cases as rc
from strikeforce_amd import abi, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "record", "record_main.cpp")
BASE = ["-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
ALL_B, ALL_G = 1 << 20, 1 << 12  # limits that cut nothing


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("record_main")
    out = {}
    for name, flags in BUILDS.items():
        out[name] = str(d / ("record_main_" + name))
        subprocess.check_call([os.environ.get("CXX", "g++")] + BASE + flags + ["-o", out[name], SRC])
    return out


class Trace:
    """the event list record_main takes"""

    def __init__(self, p, bpa, G):
        cfg = p.w.cfg
        self.p, self.n = p, cfg.n_agents
        self.words = [np.array([cfg.arenas, cfg.cap_humans, cfg.n_agents, cfg.ind, cfg.auto_reset, G, bpa], dtype=np.int32)]
        self.collects = 0

    def _add(self, *arrs):
        self.words += [np.ascontiguousarray(a).astype(np.int64).astype(np.uint32).view(np.int32).reshape(-1) if not isinstance(a, int)
                       else np.array([a], dtype=np.int32) for a in arrs]

    def iteration(self, t, top=None):
        p = self.p
        c = p.cmds[t]
        self._add(0, p.tops[t] if top is None else top, c)
        if self.n > 1:
            self._add(1, p.flags[t].astype(np.int64), c)
        self._add(2, p.ends[t], p.results[t])

    def flush(self):
        self._add(3)

    def collect(self, max_bytes=ALL_B, max_games=ALL_G):
        self._add(4, int(max_bytes), int(max_games))
        self.collects += 1

    def run(self, programs, tmp_path):
        """[(counts, games int32 [n][12], bytes uint8 [m])] per collect — the same from both builds"""
        path = str(tmp_path / "trace.bin")
        np.concatenate(self.words).tofile(path)
        results = []
        for build, exe in programs.items():
            got = str(tmp_path / ("out_" + build + ".bin"))
            r = subprocess.run([exe, path, got], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (build, r.stdout[-2000:], r.stderr[-4000:])
            assert r.stdout.split()[:2] == ["record_main", "ok"] and int(r.stdout.split()[3]) == self.collects, r.stdout
            raw, at, out = np.fromfile(got, dtype=np.uint8), 0, []
            for _ in range(self.collects):
                counts = raw[at:at + 48].view(np.int64).copy()
                at += 48
                games = raw[at:at + 48 * int(counts[0])].view(np.int32).reshape(-1, 12).copy()
                at += 48 * int(counts[0])
                data = raw[at:at + int(counts[1])].copy()
                at += (int(counts[1]) + 7) // 8 * 8
                out.append((counts.tolist(), games, data))
            assert at == len(raw)
            results.append(out)
        a, b = results
        assert len(a) == len(b) and all(x[0] == y[0] and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]) for x, y in zip(a, b))
        return a


def record_all(p, programs, tmp_path, bpa=None, G=8, every=None):
    """the whole play through the recorder: a collect every `every` iterations, then flush and a last collect"""
    T = len(p.cmds)
    tr = Trace(p, bpa if bpa is not None else 3 * T + 8, G)
    for t in range(T):
        tr.iteration(t)
        if every and t % every == every - 1:
            tr.collect()
    tr.flush()
    tr.collect()
    return tr.run(programs, tmp_path)


def by_arena(collects):
    out = {}
    for _, games, data in collects:
        for g in rc.delivered_games(games, data):
            out.setdefault(g[0], []).append(g)
    return out


def test_the_24_match_batch_gives_the_bytes_of_the_oracle_side_logger(programs, tmp_path):
    p = rc.batch_played()
    (counts, games, data), = record_all(p, programs, tmp_path)
    got = rc.delivered_games(games, data)
    assert got == rc.expected_games(p) and len(got) == rc.BATCH_ARENAS
    assert counts == [len(got), sum(g[4] for g in got), 0, 0, 0, 0]
    kinds = set()
    for g, (tb, serial, seed, quit_at, ind_quits) in zip(got, rc.batch_plan()):
        s = oc.play_and_log(tb, serial, g[5], seed, quit_at=quit_at, ind_quits_at=ind_quits)
        assert g[8] == s.commands.encode() and (g[2], g[3]) == (tb, serial)
        assert g[6] == (abi.RECORD_GAME_ENDED if ind_quits is not None else abi.RECORD_CUT)
        assert g[5] == (ind_quits + 1 if ind_quits is not None else rc.BATCH_ITERS)
        assert (len(g[8]) < 3 * g[5]) == (quit_at is not None and quit_at[1] + 1 < g[5])
        kinds.add((quit_at is not None, ind_quits is not None))
    assert kinds == {(False, False), (True, False), (False, True)}


@pytest.mark.parametrize("name", oc.NAMES)
def test_a_fixture_match_gives_the_reference_clients_own_file(programs, tmp_path, name):
    p, s, f = rc.fixture_played(name)
    assert ["%016x" % int(x) for x in p.digests[:, 0]] == f["digests"]  # the play IS the logged match
    (counts, games, data), = record_all(p, programs, tmp_path)
    (g,) = rc.delivered_games(games, data)
    assert g[8] == s.commands.encode()  # byte for byte the command lines the reference's client wrote
    assert g[:8] == (0, 0, s.tb, s.serial, len(s.commands), 120, abi.RECORD_CUT, abi.RUNNING)
    (made,) = replay.samples_from_recording(games, data, s)
    out = str(tmp_path / "again.sf_sample")
    replay.write_sample(out, made, layout="logged")
    assert open(out, "rb").read() == open(oc.path_of(name), "rb").read()
    assert made.recorded == dict(arena=0, episode=0, iterations=120, end=abi.RECORD_CUT, outcome=abi.RUNNING)


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_the_cases_give_the_streams_the_oracle_says(programs, tmp_path, name):
    p = rc.CASES[name]()
    (counts, games, data), = record_all(p, programs, tmp_path)
    got, want = rc.delivered_games(games, data), rc.expected_games(p)
    assert got == want
    assert counts[4] == 0 and counts[5] == p.substituted and (counts[5] > 0) == any("substituted" in f for f in p.facts)
    for g in got:  # seeds under auto_reset: tb + episode * reseed stride (the arena count)
        assert (g[2], g[3]) == (p.tb[g[0]] + g[1] * p.w.cfg.arenas * p.w.cfg.auto_reset, p.serial[g[0]])


@pytest.mark.parametrize("name", ["fight", "solo"])
def test_a_collect_every_7_iterations_gives_the_same_games(programs, tmp_path, name):
    p = rc.CASES[name]()
    often = record_all(p, programs, tmp_path, every=7)
    assert sum(1 for c in often[:-1] if c[0][0]) >= 2  # (games were delivered along the way)
    assert all(c[0][2:5] == [0, 0, 0] for c in often)
    want = {}
    for g in rc.expected_games(p):
        want.setdefault(g[0], []).append(g)
    assert by_arena(often) == want
    # ... and with a region that only holds everything because collects free it
    longest = max(g[4] for g in rc.expected_games(p))
    tight = record_all(p, programs, tmp_path, bpa=longest + 7 * p.w.cfg.n_agents + p.w.cfg.n_agents, every=7)
    assert by_arena(tight) == want


# ---- collection on layouts known by construction -------------------------------------------------------------------------
def synthetic(lengths, n=2, T=None, deaths=()):
    """A Played built by hand under auto_reset: arena a plays games of lengths[a][0], lengths[a][1], ... iterations one after
    the other (each ended by check_end with outcome 1 + game % 5); agent 1 is alive except in the (arena, iteration) pairs
    of `deaths`.  Commands are distinct printable bytes, so every stream is known."""
    A = len(lengths)
    T = T if T is not None else max(sum(x) for x in lengths)
    p = rc.Played()

    class W:
        pass
    p.w = W()
    p.w.cfg = type("Cfg", (), dict(arenas=A, cap_humans=4, n_agents=n, ind=0, auto_reset=1))()
    p.cmds = (0x21 + (np.arange(T * A * n).reshape(T, A, n) * 7) % 0x5e).astype(np.uint8)
    p.tops, p.ends = np.zeros((T, A, rc.SC_WORDS), np.int32), np.zeros((T, A, rc.SC_WORDS), np.int32)
    p.flags, p.results = np.zeros((T, A, 4), np.uint32), np.zeros((T, A, n, 8), np.int32)
    p.games, p.tb, p.serial = [[] for _ in range(A)], [5_000_000_000 + a for a in range(A)], [7 + a for a in range(A)]
    for a in range(A):
        ep, i, g = 0, 0, None
        for t in range(T):
            hdr = lambda steps, e: type("H", (), dict(steps=steps, episodes=e, done=0, outcome=0, tb=p.tb[a] + e * A, serial=p.serial[a]))()
            p.tops[t, a] = rc._scal(hdr(i, ep), 0)
            if i == 0:
                g = dict(arena=a, episode=ep, tb=p.tb[a] + ep * A, serial=p.serial[a], stream=bytearray(), iterations=0, end=None,
                         outcome=0, first=t)
            g["stream"].append(p.cmds[t, a, 0])
            g["iterations"] += 1
            alive = (a, t) not in deaths
            p.flags[t, a] = [rc.HF_ALIVE | rc.HF_CTRL, (rc.HF_ALIVE | rc.HF_CTRL) if alive else rc.HF_ALIVE, rc.HF_ALIVE | rc.HF_CTRL, 0]
            if n > 1 and alive:
                g["stream"].append(p.cmds[t, a, 1])
            i += 1
            over = ep < len(lengths[a]) and i == lengths[a][ep]
            if over:
                g["end"], g["outcome"] = abi.RECORD_GAME_ENDED, 1 + ep % 5
                p.results[t, a, 0, 7] = g["outcome"]
                p.games[a].append(g)
                ep, i, g = ep + 1, 0, None
            p.ends[t, a] = rc._scal(hdr(i, ep), 1 if over else 0)
        if g is not None:
            p.games[a].append(g)
    return p


FIVE = [[3, 2], [70], [1, 40]]  # five closed games over three arenas; then every arena has an open one


def test_limits_cut_the_delivery_at_every_position_of_a_five_game_layout(programs, tmp_path):
    p = synthetic(FIVE, T=75, deaths={(1, 5), (2, 3)})
    closed = [g for g in rc.expected_games(p, flushed=False)]
    assert [g[4] for g in closed] == [6, 4, 139, 2, 79] and len(rc.expected_games(p)) == 8
    cum = np.cumsum([g[4] for g in closed]).tolist()
    limits = [(ALL_B, k) for k in range(1, 6)]
    for c in cum:
        limits += [(c - 1, ALL_G), (c, ALL_G), (c + 1, ALL_G)]
    limits += [(cum[1], 1), (cum[0], 3), (1, ALL_G)]
    tr = Trace(p, 160, 4)
    for t in range(75):
        tr.iteration(t)
    # (every trace is the same play: each run applies one pair of limits, then takes the rest, then the open games)
    for mb, mg in limits:
        one = Trace(p, 160, 4)
        one.words = list(tr.words)
        one.collect(mb, mg), one.collect(), one.flush(), one.collect()
        first, rest, opened = one.run(programs, tmp_path)
        k = max([0] + [j + 1 for j in range(5) if cum[j] <= mb and j + 1 <= mg])
        assert first[0][:4] == [k, cum[k - 1] if k else 0, 5 - k, cum[4] - (cum[k - 1] if k else 0)], (mb, mg, first[0])
        assert rc.delivered_games(first[1], first[2]) == closed[:k], (mb, mg)
        assert rc.delivered_games(rest[1], rest[2]) == closed[k:] and rest[0][:4] == [5 - k, cum[4] - (cum[k - 1] if k else 0), 0, 0]
        # the open games went on uninterrupted through both collects (their bytes moved to the front of the region)
        assert rc.delivered_games(opened[1], opened[2]) == [g for g in rc.expected_games(p) if g[6] == abi.RECORD_CUT]


def test_an_empty_recorder_an_open_game_and_a_full_index(programs, tmp_path):
    p = synthetic([[4, 3, 2], [20]], T=14)
    tr = Trace(p, 64, 2)
    tr.collect()  # nothing recorded yet
    for t in range(3):
        tr.iteration(t)
    tr.collect()  # only open games
    for t in range(3, 14):
        tr.iteration(t)
    tr.collect()
    tr.flush(), tr.collect()
    empty, opened, full, rest = tr.run(programs, tmp_path)
    assert empty[0] == [0] * 6 and opened[0] == [0] * 6 and len(empty[1]) == 0
    want = rc.expected_games(p)
    # arena 0's index of two is full when its third game would open (iteration 7): lost, and again for the fourth (9)
    assert full[0] == [2, 8 + 6, 0, 0, 2, 0] and rc.delivered_games(full[1], full[2]) == want[:2]
    # the collect made room; the fourth game was already running then (steps != 0): only arena 1's open game is left
    assert rc.delivered_games(rest[1], rest[2]) == [want[-1]] and rest[0] == [1, 28, 0, 0, 0, 0]


def test_overflow_closes_the_game_with_whole_iterations_only(programs, tmp_path):
    p = synthetic([[9], [9]], T=9, deaths={(1, t) for t in range(9)})
    tr = Trace(p, 7, 4)  # arena 0 takes two bytes per iteration: three iterations fit 7 bytes, the fourth needs 2 free of 1
    for t in range(9):
        tr.iteration(t)
    tr.collect()
    (counts, games, data), = tr.run(programs, tmp_path)
    got = rc.delivered_games(games, data)
    want = rc.expected_games(p)
    assert got[0][:8] == want[0][:4] + (6, 3, abi.RECORD_OVERFLOW, abi.RUNNING) and got[0][8] == want[0][8][:6]
    # arena 1 (one byte per iteration) fits six iterations: the seventh would leave fewer than n_agents bytes
    assert got[1][:8] == want[1][:4] + (6, 6, abi.RECORD_OVERFLOW, abi.RUNNING) and got[1][8] == want[1][8][:6]
    assert counts == [2, 12, 0, 0, 0, 0]


def test_broken_and_cut(programs, tmp_path):
    p = synthetic([[30], [30], [30]], T=12)
    tr = Trace(p, 64, 4)
    for t in range(4):
        tr.iteration(t)
    top = p.tops[6].copy()  # arena 0 was stepped twice through another entry point: steps 6 where the game has 4
    top[1, rc.SC_STEPS], top[2, rc.SC_STEPS] = 4, 0  # arena 2 was restarted (steps 0, the same episode count): cut, and a new game
    tr.iteration(4, top=top)
    tr.flush(), tr.collect()
    (counts, games, data), = tr.run(programs, tmp_path)
    got = rc.delivered_games(games, data)
    assert [(g[0], g[4], g[5], g[6]) for g in got] == [(0, 8, 4, abi.RECORD_BROKEN), (1, 10, 5, abi.RECORD_CUT),
                                                       (2, 8, 4, abi.RECORD_CUT), (2, 2, 1, abi.RECORD_CUT)]
