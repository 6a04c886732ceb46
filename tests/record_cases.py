"""Shared by the sf_record_* tests: games played on the oracle through the split step, with everything the record kernels
read dumped per iteration (the scalar words, the humans' flag words, the command row) and the streams and game records the
reference's logger would have produced worked out from the oracle alone.  Test infrastructure only."""
import ctypes as C
import functools

import numpy as np

import online_cases as oc
from oracle_lib import Oracle
from strikeforce_amd import abi, config, replay

SC_WORDS, SC_STEPS, SC_EPISODES, SC_DONE, SC_OUTCOME, SC_ENDED, SC_TB_LO, SC_TB_HI, SC_SR_LO, SC_SR_HI = 24, 6, 7, 8, 9, 10, 11, 12, 13, 14
HF_ALIVE, HF_CTRL = 1 << 11, 1 << 15  # csrc/sf_types.hpp
QUIT, NOP = ord("_"), ord("+")


def writable(c):
    """what a sample can carry of a command byte (one token per command)"""
    return NOP if c <= 0x20 or c >= 0x7f else int(c)


class Played:
    """One batch of arenas played for T iterations.  tops / ends: int32 [T][A][SC_WORDS] in front of and behind iteration t;
    flags: uint32 [T][A][H] between its halves; results: int32 [T][A][n][8] behind it; digests: [T + 1][A] (0 = behind the
    reset); games: per arena the games in order, dicts of arena, episode, tb, serial, stream (bytes), iterations, end (a
    RECORD_* code, None for a game still open when the play stopped), outcome, first (the iteration it began in); facts:
    what the play met, per arena a set of names; substituted: how many bytes of the streams stand for one no sample carries."""


def _scal(hdr, ended):
    w = np.full(SC_WORDS, 0x5A5A5A5A, dtype=np.int64)  # (words the record kernels must not read)
    w[SC_STEPS], w[SC_EPISODES], w[SC_DONE], w[SC_OUTCOME], w[SC_ENDED] = hdr.steps, hdr.episodes, hdr.done, hdr.outcome, ended
    w[SC_TB_LO], w[SC_TB_HI], w[SC_SR_LO], w[SC_SR_HI] = hdr.tb & 0xFFFFFFFF, hdr.tb >> 32, hdr.serial & 0xFFFFFFFF, hdr.serial >> 32
    return w.astype(np.uint32).view(np.int32)


def play(w, tb, serial, cmds):
    """cmds: uint8 [T][A][n_agents].  Everything from the oracle."""
    cfg = w.cfg
    A, n, ind, H, ar = cfg.arenas, cfg.n_agents, cfg.ind, cfg.cap_humans, cfg.auto_reset
    T = len(cmds)
    o = Oracle(w)
    o.reset((C.c_uint64 * A)(*tb), (C.c_uint64 * A)(*serial))
    p = Played()
    p.w, p.cmds, p.tb, p.serial = w, np.ascontiguousarray(cmds, dtype=np.uint8), list(tb), list(serial)
    p.tops, p.ends = np.zeros((T, A, SC_WORDS), np.int32), np.zeros((T, A, SC_WORDS), np.int32)
    p.flags, p.results = np.zeros((T, A, H), np.uint32), np.zeros((T, A, n, 8), np.int32)
    p.digests = np.zeros((T + 1, A), np.uint64)
    p.digests[0] = o.digest()
    p.games, p.facts, p.substituted = [[] for _ in range(A)], [set() for _ in range(A)], 0
    open_ = [None] * A
    ended = np.zeros(A, dtype=np.int64)
    for t in range(T):
        top = [o.dump(a) for a in range(A)]
        for a in range(A):
            h = top[a].hdr
            p.tops[t, a] = _scal(h, ended[a])
            if h.done:
                continue
            if h.steps == 0:
                assert open_[a] is None
                open_[a] = dict(arena=a, episode=h.episodes, tb=h.tb, serial=h.serial, stream=bytearray(), iterations=0, end=None,
                                outcome=abi.RUNNING, first=t)
            g = open_[a]
            g["stream"].append(writable(cmds[t][a][ind]))
            g["iterations"] += 1
            if writable(cmds[t][a][ind]) != cmds[t][a][ind]:
                p.facts[a].add("substituted")
                p.substituted += 1
        o.step_begin()
        alive = o.agent_alive()
        for a in range(A):
            d = o.dump(a)
            for s in range(H):
                p.flags[t, a, s] = (HF_ALIVE if d.humans[s].alive else 0) | (HF_CTRL if s < n and alive[a][s] else 0) | 0x7 | (s << 16)
            if s_reused(d, alive[a], n, ind):
                p.facts[a].add("npc in a dead player's slot")
            if open_[a] is None:
                continue
            if top[a].humans[ind].alive and not d.humans[ind].alive:
                p.facts[a].add("ind died in the first half")
            for s in range(n):
                if s != ind and alive[a][s]:
                    open_[a]["stream"].append(writable(cmds[t][a][s]))
                    if writable(cmds[t][a][s]) != cmds[t][a][s]:
                        p.facts[a].add("substituted")
                        p.substituted += 1
        o.step_end(cmds[t])
        ended = o.done().astype(np.int64)
        p.results[t] = o.results()
        p.digests[t + 1] = o.digest()
        for a in range(A):
            h = o.dump(a).hdr
            p.ends[t, a] = _scal(h, ended[a] if ar else 0)
            if open_[a] is not None and (ended[a] if ar else h.done):
                g, open_[a] = open_[a], None
                g["end"], g["outcome"] = abi.RECORD_GAME_ENDED, int(p.results[t, a, 0, 7])
                assert g["outcome"] == (p.results[t, a, 0, 7] if ar else h.outcome) and g["outcome"] != abi.RUNNING
                p.games[a].append(g)
                p.facts[a].add("ended by check_end")
                if len(p.games[a]) >= 2:
                    p.facts[a].add("two games in one arena")
    for a in range(A):
        if open_[a] is not None:
            p.games[a].append(open_[a])
    o.close()
    return p


def s_reused(d, alive_row, n, ind):
    return any(s != ind and d.humans[s].alive and not alive_row[s] for s in range(n))


# ---- the 24-match batch and the two fixture matches (CPU test 1, GPU test 1) ---------------------------------------------
BATCH_ARENAS, BATCH_ITERS = 24, 60


def batch_commands(seed, iterations, quit_at=None, ind_quits_at=None):
    """the command rows online_cases.play_and_log draws for this seed"""
    rng = np.random.RandomState(seed)
    rows = np.zeros((iterations, 3), dtype=np.uint8)
    for it in range(iterations):
        rows[it] = [ord(abi.BENCH_COMMANDS[i]) for i in rng.randint(0, 28, size=3)]
        if quit_at is not None and it == quit_at[1]:
            rows[it, quit_at[0]] = QUIT
        if ind_quits_at is not None and it == ind_quits_at:
            rows[it, oc.BATCH["ind"]] = QUIT
    return rows


def batch_plan():
    """per arena (tb, serial, seed, quit_at, ind_quits_at): every fourth has a rival quitting, every sixth `ind`"""
    out = []
    for k in range(BATCH_ARENAS):
        quit_at = ((0 if k % 8 == 1 else 2), 7 + k) if k % 4 == 1 else None
        ind_quits = 9 + k if k % 6 == 2 else None
        out.append((1_700_000_000 + 17 * k, 123_456_789 + k, 2024 + k, quit_at, ind_quits))
    return out


def batch_workload(arenas=BATCH_ARENAS, auto_reset=0):
    proto = replay.Sample(1, 2, oc.RECORD, "", name="p1", ind=oc.BATCH["ind"], team=oc.BATCH["teams"][oc.BATCH["ind"]], players=3,
                          names=["p0", "p1", "p2"], records=[oc.RECORD] * 3, teams=oc.BATCH["teams"])
    w = oc.workload(proto, oc.BATCH, arenas=arenas)
    w.cfg.auto_reset = auto_reset
    return w


@functools.lru_cache(maxsize=None)
def batch_played():
    plan = batch_plan()
    cmds = np.stack([batch_commands(s, BATCH_ITERS, q, iq) for _, _, s, q, iq in plan], axis=1)
    return play(batch_workload(), [x[0] for x in plan], [x[1] for x in plan], cmds)


@functools.lru_cache(maxsize=None)
def fixture_played(name):
    """A fixture match the reference's own client logged, its rows fed as the commands (0 -> '+')."""
    s, f = oc.load(name)
    q = f["quit"]
    alive = [[g for g in range(3) if g != s.ind and not (q and g == q[0] and it > q[1])] for it in range(f["iterations"])]
    rows = np.array(oc.lines_per_iteration(s, alive), dtype=np.uint8)
    rows[rows == 0] = NOP
    return play(oc.workload(s, f), [s.tb], [s.serial], rows[:, None, :]), s, f


# ---- the reach of the inputs (tests/test_record_cases.py) ---------------------------------------------------------------
def squad_workload(arenas, auto_reset):
    cfg = config.make_config(arenas, 32, 32, H=10, Z=8, B=64, P=8, mode=abi.MODE_SQUAD, n_agents=3, auto_reset=auto_reset)
    keep = [(0, 3, 1)] + [(0, 1, i + 1) for i in range(1, 10)]
    return config.Workload("record-squad3", cfg, *config.synthetic_map(32, 32, wall_p=0.02, keep_clear=keep))


@functools.lru_cache(maxsize=None)
def squad_played():
    """Squad, ten humans in ten slots, the commanded humans standing still: agent 1 quits in iteration 24, the human NPC the
    loop top of frame 51 spawns takes its slot; agent 2 quits in iteration 27; `ind` quits in iteration 40 (arena 1 only)."""
    w = squad_workload(2, 0)
    rows = np.full((56, 2, 3), NOP, dtype=np.uint8)
    rows[24, :, 1] = QUIT
    rows[27, :, 2] = QUIT
    rows[40, 1, 0] = QUIT
    return play(w, [1_700_000_400, 1_700_000_401], [123_456_789] * 2, rows)


FIGHT_ARENAS, FIGHT_ITERS = 32, 100


@functools.lru_cache(maxsize=None)
def fight_played():
    """The BATCH shape under auto_reset, random play with shots four times as likely: games that check_end ends by itself,
    several per arena, and bytes no sample can carry in arenas 3 (`ind`) and 5 (a rival)."""
    w = batch_workload(FIGHT_ARENAS, auto_reset=1)
    rng = np.random.RandomState(77)
    table = np.frombuffer((abi.BENCH_COMMANDS + "xxxzzzxxx").encode(), dtype=np.uint8)
    rows = table[rng.randint(0, len(table), size=(FIGHT_ITERS, FIGHT_ARENAS, 3))].copy()
    for k, a in enumerate(range(0, FIGHT_ARENAS, 4)):  # `ind` gives up twice in every fourth arena: at least two games there
        rows[6 + k, a, 1] = QUIT
        rows[40 + k, a, 1] = QUIT
    rows[2, 3, 1], rows[4, 3, 1], rows[5, 3, 1], rows[7, 3, 1] = 0x00, 0x20, 0x7f, 0xff
    rows[3, 5, 0], rows[3, 5, 2], rows[9, 5, 2] = 0x80, 0x0a, 0x1f
    tb = [1_700_100_000 + 31 * a for a in range(FIGHT_ARENAS)]
    return play(w, tb, [987_654_321 + a for a in range(FIGHT_ARENAS)], rows)


SOLO_ARENAS, SOLO_ITERS = 16, 100


def solo_workload(arenas, auto_reset):
    tok = list(config.HUMAN_TOKENS)
    tok[0] = 100
    cfg = config.make_config(arenas, 12, 12, H=1, Z=16, B=16, P=4, auto_reset=auto_reset, player_tokens=tok)
    return config.Workload("record-solo", cfg, *config.synthetic_map(12, 12))


@functools.lru_cache(maxsize=None)
def solo_played():
    """A lone player of 100 Hp among sixteen zombies on 12 x 12 cells, under auto_reset: zombie_action kills `ind` in the
    first half of an iteration (its line of that iteration is in the stream), check_end ends the game at the next loop top,
    the arena goes on with the next game.  No line but the player's own (n_agents == 1)."""
    w = solo_workload(SOLO_ARENAS, 1)
    rows = config.bench_commands(SOLO_ARENAS, 1, SOLO_ITERS, seed0=5)[0]
    return play(w, [1_700_200_000 + a for a in range(SOLO_ARENAS)], [11 + a for a in range(SOLO_ARENAS)], rows)


CASES = {"squad": squad_played, "fight": fight_played, "solo": solo_played}
WORKLOADS = {"squad": squad_workload, "fight": batch_workload, "solo": solo_workload}  # (arenas, auto_reset) -> the case's world


# ---- what a recorder fed with a play must deliver -----------------------------------------------------------------------
def expected_games(p, flushed=True):
    """The game tuples (arena, episode, tb, serial, lines, iterations, end, outcome, stream) of a play recorded from its
    reset on with room for everything, arena ascending and game ascending; a game still open at the end is CUT by a flush
    and absent without one."""
    out = []
    for gs in p.games:
        for g in gs:
            if g["end"] is None and not flushed:
                continue
            out.append((g["arena"], g["episode"], g["tb"], g["serial"], len(g["stream"]), g["iterations"],
                        g["end"] if g["end"] is not None else abi.RECORD_CUT, g["outcome"], bytes(g["stream"])))
    return out


def delivered_games(games, data):
    """The same tuples from what a collect delivered (int32 [n][12], uint8 [m]); checks that the streams lie back to back."""
    from strikeforce_amd import env
    d = env.decode_games(games)
    out, at = [], 0
    for i in range(len(d["arena"])):
        off, n = int(d["offset"][i]), int(d["lines"][i])
        assert off == at, (i, off, at)
        at += n
        out.append((int(d["arena"][i]), int(d["episode"][i]), int(d["tb"][i]), int(d["serial"][i]), n, int(d["iterations"][i]),
                    int(d["end"][i]), int(d["outcome"][i]), bytes(np.asarray(data[off:off + n], dtype=np.uint8))))
    assert at == len(data)
    return out
