"""The workloads of the sf_signals_* tests and the driver that runs one on an engine and on the restatement side by side
(tests/test_signals_emu.py on the CPU runtime, tests/test_gpu_signals.py on the device, tests/test_signals_cases.py on the
restatement alone, to show that the cases reach every rule).  Test helper only.

A case is a world and a script: a list of operations
  ("reset", tb, sr)                   a whole sf_reset
  ("step", row)                       one sf_step, row uint8 [arenas][n_agents]
  ("many", rows)                      ONE k-step launch (sf_step_device), rows uint8 [k][arenas][n_agents]
  ("signals",)                        one sf_signals_step, compared with the restatement
  ("restart", kwargs, announce)       sf_reset_arenas(**kwargs); announce: d_selected goes into the next call's d_rebase
  ("save", slots) / ("load", slots, announce)    sf_snapshot_save / sf_snapshot_load, slots int [arenas]
  ("replay_step",)                    sf_replay_step
An engine has: cfg, reset, step, step_many, reset_arenas(**kwargs) -> selected uint8 [arenas][n_agents], save, load,
replay_load, replay_step, digest, dump, and new_signals() (see Checker)."""
import types

import numpy as np

from reset_sel_ref import ResetSelRef
from signals_ref import ReplayRef, SignalsRef
from snapshot_ref import SnapshotRef
from strikeforce_amd import abi, config, env

QUIT, NOP = ord("_"), ord("+")
SF_DIED, SF_WON, SF_TIME_LOST, SF_TIME_WON, SF_SAMPLE_END = 1, 2, 3, 4, 6


def weights():
    """Weights no product or sum of which is exact in float32, so that a fused or reordered sum shows."""
    return env.reward_weights(per_step=-0.01, kills=1.5, teams_kills=0.25, loot=0.001, damage=0.003, effect=-0.002, hp=0.01,
                              died=-3.3, outcome=[0.0, -1.1, 2.2, -0.7, 0.9, -0.5, 0.05, 0.0])


# ---- worlds ----------------------------------------------------------------------------------------------------------
def _solo(A, ar):
    cfg = config.make_config(A, 24, 24, H=1, Z=8, B=16, P=4, auto_reset=ar)
    return config.Workload("sig-solo", cfg, *config.synthetic_map(24, 24))


def _timer(A, ar):  # a Timer game of three steps: frame - 1 = 2 * steps reaches the limit of 6 frames
    cfg = config.make_config(A, 24, 24, H=4, Z=8, B=16, P=4, mode=abi.MODE_TIMER, auto_reset=ar, timer_frames=6)
    return config.Workload("sig-timer", cfg, *config.synthetic_map(24, 24))


def _battle3(A, ar):  # as many human slots as players: no NPC spawns, a dead player's slot stays empty
    cfg = config.make_config(A, 24, 24, H=3, Z=8, B=32, P=4, mode=abi.MODE_BATTLE, n_agents=3, teams=[1, 2, 3], auto_reset=ar)
    return config.Workload("sig-battle3", cfg, *config.synthetic_map(24, 24, wall_p=0.03))


def _squad3(A, ar):  # ten humans in ten slots: a commanded human that dies frees the lowest slot for the next spawned NPC
    cfg = config.make_config(A, 32, 32, H=10, Z=8, B=64, P=8, mode=abi.MODE_SQUAD, n_agents=3, auto_reset=ar)
    keep = [(0, 3, 1)] + [(0, 1, i + 1) for i in range(1, 10)]
    return config.Workload("sig-squad3", cfg, *config.synthetic_map(32, 32, wall_p=0.02, keep_clear=keep))


def _battle16(A, ar):
    cfg = config.make_config(A, 32, 32, H=16, Z=8, B=64, P=8, mode=abi.MODE_BATTLE, n_agents=16,
                             teams=[1 + (i % 3) for i in range(16)], auto_reset=ar)
    return config.Workload("sig-battle16", cfg, *config.synthetic_map(32, 32, wall_p=0.03))


def _rows(w, steps, seed):
    return config.bench_commands(w.cfg.arenas, w.cfg.n_agents, steps, seed0=seed)[0].reshape(steps, w.cfg.arenas, w.cfg.n_agents).copy()


def _seeds(w, base=1_700_000_000):
    tb, sr = w.seeds(base_tb=base)
    return list(tb), list(sr)


# ---- scripts ---------------------------------------------------------------------------------------------------------
def _timer_script(w):
    """Timer games of three steps: k = 1 calls that meet rule 3 every third step, a call without a step, a k = 8 launch in
    which every arena ends two games (rule 2), a whole reset on the same seeds (n < 0)."""
    rows, (tb, sr) = _rows(w, 20, 11), _seeds(w)
    s = [("reset", tb, sr), ("signals",)]
    for i in range(7):
        s += [("step", rows[i]), ("signals",)]
    s += [("signals",)]  # no step in between: all-zero deltas
    s += [("many", rows[7:15]), ("signals",)]
    s += [("step", rows[15]), ("signals",), ("reset", tb, sr), ("signals",), ("step", rows[16]), ("signals",)]
    return s


def _timer_still_script(w):
    """auto_reset 0: the game ends (rule 3), the arena stands still (IDLE) through steps and calls; a k = 8 launch."""
    rows, (tb, sr) = _rows(w, 16, 12), _seeds(w, 1_700_000_100)
    s = [("reset", tb, sr), ("signals",)]
    for i in range(5):
        s += [("step", rows[i]), ("signals",)]
    s += [("many", rows[5:13]), ("signals",)]
    return s


def _solo_script(w):
    """Solo, auto_reset as the world says: the reference's quit '_' in arena 1 (outcome DIED), then sf_reset_arenas on the
    finished games (announced), by mask on a new seed (not announced: the seed gives it away), on the SAME seed not
    announced (the step count gives it away) and on the same seed announced."""
    A = w.cfg.arenas
    rows, (tb, sr) = _rows(w, 24, 13), _seeds(w, 1_700_000_200)
    rows[3, 1, 0] = QUIT
    s = [("reset", tb, sr), ("signals",)]
    for i in range(6):
        s += [("step", rows[i]), ("signals",)]
    s += [("restart", dict(done_too=True), True), ("signals",), ("step", rows[6]), ("signals",)]
    m = np.zeros(A, dtype=np.uint8)
    m[0] = 1
    new_tb, new_sr = [1_800_000_000 + a for a in range(A)], [77 + a for a in range(A)]
    s += [("restart", dict(mask=m, tb=new_tb, serial=new_sr), False), ("signals",), ("step", rows[7]), ("signals",)]
    m2 = np.zeros(A, dtype=np.uint8)
    m2[2] = 1
    s += [("restart", dict(mask=m2, tb="same", serial="same"), False), ("signals",), ("step", rows[8]), ("signals",)]
    m3 = np.zeros(A, dtype=np.uint8)
    m3[A - 1] = 1
    s += [("restart", dict(mask=m3, tb="same", serial="same"), True), ("signals",)]
    for i in range(9, 12):
        s += [("step", rows[i]), ("signals",)]
    return s


def _battle3_script(w):
    """Battle of three teams, three slots.  Arena 0: agent 1 quits (its corpse's row, the slot stays empty), later agent 2
    quits and `ind` has WON.  Arena 1: both rivals quit in one step: WON.  Arena 2: `ind` quits: DIED.  Further arenas: an
    agent quits inside a k = 4 launch (a death several steps old)."""
    A = w.cfg.arenas
    rows, (tb, sr) = _rows(w, 24, 14), _seeds(w, 1_700_000_300)
    rows[:8] = NOP  # nobody fights before the scripted deaths
    rows[1, 0, 1] = QUIT
    rows[4, 0, 2] = QUIT
    rows[2, 1, 1] = rows[2, 1, 2] = QUIT
    rows[3, 2, 0] = QUIT
    for a in range(3, A):
        rows[6, a, 1 + a % 2] = QUIT
    s = [("reset", tb, sr), ("signals",)]
    for i in range(5):
        s += [("step", rows[i]), ("signals",)]
    s += [("many", rows[5:9]), ("signals",), ("signals",)]
    for i in range(9, 12):
        s += [("step", rows[i]), ("signals",)]
    s += [("many", rows[12:20]), ("signals",)]
    return s


def _squad3_script(w):
    """Squad, ten humans in ten slots: agent 1 quits in the step whose loop top spawns a human NPC (frame 51: step 25), so
    the NPC takes its slot inside the same call where the drawn cell is free; agent 2 quits a few steps later and is looked
    at only after the next spawn (several steps: UNRESOLVED)."""
    rows, (tb, sr) = _rows(w, 60, 15), _seeds(w, 1_700_000_400)
    rows[:, :, :] = NOP  # the commanded humans stand still: the script decides who dies
    rows[24, :, 1] = QUIT
    rows[27, :, 2] = QUIT
    s = [("reset", tb, sr), ("signals",), ("many", rows[0:8]), ("signals",), ("many", rows[8:16]), ("signals",),
         ("many", rows[16:24]), ("signals",), ("step", rows[24]), ("signals",), ("step", rows[25]), ("signals",),
         ("step", rows[26]), ("signals",)]
    s += [("many", rows[27:35]), ("many", rows[35:43]), ("many", rows[43:51]), ("signals",), ("step", rows[51]), ("signals",)]
    return s


def _battle16_script(w):
    """Sixteen agents: random play with k = 1 and k = 8 launches, a few scripted quits."""
    rows, (tb, sr) = _rows(w, 40, 16), _seeds(w, 1_700_000_500)
    rows[2, 0, 5] = rows[2, 0, 9] = rows[3, 1, 15] = rows[5, 2, 1] = QUIT
    s = [("reset", tb, sr), ("signals",)]
    for i in range(8):
        s += [("step", rows[i]), ("signals",)]
    s += [("many", rows[8:16]), ("signals",), ("many", rows[16:24]), ("signals",)]
    for i in range(24, 28):
        s += [("step", rows[i]), ("signals",)]
    return s


def _snapshot_script(w):
    """Forks and rewinds: arena 2 loads arena 0's slot (another seed), arena 1 its own earlier state (same seed, fewer
    steps), both not announced; arena 3 loads arena 0's slot announced."""
    A = w.cfg.arenas
    rows, (tb, sr) = _rows(w, 24, 17), _seeds(w, 1_700_000_600)
    rows[:12] = NOP
    rows[5, 0, 1] = QUIT
    s = [("reset", tb, sr), ("signals",)]
    for i in range(3):
        s += [("step", rows[i]), ("signals",)]
    s += [("save", [0, 1] + [-1] * (A - 2))]
    for i in range(3, 7):
        s += [("step", rows[i]), ("signals",)]
    s += [("load", [-1, 1, 0] + [-1] * (A - 3), False), ("signals",), ("step", rows[7]), ("signals",)]
    s += [("load", [-1, -1, -1, 0] + [-1] * (A - 4), True), ("signals",)]
    for i in range(8, 11):
        s += [("step", rows[i]), ("signals",)]
    return s


def _replay_script(w):
    """Replayed streams of 3, 5 and 0 lines: each arena stops with SF_SAMPLE_END where its stream runs out, then stands still."""
    tb, sr = _seeds(w, 1_700_000_700)
    s = [("reset", tb, sr), ("signals",)]
    for _ in range(7):
        s += [("replay_step",), ("signals",)]
    return s


def _replay_streams(w):
    r = config.bench_commands(w.cfg.arenas, 1, 5, seed0=18)[0].reshape(5, w.cfg.arenas)
    lens = [3, 5, 0] + [4] * (w.cfg.arenas - 3)
    return [bytes(r[:n, a].tolist()).replace(b"_", b"+") for a, n in enumerate(lens)]


#        name              world      arenas  auto_reset  kind        script
CASES = [("timer-k1-k8", _timer, 3, 1, "reset", _timer_script),
         ("timer-still", _timer, 5, 0, "reset", _timer_still_script),
         ("solo-restarts", _solo, 5, 1, "reset", _solo_script),
         ("solo-restarts-still", _solo, 3, 0, "reset", _solo_script),
         ("battle3", _battle3, 5, 1, "reset", _battle3_script),
         ("battle3-still", _battle3, 3, 0, "reset", _battle3_script),
         ("squad3-npc", _squad3, 5, 0, "reset", _squad3_script),
         ("battle16", _battle16, 5, 1, "reset", _battle16_script),
         ("battle16-still", _battle16, 3, 0, "reset", _battle16_script),
         ("snapshot", _battle3, 5, 1, "snapshot", _snapshot_script),
         ("replay-end", _solo, 3, 0, "replay", _replay_script)]
NAMES = [c[0] for c in CASES]


def case(name):
    _, world, A, ar, kind, script = CASES[NAMES.index(name)]
    w = world(A, ar)
    return types.SimpleNamespace(name=name, w=w, kind=kind, script=script(w),
                                 streams=_replay_streams(w) if kind == "replay" else None)


def make_ref(c):
    """The restatement's source for a case, reset on the script's first operation's seeds."""
    op = c.script[0]
    assert op[0] == "reset"
    if c.kind == "snapshot":
        return SnapshotRef(c.w, op[1], op[2], 3)
    if c.kind == "replay":
        return ReplayRef(c.w, op[1], op[2], c.streams)
    return ResetSelRef(c.w, op[1], op[2])


def _restart_seeds(src, kw):
    """tb / serial of a restart: "same" = every arena's running seed."""
    kw = dict(kw)
    if isinstance(kw.get("tb"), str):
        hdrs = [src.dump(a).hdr for a in range(src.cfg.arenas)]
        kw["tb"], kw["serial"] = [int(h.tb) for h in hdrs], [int(h.serial) for h in hdrs]
    return kw


def run(c, engine=None, check=None):
    """Plays the case on the restatement and, where given, on the engine; check(op_index, got, want, engine, sref) after
    every signals call, got / want = (vitals, delta, reward, status).  Returns the SignalsRef (its .reach)."""
    A, n = c.w.cfg.arenas, c.w.cfg.n_agents
    src = make_ref(c)
    sref = SignalsRef(src)
    wts = weights()
    pending = None  # the rebase mask the next call announces
    if engine is not None and c.kind == "replay":
        engine.replay_load(c.streams)
    try:
        for i, op in enumerate(c.script):
            if op[0] == "reset":
                if i:  # (make_ref has played the first one)
                    src.reset(op[1], op[2])
                if engine is not None:
                    engine.reset(op[1], op[2])
            elif op[0] == "step":
                src.step(op[1])
                if engine is not None:
                    engine.step(op[1])
            elif op[0] == "many":
                for row in op[1]:
                    src.step(row)
                if engine is not None:
                    engine.step_many(op[1])
            elif op[0] == "restart":
                kw = _restart_seeds(src, op[1])
                sel = src.reset_arenas(**kw)
                if engine is not None:
                    got = engine.reset_arenas(**kw)
                    assert (got == np.repeat(sel.astype(np.uint8), n).reshape(A, n)).all(), (c.name, i)
                if op[2]:
                    m = np.repeat(sel.astype(np.uint8), n).reshape(A, n)
                    pending = m if pending is None else pending | m
            elif op[0] == "save":
                src.save(op[1])
                if engine is not None:
                    engine.save(op[1])
            elif op[0] == "load":
                src.load(op[1])
                if engine is not None:
                    engine.load(op[1])
                if op[2]:
                    m = np.repeat((np.asarray(op[1]) >= 0).astype(np.uint8), n).reshape(A, n)
                    pending = m if pending is None else pending | m
            elif op[0] == "replay_step":
                src.replay_step()
                if engine is not None:
                    engine.replay_step()
            elif op[0] == "signals":
                want = sref.step(pending, wts) + (sref.status(),)
                if engine is not None:
                    check(i, engine, pending, wts, want, sref)
                pending = None
            else:
                raise ValueError(op[0])
    finally:
        src.close()
    return sref


def compare(what, got, want):
    """vitals, delta, reward bits and status of one call, engine against restatement."""
    gv, gd, gr, gs = got
    wv, wd, wr, ws = want
    assert np.array_equal(gd, wd), (what, "delta", np.argwhere(gd != wd)[:4].tolist(), gd[gd != wd][:4], wd[gd != wd][:4])
    assert np.array_equal(gv, wv), (what, "vitals", np.argwhere(gv != wv)[:4].tolist(), gv[gv != wv][:4], wv[gv != wv][:4])
    gb, wb = np.asarray(gr, dtype=np.float32).view(np.uint32), np.asarray(wr, dtype=np.float32).view(np.uint32)
    assert np.array_equal(gb.reshape(wb.shape), wb), (what, "reward bits", gr, wr)
    assert tuple(gs) == tuple(ws), (what, "status", gs, ws)


# ---- what the engines' tests share: buffers with sentinels and guards, and the checks after every call ---------------
SENTINEL = np.int32(-0x5A5A5A5B)  # every word of an output buffer before the call, and the guard word behind it
SENTINEL_F = np.float32(-12345.678)


def out_buffers(A, n, outs):
    """Host images of the output buffers a call gets: sentinel-filled, one guard word behind the last record; None for an
    output that is left out (NULL)."""
    v = np.full(A * n * abi.VITALS_WORDS + 1, SENTINEL, dtype=np.int32) if "v" in outs else None
    d = np.full(A * n * abi.DELTA_WORDS + 1, SENTINEL, dtype=np.int32) if "d" in outs else None
    r = np.full(A * n + 1, SENTINEL_F, dtype=np.float32) if "r" in outs else None
    return v, d, r


def take_buffers(A, n, v, d, r, what):
    """The records of the buffers after the call; the guard words must stand."""
    for b, s in ((v, SENTINEL), (d, SENTINEL), (r, SENTINEL_F)):
        assert b is None or b[-1] == s, (what, "guard word overwritten")
    return (None if v is None else v[:-1].reshape(A, n, abi.VITALS_WORDS), None if d is None else d[:-1].reshape(A, n, abi.DELTA_WORDS),
            None if r is None else r[:-1].reshape(A, n))


def rebase_bytes(mask, call):
    """d_rebase of a call: None (NULL) or an all-zero mask in turn where nothing is announced; where something is, the set
    bytes carry 0x80, 0xFF or 2 — the rule is `!= 0`, not `== 1`."""
    if mask is None:
        return None if call % 2 == 0 else "zeros"
    m = np.asarray(mask, dtype=np.uint8).copy()
    m[m != 0] = (0x80, 0xFF, 2)[call % 3]
    return m


class Checker:
    """check() of run(): every call goes to five signals objects of the engine, each with a baseline of its own — all
    outputs; vitals, delta, reward alone (the other outputs NULL); and one that is called twice.  engine.new_signals()
    returns an object with step(rebase uint8 [A][n] / None / "zeros", weights, outs) -> (vitals, delta, reward) (None where
    left out; sentinels and guards checked), status() and close()."""

    def __init__(self, engine, name):
        self.e, self.name, self.calls = engine, name, 0
        self.objs = {k: engine.new_signals() for k in ("vdr", "v", "d", "r", "twice")}

    def close(self):
        for o in self.objs.values():
            o.close()

    def __call__(self, i, engine, pending, wts, want, sref):
        what = "%s, operation %d" % (self.name, i)
        A, n = engine.cfg.arenas, engine.cfg.n_agents
        rb = rebase_bytes(pending, self.calls)
        self.calls += 1
        before = engine.digest()
        o = self.objs["vdr"]
        got = o.step(rb, wts, "vdr")
        compare(what, got + (o.status(),), want)
        for k, j in (("v", 0), ("d", 1), ("r", 2)):  # each output with the two others NULL
            alone = self.objs[k].step(rb, wts, k)
            assert [x is None for x in alone] == [x != j for x in range(3)], what
            compare(what + ", only " + k, tuple(alone[x] if x == j else want[x] for x in range(3)) + (want[3],), want)
        t = self.objs["twice"]
        compare(what + ", first of two", t.step(rb, wts, "vdr") + (t.status(),), want)
        v2, d2, r2 = t.step(None, wts, "vdr")  # no step in between: nothing changed
        assert not d2[:, :, 1:].any(), (what, "second call", d2)
        assert not (d2[:, :, 0] & ~(abi.SIG_PRESENT | abi.SIG_IDLE)).any(), (what, "second call", d2[:, :, 0])
        assert np.array_equal(v2[:, :, 1:], want[0][:, :, 1:]) and t.status() == (0, 0), what
        assert (engine.digest() == before).all(), (what, "a signals call changed an arena")
        vit = got[0]
        for a in range(A):  # the vitals against sf_dump_arena's own fields
            dump = engine.dump(a)
            h = dump.hdr
            assert [int(x) for x in vit[a, 0, 12:16]] == [h.kills, h.teams_kills, h.loot, h.steps], (what, a)
            for g in range(n):
                hu = dump.humans[g]
                if vit[a, g, 0] & abi.SIG_PRESENT:
                    assert hu.alive and [int(x) for x in vit[a, g, 1:12]] == [hu.hp, hu.stamina, hu.mindamage, hu.kills, hu.damage,
                                                                               hu.effect, hu.f, hu.r, hu.c, hu.way, hu.team], (what, a, g)
                else:
                    assert not vit[a, g, 1:12].any(), (what, a, g)
