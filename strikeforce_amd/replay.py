"""`.sf_sample` trajectories — the reference's own record/replay format.

Written by gameplay::load_data / human_action when logging is on (gameplay.hpp:1784-1794,1910-1914,966-967) and read
back in replay mode (gameplay.hpp:1771-1782,968-969); the player blob is Human::log_file / scan_file
(Character.hpp:619-648,570-617).  Offline Solo / Timer files look like

    <tb> <serial>
    1 <ind> <team>
    <name>                       \\
    <def_Hp> ... 31 more integers, one per line   (the character record)
    <one command char per loop iteration, one per line>

Online files (a Battle match, `players` > 1) exist in two layouts, because the reference's writer and reader disagree:

    "logged"  what the reference WRITES (gameplay.hpp:1836-1845): `tb serial` / `players ind team(ind)` / the blob of
              `ind` / the blob of every other player in slot order / the command lines.  No team of the other players.
    "replay"  what the reference READS (gameplay.hpp:1762-1778,1796-1806): three leading tokens (ip, port, password:
              read and thrown away), `tb serial`, `players ind team`, the blob of `ind`, then for every other slot its
              blob FOLLOWED BY ITS TEAM, then the command lines.

So the reference cannot replay its own online log as written; read here as "logged" with the teams supplied and written
as "replay", it can.  The command lines of a match are, per loop iteration, the command of `ind` and then one for every
other player that is alive and remote when human_action runs, slots ascending (gameplay.hpp:966-967,979-986): how many
lines an iteration has depends on the game.

This module reads and writes the format and replays a sample through any backend with the reset/step surface
(ArenaBatch on the GPU; the oracle and the emulator in tests); matches need the split step (step_begin / agent_alive /
step_end), or ArenaBatch's device form (replay_batch: the lines are fetched on the device, env.ArenaBatch.replay_step).
"""
import collections
import ctypes as C

import numpy as np

from . import abi, config

LAYOUTS = ("auto", "logged", "replay")


class Sample:
    """One logged game.  Offline: the player's record and one command per iteration.  A match (`players` > 1)
    additionally has per player `names[i]`, `records[i]` (32 integers) and `teams[i]` (None where the file does not say:
    layout "logged" only carries the team of `ind`), and optionally the three strings layout "replay" starts with.
    `commands` is the flat stream of command chars in file order either way; name / profile_tokens / team are those of
    `ind`."""

    def __init__(self, tb, serial, profile_tokens, commands, name="player", ind=0, team=1, players=1, names=None,
                 records=None, teams=None, ip="0.0.0.0", port="0", password="-"):
        if len(profile_tokens) != 32:
            raise ValueError("a character record has 32 integers after the name")
        self.tb, self.serial = int(tb), int(serial)
        self.profile_tokens = [int(x) for x in profile_tokens]
        self.commands = str(commands)
        self.name, self.ind, self.team = name, int(ind), int(team)
        self.players = int(players)
        if not 0 <= self.ind < self.players:
            raise ValueError("ind must be one of the %d players" % self.players)
        self.names = list(names) if names is not None else [name] * self.players
        self.records = [[int(x) for x in r] for r in records] if records is not None else [list(self.profile_tokens)] * self.players
        self.teams = list(teams) if teams is not None else [None] * self.players
        if not (len(self.names) == len(self.records) == len(self.teams) == self.players):
            raise ValueError("names, records and teams need one entry per player")
        if any(len(r) != 32 for r in self.records):
            raise ValueError("a character record has 32 integers after the name")
        self.names[self.ind], self.records[self.ind], self.teams[self.ind] = name, list(self.profile_tokens), self.team
        self.ip, self.port, self.password = str(ip), str(port), str(password)


def _blob(f, name, tokens):
    f.write(name + "\n")
    for t in tokens:
        f.write("%d\n" % t)


def write_sample(path, sample, layout="logged"):
    """Same byte layout as the reference's logger: header, Human::log_file blob(s), then `command << '\\n'` per line.
    layout "logged" (the default; "auto" means the same here): what the reference writes; "replay": what the
    reference's replay mode reads (module docstring) — every player's team must be known for it.  An offline sample
    (players == 1) is the same bytes whatever `layout` says."""
    if layout not in LAYOUTS:
        raise ValueError("layout must be one of %s" % (LAYOUTS,))
    match = sample.players > 1
    as_replay = match and layout == "replay"
    if as_replay and any(t is None for t in sample.teams):
        raise ValueError("layout 'replay' carries every player's team: this sample lacks some (read it with teams=)")
    with open(path, "w") as f:
        if as_replay:
            f.write("%s\n%s\n%s\n" % (sample.ip, sample.port, sample.password))
        f.write("%d %d\n" % (sample.tb, sample.serial))
        f.write("%d %d %d\n" % (sample.players, sample.ind, sample.team))
        _blob(f, sample.name, sample.profile_tokens)
        for i in range(sample.players):
            if i == sample.ind:
                continue
            _blob(f, sample.names[i], sample.records[i])
            if as_replay:
                f.write("%d\n" % sample.teams[i])
        for c in sample.commands:
            f.write(c + "\n")


def _is_int(t):
    try:
        int(t)
        return True
    except ValueError:
        return False


def _parse(tok, layout, teams):
    """The tokens of one file in one explicit layout -> Sample; ValueError where they do not fit it."""
    lead = None
    if layout == "replay" and not (len(tok) > 2 and _is_int(tok[0]) and _is_int(tok[1]) and tok[2] == "1"):
        lead, tok = tok[:3], tok[3:]  # (an offline file has no such tokens: gameplay.hpp:1762 `if(online)`)
    if len(tok) < 5 + 33 or not all(_is_int(t) for t in tok[:5]):
        raise ValueError("header: expected `tb serial` and `players ind team`")
    tb, serial, players, ind, team = (int(t) for t in tok[:5])
    if players < 1 or players > abi.MAX_AGENTS or not 0 <= ind < players:
        raise ValueError("header: players must be 1..%d and ind one of them, got players=%d ind=%d" % (abi.MAX_AGENTS, players, ind))
    pos = 5
    order = [ind] + [i for i in range(players) if i != ind]
    names, records, tms = [None] * players, [None] * players, [None] * players
    tms[ind] = team
    for i in order:
        rec = tok[pos + 1:pos + 33]
        if len(rec) != 32 or not all(_is_int(t) for t in rec):
            raise ValueError("character record of player %d: fewer than 32 integers" % i)
        names[i], records[i] = tok[pos], [int(t) for t in rec]
        pos += 33
        if layout == "replay" and i != ind:
            if pos >= len(tok) or not _is_int(tok[pos]):
                raise ValueError("layout 'replay': the team of player %d is missing behind its record" % i)
            tms[i] = int(tok[pos])
            pos += 1
    if players > 1 and layout == "logged":
        if teams is None:
            raise ValueError("a logged online sample (players=%d) holds only the team of `ind`: pass teams=[...], one per "
                             "player (layout 'logged', gameplay.hpp:1836-1845)" % players)
        if len(teams) != players or int(teams[ind]) != team:
            raise ValueError("teams= needs one entry per player, and teams[ind] must be the file's own (%d)" % team)
        tms = [int(t) for t in teams]
    # `replay_file >> command[i]` reads one char at a time: a token like "ab" is two commands
    cmds = "".join(tok[pos:])
    kw = dict(zip(("ip", "port", "password"), lead)) if lead else {}
    return Sample(tb, serial, records[ind], cmds, name=names[ind], ind=ind, team=team, players=players, names=names,
                  records=records, teams=tms, **kw)


def read_sample(path, layout="auto", teams=None):
    """Parses like the reference does: whitespace-separated tokens (operator>>), one non-blank char per command.
    layout "logged" / "replay": exactly that layout (module docstring), never a guess.  "auto": the file is taken as
    "logged" if it parses as such — five integers, then a name and 32 integers per player — and otherwise as "replay",
    i.e. the same behind three leading tokens (an IP address is no integer, so a "replay" file never parses as "logged").
    teams: the team of every player, for a "logged" match file (which only holds the team of `ind`); reading one without
    them is an error.  Offline files (players == 1) read the same in every layout."""
    if layout not in LAYOUTS:
        raise ValueError("layout must be one of %s" % (LAYOUTS,))
    tok = open(path).read().split()
    if layout != "auto":
        return _parse(tok, layout, teams)
    try:
        return _parse(tok, "logged", teams)
    except ValueError as e:
        if len(tok) > 0 and _is_int(tok[0]):
            raise  # it begins like a "logged" file: the complaint about that layout is the useful one
        first = e
    try:
        return _parse(tok, "replay", teams)
    except ValueError as e:
        raise ValueError("neither layout fits: as 'logged': %s; as 'replay': %s" % (first, e))


def workload_for(sample, rows, cols, map_bytes, portal=None, floors=1, mode=abi.MODE_SOLO, level=1, H=64, Z=64, B=256,
                 P=16, chests=9000, device=0, arenas=1):
    """A one-arena workload that replays `sample` on the given map with the sample's character record; for a match
    sample: match_workload_for."""
    if sample.players > 1:
        return match_workload_for(sample, rows, cols, map_bytes, portal, floors=floors, H=H, Z=Z, B=B, P=P, chests=chests,
                                  device=device, arenas=arenas)
    cfg = config.make_config(arenas, rows, cols, floors=floors, H=H, Z=Z, B=B, P=P, chests=chests, mode=mode, level=level,
                             auto_reset=0, player_tokens=sample.profile_tokens, device=device)
    return config.Workload("replay", cfg, map_bytes, portal or [-1] * (floors * rows * cols))


def match_workload_for(sample, rows, cols, map_bytes, portal=None, floors=1, H=64, Z=64, B=256, P=32, chests=9000, device=0,
                       arenas=1):
    """The Battle workload of a logged match as the logging client saw it: n_agents = players, `ind`, the teams and one
    character record per player from the file's blobs (what lockstep.MatchClient.workload builds from the wire)."""
    if any(t is None for t in sample.teams):
        raise ValueError("the teams of the other players are unknown: read the sample with teams=")
    cfg = config.make_config(arenas, rows, cols, floors=floors, H=H, Z=Z, B=B, P=P, chests=chests, mode=abi.MODE_BATTLE,
                             level=1, n_agents=sample.players, teams=sample.teams, auto_reset=0,
                             player_tokens=sample.profile_tokens, device=device, ind=sample.ind, agent_tokens=sample.records)
    return config.Workload("replay-match", cfg, map_bytes, portal or [-1] * (floors * rows * cols))


def _profile_tokens(p):
    """The 32 integers of a character record from an abi.Profile (the inverse of abi.Profile.from_tokens)."""
    t = [p.def_hp, p.mindamage_def, p.def_stamina, p.level_solo, p.level_timer, p.level_squad, p.money, p.rate_solo,
         p.rate_timer, p.rate_squad, p.rate] + [p.cons[i] for i in range(4)]
    for i in range(4):
        t += [p.throw_lvl_cnt[i][0], p.throw_lvl_cnt[i][1]]
    return [int(x) for x in t + [p.weapon_lvl[i] for i in range(8)] + [p.backpack_lvl]]


def samples_from_recording(games, data, like):
    """The games a Recorder collected (env.Recorder.collect: int32 [n][12] game records, the streams back to back) as
    Samples, one per game in the order delivered: seed and command stream from the recording; `ind`, the teams, names and
    character records — which the recorder does not know — from `like`, a Sample (a match the games continue or resemble)
    or the workload the games were played on (Battle: one player per commanded human, the records of its configuration,
    names p0, p1, ...; other modes: the one player's own lines, as the reference logs an offline game, so n_agents must be
    1).  Each Sample carries the game's record as .recorded (arena, episode, iterations, end, outcome).  write_sample then
    produces files the reference reads."""
    from . import env
    d = env.decode_games(games)
    data = np.asarray(data, dtype=np.uint8)
    if isinstance(like, Sample):
        proto = dict(profile_tokens=like.profile_tokens, name=like.name, ind=like.ind, team=like.team, players=like.players,
                     names=like.names, records=like.records, teams=like.teams, ip=like.ip, port=like.port, password=like.password)
    else:
        cfg = like.cfg
        n = cfg.n_agents
        if cfg.mode != abi.MODE_BATTLE and n != 1:
            raise ValueError("only a Battle match logs other players' lines: pass a Sample to say who the players are")
        recs = [_profile_tokens(cfg.agent_profile[i] if cfg.n_agent_profiles else cfg.player) for i in range(n)]
        teams = [int(cfg.agent_team[i]) for i in range(n)] if n > 1 else [1]
        proto = dict(profile_tokens=recs[cfg.ind], name="p%d" % cfg.ind, ind=cfg.ind, team=teams[cfg.ind], players=n,
                     names=["p%d" % i for i in range(n)], records=recs, teams=teams)
    out = []
    for i in range(len(d["arena"])):
        off, n = int(d["offset"][i]), int(d["lines"][i])
        if off < 0 or off + n > len(data):
            raise ValueError("game %d: its stream [%d, %d) lies outside the %d bytes given" % (i, off, off + n, len(data)))
        s = Sample(int(d["tb"][i]), int(d["serial"][i]), commands=data[off:off + n].tobytes().decode("latin-1"), **proto)
        s.recorded = dict(arena=int(d["arena"][i]), episode=int(d["episode"][i]), iterations=int(d["iterations"][i]),
                          end=int(d["end"][i]), outcome=int(d["outcome"][i]))
        out.append(s)
    return out


ReplayResult = collections.namedtuple("ReplayResult", "iterations state cursor")


def replay_lines(sample, sim, on_iteration=None):
    """The replay loop with the lines fetched on the host, on any backend with the split step (step_begin, agent_alive,
    step_end) — the definition the device form (ArenaBatch.replay_step) is tested against.  Per iteration the command of
    `ind` is the next line; after step_begin every commanded human g != ind that agent_alive reports takes the next
    line, slots ascending, the others get '+'; then step_end.  Stops at a loop top: where check_end has ended the game
    ("game ended", the rest unread, gameplay.hpp:1450), or the lines have run out ("sample ended"); a stream cut in the
    middle of an iteration leaves the humans without a line '+' and ends as "truncated" at the next loop top.
    on_iteration(n, sim, taken): after the reset (n = 0) and after iteration n (1-based), taken = uint8 [players], the
    line each player took in it, 0 where none.
    Returns ReplayResult(iterations, state (abi.REPLAY_*), cursor)."""
    sim.reset((C.c_uint64 * 1)(sample.tb), (C.c_uint64 * 1)(sample.serial))
    tok, n_pl, ind = sample.commands, sim.cfg.n_agents, sample.ind
    cur = n = 0
    cut = False
    if on_iteration:
        on_iteration(0, sim, np.zeros(n_pl, dtype=np.uint8))
    while True:
        if cut:
            return ReplayResult(n, abi.REPLAY_TRUNCATED, cur)
        if sim.done()[0]:
            return ReplayResult(n, abi.REPLAY_GAME_ENDED, cur)
        if cur == len(tok):
            return ReplayResult(n, abi.REPLAY_SAMPLE_ENDED, cur)
        cmd = np.full(n_pl, ord("+"), dtype=np.uint8)
        taken = np.zeros(n_pl, dtype=np.uint8)
        cmd[ind] = taken[ind] = ord(tok[cur])
        cur += 1
        sim.step_begin()
        alive = np.asarray(sim.agent_alive()).reshape(-1)[:n_pl]
        for g in range(n_pl):
            if g == ind or not alive[g]:
                continue
            if cur < len(tok):
                cmd[g] = taken[g] = ord(tok[cur])
                cur += 1
            else:
                cut = True
        sim.step_end(cmd)
        n += 1
        if on_iteration:
            on_iteration(n, sim, taken)


def replay(sample, sim):
    """Feeds the sample's command stream to `sim` (already constructed on workload_for(sample, ...)); stops when the
    episode ends, like the reference's loop.  Returns the number of iterations played.  (A match: replay_lines, which
    also tells how the replay ended.)"""
    if sample.players > 1:
        return replay_lines(sample, sim).iterations
    tb = (C.c_uint64 * 1)(sample.tb)
    sr = (C.c_uint64 * 1)(sample.serial)
    sim.reset(tb, sr)
    n = 0
    for ch in sample.commands:
        if sim.done()[0]:
            break
        sim.step(np.array([ord(ch)], dtype=np.uint8))
        n += 1
    return n


def replay_batch(samples, sim, max_iterations=None):
    """Many samples at once on an ArenaBatch, one per arena, the lines fetched on the device (sf_replay_load /
    sf_replay_step): no host round trip inside an iteration.  An env has ONE sf_config, so the samples must share what it
    holds — the number of players, `ind`, the teams, every player's character record (and the map, mode and level `sim`
    was built with, e.g. on workload_for(samples[0], ..., arenas=len(samples))); they differ in seed and commands.  A
    batch whose records differ is refused rather than replayed wrongly.  Steps until every arena has stopped (the status
    is read back every 16 iterations) and returns the status, int32 [arenas][4] = state, cursor, iterations, 0."""
    if len(samples) != sim.cfg.arenas:
        raise ValueError("replay_batch takes one sample per arena")
    s0 = samples[0]
    for k, s in enumerate(samples):
        if (s.players, s.ind, s.records, s.teams) != (s0.players, s0.ind, s0.records, s0.teams):
            raise ValueError("sample %d differs from sample 0 in players / ind / teams / character records: one env has "
                             "one sf_config (per-arena records are not supported)" % k)
    if s0.players != sim.cfg.n_agents or s0.ind != sim.cfg.ind:
        raise ValueError("the env was not built for these samples (n_agents / ind)")
    n = len(samples)
    sim.reset((C.c_uint64 * n)(*[s.tb for s in samples]), (C.c_uint64 * n)(*[s.serial for s in samples]))
    sim.replay_load(samples)
    limit = max_iterations if max_iterations is not None else max(len(s.commands) for s in samples) + 2
    it = 0
    while True:
        st = sim.replay_status()
        if (st[:, 0] != abi.REPLAY_RUNNING).all() and sim.done().all():
            return st
        if it >= limit:
            raise RuntimeError("replay_batch: arenas still running after %d iterations" % it)
        for _ in range(16):
            sim.replay_step()
        it += 16
