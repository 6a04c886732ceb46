"""Replay of logged matches with the command lines fetched ON THE DEVICE (include/strikeforce.h sf_replay_load /
sf_replay_step; sf_core.hpp replay_fetch): how many lines an iteration takes depends on who is alive after its first
half (gameplay.hpp:966-969,979-986), so the stream position is advanced where the state is.  Against the reference
client's own per-iteration digests (tests/golden/online_samples.json), against the host form of the same replay
(strikeforce_amd.replay.replay_lines: step_begin / agent_alive / step_end) and against the oracle.  Reads only
tests/golden/."""
import ctypes as C

import numpy as np
import pytest

import online_cases as oc
from oracle_lib import ArenaDump, Oracle, diff_dumps
from strikeforce_amd import abi, config, replay

pytestmark = pytest.mark.gpu


def _env(workload):
    from strikeforce_amd import env
    return env.ArenaBatch(workload)


def _taken(sim, d_buf):
    sim.replay_commands_device(d_buf.data_ptr())
    sim.synchronize()
    return d_buf.cpu().numpy().copy()


def _expected_lines(s, f):
    q = f["quit"]
    alive = [[g for g in range(3) if g != s.ind and not (q and g == q[0] and it > q[1])] for it in range(f["iterations"])]
    return oc.lines_per_iteration(s, alive)


@pytest.mark.parametrize("name", oc.NAMES)
def test_a_match_the_reference_logged_replays_on_the_device(name):
    import torch
    s, f = oc.load(name)
    sim = _env(oc.workload(s, f))
    sim.reset((C.c_uint64 * 1)(s.tb), (C.c_uint64 * 1)(s.serial))
    sim.replay_load([s])
    d_taken = torch.zeros((1, 3), dtype=torch.uint8, device="cuda")
    lines = _expected_lines(s, f)
    assert "%016x" % int(sim.digest()[0]) == f["digests"][0]
    differing = []
    for it in range(120):
        sim.replay_step()
        if "%016x" % int(sim.digest()[0]) != f["digests"][it + 1]:
            differing.append(it)
        assert _taken(sim, d_taken)[0].tolist() == lines[it], it
        assert sim.replay_status()[0].tolist() == [abi.REPLAY_RUNNING, sum(sum(1 for x in r if x) for r in lines[:it + 1]), it + 1, 0]
    assert differing == []
    if f["quit"]:  # no line for the player that has left, from the iteration after its '_' on
        assert lines[f["quit"][1]][f["quit"][0]] == ord("_") and all(r[f["quit"][0]] == 0 for r in lines[f["quit"][1] + 1:])
    # the 121st call is the loop top that finds the stream empty: exactly hdr.done / hdr.outcome change
    assert not sim.done()[0]
    before = ArenaDump(*sim.dump_raw(0))
    sim.replay_step()
    after = ArenaDump(*sim.dump_raw(0))
    a, b = before.as_dict(), after.as_dict()
    assert (a["hdr"]["done"], a["hdr"]["outcome"], b["hdr"]["done"], b["hdr"]["outcome"]) == (0, abi.RUNNING, 1, abi.SAMPLE_END)
    a["hdr"]["done"], a["hdr"]["outcome"] = 1, abi.SAMPLE_END
    assert diff_dumps(a, b) is None
    assert int(sim.digest()[0]) == oc.digest_of_dump(before, sim.cfg, done=1, outcome=abi.SAMPLE_END)
    assert oc.digest_of_dump(before, sim.cfg) == int(f["digests"][-1], 16)
    assert sim.replay_status()[0].tolist() == [abi.REPLAY_SAMPLE_ENDED, len(s.commands), 120, 0]
    assert sim.done()[0] == 1 and after.hdr.episodes == 0 and not sim.results().any()
    assert not _taken(sim, d_taken).any()
    # a 122nd call changes nothing at all
    digest = int(sim.digest()[0])
    sim.replay_step()
    assert diff_dumps(b, ArenaDump(*sim.dump_raw(0)).as_dict()) is None and int(sim.digest()[0]) == digest
    assert sim.replay_status()[0].tolist() == [abi.REPLAY_SAMPLE_ENDED, len(s.commands), 120, 0]
    # sf_reset rewinds the stream; freeing the streams turns the entry points off again
    sim.reset((C.c_uint64 * 1)(s.tb), (C.c_uint64 * 1)(s.serial))
    assert sim.replay_status()[0].tolist() == [abi.REPLAY_RUNNING, 0, 0, 0]
    sim.replay_step()
    assert "%016x" % int(sim.digest()[0]) == f["digests"][1]
    sim.replay_load(None)
    from strikeforce_amd.env import StrikeForceError
    with pytest.raises(StrikeForceError, match="no command streams loaded"):
        sim.replay_step()


@pytest.mark.parametrize("name", oc.NAMES)
def test_the_device_fetch_equals_the_host_fetch(name):
    s, f = oc.load(name)
    host, digests = _env(oc.workload(s, f)), []
    end = replay.replay_lines(s, host, lambda n, sim, row: digests.append("%016x" % int(sim.digest()[0])))
    assert end == (120, abi.REPLAY_SAMPLE_ENDED, len(s.commands))
    assert digests == f["digests"]
    dev = _env(oc.workload(s, f))
    st = replay.replay_batch([s], dev)
    assert st[0].tolist() == [abi.REPLAY_SAMPLE_ENDED, len(s.commands), 120, 0]
    assert int(dev.digest()[0]) == oc.digest_of_dump(ArenaDump(*host.dump_raw(0)), host.cfg, done=1, outcome=abi.SAMPLE_END)


def test_a_replay_needs_a_single_episode_env():
    from strikeforce_amd.env import StrikeForceError
    s, f = oc.load("online_plain")
    w = oc.workload(s, f)
    w.cfg.auto_reset = 1
    sim = _env(w)
    with pytest.raises(StrikeForceError, match="auto_reset"):
        sim.replay_load([s])
    with pytest.raises(StrikeForceError, match="no command streams loaded"):
        sim.replay_status()


def test_a_batch_of_4096_arenas_each_stops_at_its_own_length(tmp_path):
    """96 matches played here on the oracle (40 ... 160 iterations; in every sixth a rival quits, every sixth is cut in the
    middle of its last iteration), written as samples, read back and spread over 4096 arenas.  The oracle replays every
    one of the 96 with the lines fetched on the host: final digest (its final dump with done = 1, outcome =
    SF_SAMPLE_END put in, where the sample ended), cursor and state of EVERY arena must equal its sample's."""
    A = 4096
    made = oc.batch_samples(tmp_path)
    kinds = [k for _, k, _ in made]
    lengths = [n for _, _, n in made]
    # conditions on the inputs
    assert kinds.count("quit") >= 8 and kinds.count("cut") >= 8 and min(lengths) == 40 and max(lengths) == 160
    rng = np.random.RandomState(4096)
    which = np.concatenate([np.arange(len(made)), rng.randint(0, len(made), size=A - len(made))])
    assert len(set(which[:64].tolist())) >= 64 and set(which.tolist()) == set(range(len(made)))
    expect = []
    for s, kind, iters in made:
        o = Oracle(oc.workload(s, oc.BATCH))
        end = replay.replay_lines(s, o)
        # the sample's own bookkeeping: every line is taken, in as many iterations as were played; "truncated" iff it was cut
        assert end == (iters, abi.REPLAY_TRUNCATED if kind == "cut" else abi.REPLAY_SAMPLE_ENDED, len(s.commands)), (kind, end)
        if kind == "quit":
            assert len(s.commands) < 3 * iters
        expect.append((end, oc.digest_of_dump(o.dump(0), o.cfg, done=1, outcome=abi.SAMPLE_END)))
    samples = [made[k][0] for k in which]
    sim = _env(oc.workload(samples[0], oc.BATCH, arenas=A))
    sim.reset((C.c_uint64 * A)(*[s.tb for s in samples]), (C.c_uint64 * A)(*[s.serial for s in samples]))
    sim.replay_load(samples)
    own = np.array([expect[k][0].iterations for k in which])
    for it in range(1, 164):
        sim.replay_step()
        if it in (50, 100, 150):  # every arena stops at its own length while the others go on
            st = sim.replay_status()
            stopped = own < it
            assert (st[stopped, 2] == own[stopped]).all() and (st[~stopped, 2] == it).all()
            assert (st[~stopped, 0] == abi.REPLAY_RUNNING).all() and (sim.done() == stopped).all()
    st, digests = sim.replay_status(), sim.digest()
    assert sim.done().all()
    for a in range(A):
        end, dg = expect[which[a]]
        assert st[a].tolist() == [end.state, end.cursor, end.iterations, 0], a
        assert int(digests[a]) == dg, a
    d = sim.dump(17)
    assert (d.hdr.done, d.hdr.outcome, d.hdr.episodes) == (1, abi.SAMPLE_END, 0)
    # the same through replay_batch, and a batch whose character records differ is refused
    st2 = replay.replay_batch(samples, sim)
    assert (st2 == st).all() and (sim.digest() == digests).all()
    other = replay.Sample(1, 2, config.HUMAN_TOKENS, "+", players=3, ind=1, team=2, teams=[1, 2, 3], records=[config.HUMAN_TOKENS] * 3)
    with pytest.raises(ValueError, match="character records"):
        replay.replay_batch([other] + samples[1:], sim)


def test_an_offline_sample_takes_the_same_path():
    """One player: the replay_step path ends, before the stopping call, in the digest of today's loop over sf_step."""
    rng = np.random.RandomState(11)
    s = replay.Sample(1771155561, 1073741823, config.HUMAN_ENEMY_TOKENS,
                      "".join(abi.BENCH_COMMANDS[i] for i in rng.randint(0, 28, size=100)), name="1")
    m, portal = config.synthetic_map(30, 100, portal_pairs=2)
    a, b = (_env(replay.workload_for(s, 30, 100, m, portal, H=16, Z=32, B=64)) for _ in range(2))
    assert replay.replay(s, a) == 100 and not a.done()[0]
    b.reset((C.c_uint64 * 1)(s.tb), (C.c_uint64 * 1)(s.serial))
    b.replay_load([s])
    for _ in range(100):
        b.replay_step()
    assert int(b.digest()[0]) == int(a.digest()[0]) and not b.done()[0]
    assert b.replay_status()[0].tolist() == [abi.REPLAY_RUNNING, 100, 100, 0]
    b.replay_step()
    assert b.replay_status()[0].tolist() == [abi.REPLAY_SAMPLE_ENDED, 100, 100, 0] and b.done()[0]
    assert diff_dumps(dict(ArenaDump(*a.dump_raw(0)).as_dict(), hdr=None), dict(ArenaDump(*b.dump_raw(0)).as_dict(), hdr=None)) is None


def test_the_episode_log_records_games_not_sample_ends():
    """Episode log on: no record for an arena whose lines ran out, one for a game that check_end ends (`ind` gives up in
    iteration 11: Hp 0, gameplay.hpp:696-699, dead at the loop top that follows)."""
    s, f = oc.load("online_plain")
    t, _ = oc.load("online_plain")
    t.commands = t.commands[:30] + "_" + t.commands[31:]
    sim = _env(oc.workload(s, f, arenas=2))
    sim.enable_episode_log(4)
    st = replay.replay_batch([s, t], sim)
    assert st[0].tolist() == [abi.REPLAY_SAMPLE_ENDED, len(s.commands), 120, 0]
    assert st[1, 0] == abi.REPLAY_GAME_ENDED and st[1, 1] == 3 * st[1, 2] < len(t.commands) and 11 <= st[1, 2] < 20
    host = Oracle(oc.workload(t, f))
    assert replay.replay_lines(t, host) == (st[1, 2], abi.REPLAY_GAME_ENDED, st[1, 1])
    assert int(sim.digest()[1]) == int(host.digest()[0])
    records, (written, lost, pending) = sim.episodes()
    from strikeforce_amd import env
    rec = env.decode_episodes(records, 3)
    assert (written, lost, pending) == (1, 0, 0) and rec["arena"].tolist() == [1] and rec["steps"].tolist() == [st[1, 2]]
    assert rec["outcome"].tolist() == [sim.dump(1).hdr.outcome] and rec["outcome"][0] != abi.SAMPLE_END
    assert (sim.dump(0).hdr.episodes, sim.dump(1).hdr.episodes) == (0, 1)
    assert not sim.results()[0].any() and sim.results()[1].any()
