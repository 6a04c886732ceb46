"""The device form of the replay (sf_replay_load / sf_replay_step) without a GPU: sf_core.hpp Core::replay_fetch — the
body of the gfx950 kernel k_replay_fetch — on the wave emulator, between the emulated halves of the step, through the
host code of the product (sf_host.hpp Env::replay_load / replay_step); the emulator and its runtime (tests/emu) have the
two wave operations and the launcher the fetch adds.  Checked against the reference client's own per-iteration digests
(tests/golden/online_samples.json) and against the host form (replay.replay_lines)."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
import online_cases as oc
from oracle_lib import Oracle, diff_dumps
from strikeforce_amd import abi, replay


class EmuReplay(emu_lib.Emu):
    """emu_lib.Emu plus ArenaBatch's replay_* calls."""

    def replay_load(self, streams):
        if streams is None:
            return self.L.sfe_replay_load(self.h, None, None)
        rows = [getattr(s, "commands", s).encode("ascii") for s in streams]
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(r) for r in rows])
        flat = np.frombuffer(b"".join(rows) or b"\0", dtype=np.uint8)
        rc = self.L.sfe_replay_load(self.h, flat.ctypes.data, off.ctypes.data)
        assert rc == 0, self.L.sfe_last_error().decode()

    def replay_step(self):
        rc = self.L.sfe_replay_step(self.h)
        assert rc == 0, self.L.sfe_last_error().decode()

    def replay_status(self):
        out = np.zeros((self.cfg.arenas, 4), dtype=np.int32)
        assert self.L.sfe_replay_status(self.h, out.ctypes.data) == 0
        return out

    def replay_commands(self):
        out = np.zeros((self.cfg.arenas, self.cfg.n_agents), dtype=np.uint8)
        assert self.L.sfe_replay_commands(self.h, out.ctypes.data) == 0
        return out


def _expected_lines(s, f):
    q = f["quit"]
    alive = [[g for g in range(3) if g != s.ind and not (q and g == q[0] and it > q[1])] for it in range(f["iterations"])]
    return oc.lines_per_iteration(s, alive)


@pytest.mark.parametrize("name", oc.NAMES)
def test_the_fetch_body_replays_the_reference_clients_matches(name):
    s, f = oc.load(name)
    sim = EmuReplay(oc.workload(s, f))
    sim.reset((C.c_uint64 * 1)(s.tb), (C.c_uint64 * 1)(s.serial))
    sim.replay_load([s])
    lines = _expected_lines(s, f)
    digests = ["%016x" % int(sim.digest()[0])]
    for it in range(120):
        sim.replay_step()
        digests.append("%016x" % int(sim.digest()[0]))
        assert sim.replay_commands()[0].tolist() == lines[it], it
        assert sim.replay_status()[0].tolist() == [abi.REPLAY_RUNNING, sum(sum(1 for x in r if x) for r in lines[:it + 1]), it + 1, 0]
    assert [i for i, (a, b) in enumerate(zip(digests, f["digests"])) if a != b] == [] and len(digests) == 121
    before = sim.dump(0)
    sim.replay_step()  # the loop top that finds the stream empty: hdr.done / hdr.outcome, nothing else
    after = sim.dump(0)
    a, b = before.as_dict(), after.as_dict()
    assert (a["hdr"]["done"], b["hdr"]["done"], b["hdr"]["outcome"], b["hdr"]["episodes"]) == (0, 1, abi.SAMPLE_END, 0)
    a["hdr"]["done"], a["hdr"]["outcome"] = 1, abi.SAMPLE_END
    assert diff_dumps(a, b) is None
    assert int(sim.digest()[0]) == oc.digest_of_dump(before, sim.cfg, done=1, outcome=abi.SAMPLE_END)
    assert sim.replay_status()[0].tolist() == [abi.REPLAY_SAMPLE_ENDED, len(s.commands), 120, 0]
    assert sim.done()[0] == 1 and not sim.results().any() and not sim.replay_commands().any()
    sim.replay_step()
    assert diff_dumps(b, sim.dump(0).as_dict()) is None


def test_a_batch_on_the_emulator_each_arena_stops_at_its_own_length(tmp_path):
    """24 matches played here on the oracle (a rival quits in every sixth, every sixth is cut in mid-iteration), one per
    arena: state, cursor, iterations and the final digest of every arena equal the host form's on the oracle."""
    made = oc.batch_samples(tmp_path, n=24)
    assert {k for _, k, _ in made} == {"plain", "quit", "cut"}
    samples = [s for s, _, _ in made]
    sim = EmuReplay(oc.workload(samples[0], oc.BATCH, arenas=len(samples)))
    st = replay.replay_batch(samples, sim)
    digests = sim.digest()
    for a, (s, kind, iters) in enumerate(made):
        o = Oracle(oc.workload(s, oc.BATCH))
        end = replay.replay_lines(s, o)
        assert end == (iters, abi.REPLAY_TRUNCATED if kind == "cut" else abi.REPLAY_SAMPLE_ENDED, len(s.commands))
        assert st[a].tolist() == [end.state, end.cursor, end.iterations, 0], (a, kind)
        assert int(digests[a]) == oc.digest_of_dump(o.dump(0), o.cfg, done=1, outcome=abi.SAMPLE_END), (a, kind)


def test_a_game_that_check_end_ends_leaves_its_stream_unread():
    s, f = oc.load("online_plain")
    s.commands = s.commands[:30] + "_" + s.commands[31:]  # `ind` gives up in iteration 11
    sim = EmuReplay(oc.workload(s, f))
    st = replay.replay_batch([s], sim)
    o = Oracle(oc.workload(s, f))
    end = replay.replay_lines(s, o)
    assert end.state == abi.REPLAY_GAME_ENDED and st[0].tolist() == [end.state, end.cursor, end.iterations, 0]
    assert int(sim.digest()[0]) == int(o.digest()[0]) and sim.dump(0).hdr.outcome != abi.SAMPLE_END
    assert sim.dump(0).hdr.episodes == 1 and sim.results()[0].any()


def test_loading_needs_a_single_episode_env_and_a_load():
    s, f = oc.load("online_plain")
    w = oc.workload(s, f)
    w.cfg.auto_reset = 1
    sim = EmuReplay(w)
    rows = s.commands.encode()
    off = np.array([0, len(rows)], dtype=np.int64)
    assert sim.L.sfe_replay_load(sim.h, rows, off.ctypes.data) == -4 and b"auto_reset" in sim.L.sfe_last_error()
    assert sim.L.sfe_replay_step(sim.h) == -4 and b"no command streams loaded" in sim.L.sfe_last_error()
