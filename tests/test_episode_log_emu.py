"""The episode log's k_step part (sf_core.hpp latch_results<true>, the code of the k_step instance launched while the log
is on) on the CPU wave emulator: the device core runs in K = 100 step launches with the log on, and after every launch its
raw rings must equal what the oracle, stepped one step at a time, says: each finished episode's sfo_results behind its
header, episode e in slot e & (depth - 1).

One-agent records on C3 and C2.  Records of 6 and of 16 agents on two cases of tests/episode_log_cases.py, whose quit
schedule ends up to 13 games per arena and launch of 40 steps; and the first launch of every variant world, with the
instance the host picks for it.

The emulator (tests/emu/sf_emu.cpp) exports sf_episode_log / sf_episode_ring over its runtime.  k_ep_late (the split
step's records, the rings emptied by sf_reset on the device) has no emulator counterpart:
tests/test_gpu_episode_log.py and tests/test_gpu_episode_log_edges.py cover it."""
import numpy as np
import pytest

import emu_lib
import episode_log_cases as ec
import variant_cases as vc
from episode_log_ref import OracleEpisodes
from oracle_lib import Oracle
from strikeforce_amd import config, env

SF_ERR_ARG = -1


class EmuLog(emu_lib.Emu):
    def episode_log(self, depth):
        return self.L.sfe_episode_log(self.h, depth)

    def ring(self, depth):
        out = np.zeros((self.cfg.arenas, depth, env.episode_record_words(self.cfg.n_agents)), dtype=np.int32)
        assert self.L.sfe_episode_ring(self.h, out.ctypes.data) == 0
        return out


def workload(which, arenas):
    w = config.baseline_workload(which, arenas=arenas)
    if which == "C3":
        w.cfg.timer_frames_per_level = 30  # every Timer episode ends at frame 31 unless the player dies first
    w.cfg.reseed_stride = 1000
    return w


@pytest.mark.parametrize("which,arenas,steps,depth", [("C3", 6, 400, 8), ("C3", 4, 300, 2), ("C2", 8, 1200, 8)])
def test_emulated_rings_equal_the_oracle_after_every_launch(which, arenas, steps, depth):
    w = workload(which, arenas)
    e = EmuLog(w)
    assert e.episode_log(depth) == 0
    tb, sr = w.seeds()
    e.reset(tb, sr)
    o = OracleEpisodes(Oracle(w), tb, sr)
    assert (e.ring(depth) == -1).all()
    cmds, _ = config.bench_commands(arenas, 1, steps)
    several = False
    for s0 in range(0, steps, 100):
        before = o.ended()
        e.step_many(cmds[s0:s0 + 100])
        for s in range(s0, s0 + 100):
            o.step(cmds[s])
        several |= bool((o.ended() - before >= 2).any())
        got, want = e.ring(depth), o.ring(depth)
        assert (got == want).all(), np.argwhere(got != want)[:5]
    if which == "C3":  # the case the log exists for (C2: data-dependent ends, fewer of them)
        assert o.ended().min() >= 2 and several
    assert o.ended().sum() >= 1
    # the newest record of every arena is what sf_results latched
    res = e.results()
    for a in range(arenas):
        n = o.ended()[a]
        if n == 0:
            continue
        assert (e.ring(depth)[a, (n - 1) & (depth - 1), env.EPISODE_HDR_WORDS:] == res[a].reshape(-1)).all()
    # a second sf_reset empties the rings, and the first episode is 0 again
    e.reset(tb, sr)
    assert (e.ring(depth) == -1).all()
    o2 = OracleEpisodes(Oracle(w), tb, sr)
    e.step_many(cmds[:100])
    for s in range(100):
        o2.step(cmds[s])
    assert (e.ring(depth) == o2.ring(depth)).all()
    e.close()


@pytest.mark.parametrize("case", ec.EMULATED, ids=lambda c: c.name)
def test_emulated_rings_of_many_agents(case):
    """latch_results<true> under 6 agents (KITS: 56-word records) and under 16 (a variant_cases world: 136 words), five
    arenas under the schedule of tests/episode_log_cases.py, depth 4 with arenas that end 13, 5, 4, 3, 1 and 0 games in a
    launch of 40 steps; what the records carry is asserted in tests/test_episode_log_cases.py."""
    run = ec.oracle_run(case)
    w = case.workload()
    e = EmuLog(w)
    assert e.episode_log(case.depth) == 0
    e.reset(*case.seeds())
    cmds = case.commands()
    launches = case.launches()[:6]
    for i, (s0, n) in enumerate(launches):
        e.step_many(cmds[s0:s0 + n])
        got, want = e.ring(case.depth), run.ring(i)
        assert (got == want).all(), (i, np.argwhere(got != want)[:5])
    assert e.last_variant("step") == vc.expected_variant(w.cfg)
    per = run.per_launch()[:len(launches)]
    assert per.max() > 3 * case.depth and {0, 1, case.depth - 1, case.depth, case.depth + 1} <= set(per.reshape(-1).tolist())
    res = e.results()  # the newest record of every arena is what sf_results latched
    for a in range(w.cfg.arenas):
        n = int(run.ends[len(launches) - 1][a])
        assert (run.o.records[a][n - 1][env.EPISODE_HDR_WORDS:] == res[a].reshape(-1)).all()
    e.close()


@pytest.mark.parametrize("case", ec.VARIANTS, ids=lambda c: c.name)
def test_host_picks_the_expected_log_instance(case):
    """All 15 variant worlds at the 5 arenas and depth 4 the device tests run them with: with the log on the host launches
    the instance variant_cases.expected_variant names (the emulated host's choice is the device host's: one dispatcher),
    and the rings behind the first launch equal the oracle's."""
    run = ec.oracle_run(case)
    w = case.workload()
    e = EmuLog(w)
    assert e.episode_log(case.depth) == 0
    e.reset(*case.seeds())
    s0, n = case.launches()[0]
    e.step_many(case.commands()[s0:s0 + n])
    assert e.last_variant("step") == vc.expected_variant(w.cfg)
    got, want = e.ring(case.depth), run.ring(0)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    e.close()


def test_log_off_leaves_the_emulated_core_as_it_was():
    w = workload("C2", 4)
    a, b = EmuLog(w), emu_lib.Emu(w)
    assert a.episode_log(4) == 0
    tb, sr = w.seeds()
    a.reset(tb, sr), b.reset(tb, sr)
    cmds, _ = config.bench_commands(4, 1, 300)
    for s0 in range(0, 300, 100):
        a.step_many(cmds[s0:s0 + 100]), b.step_many(cmds[s0:s0 + 100])
        assert (a.digest() == b.digest()).all() and (a.results() == b.results()).all() and (a.done() == b.done()).all()
    assert a.episode_log(3) == SF_ERR_ARG and a.episode_log(128) == SF_ERR_ARG
    assert a.episode_log(0) == 0

