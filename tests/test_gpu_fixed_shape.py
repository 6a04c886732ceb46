"""k_step_fixed<Shape> on the MI355X (sf_api.hip; sf_types.hpp FixedShapes): the step kernel compiled for BASELINE
configs[2]'s configuration against the generic k_step instance of the same library (an environment created under
SF_STEP_GENERIC=1) and against the oracle, bit for bit; and the host's choice between the two (sf_host.hpp Env::create).
The world and its commands are the emulator test's (test_fixed_shape_emu.py), with the Timer game 1 200 frames long: the
zombie pool is full before step 520 in some arenas, and every arena's game ends at step 600, inside the last launch."""
import numpy as np
import pytest

import test_fixed_shape_emu as fx
from episode_log_ref import OracleEpisodes
from oracle_lib import Oracle

pytestmark = pytest.mark.gpu

C3_SHAPE, C2_SHAPE = fx.C3_SHAPE, fx.C2_SHAPE
ORACLE_STEPS, PREROLL = 20, 500
LAUNCHES = (1, 7, 100)
STEPS = ORACLE_STEPS + PREROLL + sum(LAUNCHES)


def _device(w, monkeypatch, generic):
    from strikeforce_amd import env
    if generic:
        monkeypatch.setenv("SF_STEP_GENERIC", "1")
    else:
        monkeypatch.delenv("SF_STEP_GENERIC", raising=False)
    g = env.ArenaBatch(w)  # (the variable is read once, when the environment is created)
    monkeypatch.delenv("SF_STEP_GENERIC", raising=False)
    return g


def _dev(cmds):
    import torch
    return torch.from_numpy(np.ascontiguousarray(cmds)).cuda()


def _world(arenas):
    w = fx.world(arenas)
    w.cfg.timer_frames_per_level = 1200
    return w


def _same(f, g, what):
    assert (f.digest() == g.digest()).all(), what + ": digests"
    assert (f.done() == g.done()).all(), what + ": done"
    assert (f.agent_alive() == g.agent_alive()).all(), what + ": agent_alive"
    assert (f.results() == g.results()).all(), what + ": results"


@pytest.mark.parametrize("A", [130, 1100])
def test_fixed_instance_equals_generic_instance_and_oracle(A, monkeypatch):
    """130 arenas: no multiple of 64 or 1024, arena order (k_rank is off below 1024 arenas).  1 100: launches of 8 steps
    and more go through the launch order `perm`, with a partial last block of 1024."""
    w = _world(A)
    g, f = _device(w, monkeypatch, True), _device(_world(A), monkeypatch, False)
    o = Oracle(_world(A))
    tb, sr = w.seeds()
    g.reset(tb, sr), f.reset(tb, sr), o.reset(tb, sr)
    cmds = fx.commands(A, STEPS)
    d = _dev(cmds)
    for s in range(ORACLE_STEPS):  # one step per launch (sf_step)
        g.step(cmds[s]), f.step(cmds[s]), o.step(cmds[s])
        assert f.step_kernel() == C3_SHAPE and g.step_kernel() == -1, "step %d: instance launched" % s
        assert (f.digest() == o.digest()).all(), "step %d: fixed instance differs from the oracle" % s
        _same(f, g, "step %d" % s)
    o.close()
    s = ORACLE_STEPS
    for k in (PREROLL,) + LAUNCHES:
        g.step_device(d.data_ptr() + s * A, k), f.step_device(d.data_ptr() + s * A, k)
        s += k
        assert f.step_kernel() == C3_SHAPE and g.step_kernel() == -1, "launch of %d: instance launched" % k
        _same(f, g, "after %d steps (launch of %d)" % (s, k))
        if k == PREROLL:  # the pools are filled before the launches of 1, 7 and 100
            dumps = [g.dump(a) for a in range(0, A, max(1, A // 32))]
            zombies = max(sum(1 for z in x.zombies if z.alive) for x in dumps)
            assert zombies == 24, "most live zombies %d" % zombies
            assert any(b.alive for x in dumps for b in x.bullets) and any(h.alive for x in dumps for h in x.humans[1:])
    assert s == STEPS
    for a in (0, 1, A // 2, A - 1):
        x, y = f.dump_raw(a), g.dump_raw(a)
        assert bytes(x[0]) == bytes(y[0]), "arena %d: header" % a
        assert x[0].episodes >= 1, "arena %d: no game ended inside the run" % a
        for xs, ys in zip(x[1:5], y[1:5]):
            assert len(xs) == len(ys) and all(bytes(p) == bytes(q) for p, q in zip(xs, ys)), "arena %d: slot pools" % a
        for xs, ys in zip(x[5:], y[5:]):
            assert np.array_equal(xs, ys), "arena %d: cell planes" % a
    g.close(), f.close()


def test_c2_shape_equals_generic_instance_and_oracle(monkeypatch):
    """The second shape of the table (BASELINE configs[1]): 130 arenas, 20 single steps against the oracle, then launches
    of 300, 1, 7 and 100 against the generic instance; the zombie pool (16) is full behind the launch of 300."""
    from strikeforce_amd import config
    A, steps = 130, 20 + 300 + 108
    w = config.baseline_workload("C2", arenas=A)
    g, f = _device(w, monkeypatch, True), _device(config.baseline_workload("C2", arenas=A), monkeypatch, False)
    o = Oracle(config.baseline_workload("C2", arenas=A))
    tb, sr = w.seeds()
    g.reset(tb, sr), f.reset(tb, sr), o.reset(tb, sr)
    cmds, _ = config.bench_commands(A, 1, steps)
    d = _dev(cmds)
    for s in range(20):
        g.step(cmds[s]), f.step(cmds[s]), o.step(cmds[s])
        assert f.step_kernel() == C2_SHAPE and g.step_kernel() == -1
        assert (f.digest() == o.digest()).all(), "step %d: fixed instance differs from the oracle" % s
        _same(f, g, "step %d" % s)
    o.close()
    s = 20
    for k in (300, 1, 7, 100):
        g.step_device(d.data_ptr() + s * A, k), f.step_device(d.data_ptr() + s * A, k)
        s += k
        assert f.step_kernel() == C2_SHAPE and g.step_kernel() == -1
        _same(f, g, "after %d steps (launch of %d)" % (s, k))
        if k == 300:
            assert max(sum(1 for z in g.dump(a).zombies if z.alive) for a in range(0, A, 8)) == 16
    assert sum(g.dump(a).hdr.episodes for a in range(A)) >= 1, "no game ended inside the run"
    g.close(), f.close()


@pytest.mark.parametrize("change", ["H 9", "Z 25", "64 x 63", "2 x 32 x 64", "two floors", "Solo", "Squad", "two agents", "level 2", "no auto_reset", "B 65", "P 65"])
def test_any_other_configuration_runs_the_generic_instance(change, monkeypatch):
    """One fixed field off C3's shape (B 65 changes the bullet words too; P 65 moves the pools to LDS): the generic
    instance, 20 steps against the oracle at 8 arenas, in single steps and in one launch of 10."""
    A = 8
    w = fx.other_world(change, A)
    f, o = _device(w, monkeypatch, False), Oracle(fx.other_world(change, A))
    tb, sr = w.seeds()
    f.reset(tb, sr), o.reset(tb, sr)
    from strikeforce_amd import config
    cmds, _ = config.bench_commands(A, w.cfg.n_agents, 20)
    d = _dev(cmds)
    for s in range(10):
        f.step(cmds[s]), o.step(cmds[s])
        assert f.step_kernel() == -1
        assert (f.digest() == o.digest()).all(), "%s: step %d" % (change, s)
    f.step_device(d.data_ptr() + 10 * A * w.cfg.n_agents, 10)
    o.step_many(cmds[10:20])
    assert f.step_kernel() == -1
    assert (f.digest() == o.digest()).all() and (f.results() == o.results()).all(), change
    f.close(), o.close()


def test_the_episode_log_runs_the_generic_log_instance(monkeypatch):
    """While the log is on, an environment of C3's shape launches k_step<.., LOG>; the fixed instance before and after.
    The rings equal the oracle's, and so does the state once the fixed instance has taken over again."""
    A, depth = 8, 4
    w = _world(A)
    w.cfg.timer_frames_per_level = 60  # a game every 30 steps; none ends in the 20 steps before the log is on
    f = _device(w, monkeypatch, False)
    tb, sr = w.seeds()
    f.reset(tb, sr)
    o = OracleEpisodes(Oracle(w), tb, sr)
    cmds = fx.commands(A, 140)
    d = _dev(cmds)

    def launch(s0, k):
        f.step_device(d.data_ptr() + s0 * A, k)
        for s in range(s0, s0 + k):
            o.step(cmds[s])

    launch(0, 20)
    assert f.step_kernel() == C3_SHAPE and o.ended().max() == 0
    f.enable_episode_log(depth)
    for s0 in (20, 70):
        launch(s0, 50)
        assert f.step_kernel() == -1
        assert (f.episode_ring() == o.ring(depth)).all(), s0
    assert o.ended().min() >= 2
    f.enable_episode_log(0)
    launch(120, 20)
    assert f.step_kernel() == C3_SHAPE
    assert (f.digest() == o.sim.digest()).all() and (f.results() == o.sim.results()).all()
    f.close()
