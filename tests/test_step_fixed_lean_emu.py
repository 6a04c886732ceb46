"""The fixed instances' step loop on the wave emulator (tests/emu: Core<WaveEmu, .., FixedShape<..>>, the body of
k_step_fixed) at the places where it differs from the generic loop: restarts run by the loop itself, on a side
branch; a command pointer that runs to its end in place of the step number; frame % {30, 40, 50} kept as counters from
load() on.  Every case of tests/step_fixed_lean_cases.py at 8 arenas, every launch plan: after each launch the fixed instance
equals the oracle's digest of that step and the generic instance run through the same launches; with launches of one step
that is every step."""
import numpy as np
import pytest

import step_fixed_lean_cases as lean
from test_fixed_shape_emu import EmuFixed

ARENAS = 8
_runs = {}


def _oracle(name):
    if name not in _runs:
        _runs[name] = lean.oracle_run(name, ARENAS)
    return _runs[name]


@pytest.mark.parametrize("name", sorted(lean.CASES))
def test_the_oracle_run_ends_the_games_the_case_is_about(name):
    r = _oracle(name)
    steps, fewest = lean.CASES[name][2], lean.CASES[name][5]
    print("%s: games ended %s, frame at the end %s, done %s" % (name, r["episodes"], r["frames"], r["done"]))
    assert (r["episodes"] >= fewest).all()
    if name == "frames":
        assert (r["episodes"] == 0).all() and (r["frames"] == 1 + 2 * steps).all()
    if name == "no_reset":
        assert r["done"].all() and (r["frames"] == 41).all()  # ended at step 20 and not stepped since
    if name in ("last_step", "every_step"):
        # the last step ended a game and began the next (sf_done, with auto_reset: a game ended in the last launch)
        assert (r["frames"] == 1).all() and r["done"].all() and not any(h.done for h in r["hdrs"])


@pytest.mark.parametrize("name,plan", [(n, p) for n in sorted(lean.CASES) for p in lean.CASES[n][4]])
def test_fixed_step_loop_equals_oracle_and_generic_core(name, plan, monkeypatch):
    world, commands, steps, kernel, plans, _ = lean.CASES[name]
    r = _oracle(name)
    monkeypatch.delenv("SF_STEP_GENERIC", raising=False)
    w = world(ARENAS)
    f = EmuFixed(w)
    monkeypatch.setenv("SF_STEP_GENERIC", "1")
    g = EmuFixed(world(ARENAS))
    monkeypatch.delenv("SF_STEP_GENERIC")
    tb, sr = w.seeds()
    f.reset(tb, sr), g.reset(tb, sr)
    cmds = commands(ARENAS, steps)
    s = 0
    for k in plans[plan]:
        if k == 1:  # sf_step: the host's one-step launch
            f.step(cmds[s]), g.step(cmds[s])
        else:
            f.step_many(cmds[s:s + k]), g.step_many(cmds[s:s + k])
        s += k
        assert f.step_kernel() == kernel and g.step_kernel() == lean.GENERIC, "after %d steps: instance" % s
        df = f.digest()
        assert (df == r["digests"][s - 1]).all(), "after %d steps (launch of %d): differs from the oracle" % (s, k)
        assert (g.digest() == df).all(), "after %d steps (launch of %d): differs from the generic core" % (s, k)
        want = lean.done_after(r, s - k, k)
        assert (f.done() == want).all() and (g.done() == want).all(), "after %d steps (launch of %d): sf_done" % (s, k)
    assert s == steps
    assert (f.results() == r["results"]).all() and (g.results() == r["results"]).all()
    for a in range(ARENAS):
        h, hg, ho = f.dump(a).hdr, g.dump(a).hdr, r["hdrs"][a]
        assert bytes(h) == bytes(hg), "arena %d: header differs from the generic core's" % a
        assert (h.frame, h.steps, h.episodes, h.jomle, list(h.rng)) == (ho.frame, ho.steps, ho.episodes, ho.jomle, list(ho.rng))
        assert f.phase_draws(a) == g.phase_draws(a) == [int(x) for x in r["phase_draws"][a]], "arena %d: draws by phase" % a
    f.close(), g.close()
