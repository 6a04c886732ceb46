"""The fixed instances' step loop on the MI355X (k_step_fixed, sf_api.hip) where it differs from the generic loop: restarts
on a side branch of the step loop, the command pointer that runs to its end, frame % {30, 40, 50} as counters.  The
cases of tests/step_fixed_lean_cases.py at 64 arenas, every launch plan: after each launch the fixed instance equals the
oracle's digest of that step and the generic instance of the same library (an environment created under
SF_STEP_GENERIC=1) run through the same launches, sf_done included; at the end the headers (generator registers, draw
count, frame, steps, games), the per-phase draw counts and the results."""
import numpy as np
import pytest

import step_fixed_lean_cases as lean

pytestmark = pytest.mark.gpu

ARENAS = 64
_runs = {}


def _oracle(name):
    if name not in _runs:
        _runs[name] = lean.oracle_run(name, ARENAS)
    return _runs[name]


def _device(w, monkeypatch, generic):
    from strikeforce_amd import env
    if generic:
        monkeypatch.setenv("SF_STEP_GENERIC", "1")
    else:
        monkeypatch.delenv("SF_STEP_GENERIC", raising=False)
    g = env.ArenaBatch(w)  # (the variable is read once, when the environment is created)
    monkeypatch.delenv("SF_STEP_GENERIC", raising=False)
    return g


@pytest.mark.parametrize("name,plan", [(n, p) for n in sorted(lean.CASES) for p in lean.CASES[n][4]])
def test_fixed_step_loop_equals_oracle_and_generic_instance(name, plan, monkeypatch):
    import torch
    world, commands, steps, kernel, plans, fewest = lean.CASES[name]
    r = _oracle(name)
    assert (r["episodes"] >= fewest).all()
    w = world(ARENAS)
    f, g = _device(w, monkeypatch, False), _device(world(ARENAS), monkeypatch, True)
    tb, sr = w.seeds()
    f.reset(tb, sr), g.reset(tb, sr)
    cmds = commands(ARENAS, steps)
    d = torch.from_numpy(np.ascontiguousarray(cmds)).cuda()
    s = 0
    for k in plans[plan]:
        if k == 1:  # sf_step: commands from the host, one step
            f.step(cmds[s]), g.step(cmds[s])
        else:
            f.step_device(d.data_ptr() + s * ARENAS, k), g.step_device(d.data_ptr() + s * ARENAS, k)
        s += k
        assert f.step_kernel() == kernel and g.step_kernel() == lean.GENERIC, "after %d steps: instance launched" % s
        df = f.digest()
        assert (df == r["digests"][s - 1]).all(), "after %d steps (launch of %d): differs from the oracle" % (s, k)
        assert (g.digest() == df).all(), "after %d steps (launch of %d): differs from the generic instance" % (s, k)
        want = lean.done_after(r, s - k, k)
        assert (f.done() == want).all() and (g.done() == want).all(), "after %d steps (launch of %d): sf_done" % (s, k)
    assert s == steps
    assert (f.results() == r["results"]).all() and (g.results() == r["results"]).all()
    assert (f.agent_alive() == g.agent_alive()).all()
    pf, pg = f.phase_draws(), g.phase_draws()
    assert (pf == pg).all() and (pf == np.array(r["phase_draws"])).all(), "draws by phase"
    for a in range(ARENAS):
        h, hg, ho = f.dump_raw(a)[0], g.dump_raw(a)[0], r["hdrs"][a]
        assert bytes(h) == bytes(hg), "arena %d: header differs from the generic instance's" % a
        assert (h.frame, h.steps, h.episodes, h.jomle, list(h.rng)) == (ho.frame, ho.steps, ho.episodes, ho.jomle, list(ho.rng)), a
    f.close(), g.close()
