"""The reference of the reward-network tests, checked on the CPU (no GPU needed).

bot-1's RewardModel (bots/bot-1/RewardNet.hpp:138-167) is evaluated by sf_reward_forward / sf_reward_sparse; the GPU tests
(tests/test_gpu_reward.py) hold those to the float64 form of oracle/policy_ref.forward_batched fed one_hot(action) as the
last action, under the gates of tests/reward_cases.py.  This file ties that reference down:
  * RewardNet.hpp:26-136 (ResB, GameCNN, Backbone) is Modules.hpp:26-136 character for character, where a reference
    checkout is at hand — so the compiled AgentModel (oracle/_ref/libsf_refmodules.so) with update_actions(a) in front of
    forward(x) IS RewardModel::forward(one_hot(a), x), its value output being D;
  * the f32 restatement equals that compiled model within tests/test_ref_modules.py's bound for forward_batched (1e-6
    relative; 1e-5 at weights x3, as there) over recurrent steps with a reset;
  * on every case the f32 restatement uses at most half of each gate against f64, so at least half is a kernel's;
  * tests/golden/reward_vectors.json (the compiled reference's D and log D) is what the generator writes, and the
    restatement reproduces it."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import policy_cases as pc
import refmodules
import reward_cases as rc
import test_ref_modules as trm
from strikeforce_amd import build, env, policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REF", "/root/reference")
GOLDEN = os.path.join(ROOT, "tests", "golden")
needs_refmodules = pytest.mark.skipif(refmodules.lib() is None,
                                      reason="oracle/_ref/libsf_refmodules.so not built (no reference checkout / libtorch)")


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "StrikeForce-client", "bots", "bot-1")), reason="no reference checkout")
def test_reward_model_backbone_is_the_policy_models_text():
    bots = os.path.join(REF, "StrikeForce-client", "bots")
    reward = open(os.path.join(bots, "bot-1", "RewardNet.hpp")).read().split("\n")
    agent = open(os.path.join(bots, "bot-0.5", "Modules.hpp")).read().split("\n")
    assert reward[25:136] == agent[25:136]
    assert "TORCH_MODULE(Backbone);" in reward[135] and "struct ResBImpl" in "\n".join(reward[25:40])
    head = "\n".join(reward[137:167])  # the head: AgentModel's `value`, update_actions first, sigmoid
    assert 'register_module("value", torch::nn::Sequential(' in head and "ResB(hidden_size, LAYER_INDEX), torch::nn::Linear(hidden_size, 1)" in head
    assert re.search(r"update_actions\(action\);\s+auto gated = backbone->forward\(x\);", head) and "return torch::sigmoid(value);" in head
    assert "torch::log(output)" in reward[256]


def test_reward_parameter_names_are_the_reward_models():
    s = policy.reward_parameter_shapes()
    assert len(s) == 22 and not any(k.startswith("policy.") for k in s)
    assert all(k.startswith("backbone.") or k.startswith("value.0.lin") or k.startswith("value.1.") for k in s)
    assert s["value.1.weight"] == (1, 160) and s["value.0.lin2.bias"] == (160,)
    full = policy.parameter_shapes()
    assert all(full[k] == v for k, v in s.items())


def test_library_exports_the_reward_entries():
    build.build(verbose=False)
    L = env.load_library()
    header = open(os.path.join(ROOT, "include", "strikeforce_policy.h")).read()
    declared = set(re.findall(r"\b(sf_reward_[a-z_]+)\s*\(", header))
    assert declared == set(policy.REWARD_EXPORTS), declared ^ set(policy.REWARD_EXPORTS)
    for name in declared:
        assert hasattr(L, name), name
    assert "#define SF_POLICY_ABI_VERSION 1" in header
    assert C.sizeof(policy.RewardIO) == 4 * 8 + 8 + 3 * 8 + 8 + 3 * 8  # four pointers, cap (padded), three, two ints, three


def test_load_checkpoint_accepts_a_reward_model_archive(tmp_path):
    params = rc.parameters("gain-1")
    reward_only = {k: torch.from_numpy(params[k]) for k in policy.reward_parameter_shapes()}
    path = str(tmp_path / "reward.pt")
    torch.save(reward_only, path)
    got = policy.load_checkpoint(path)
    assert set(got) == set(policy.reward_parameter_shapes()) and all(np.array_equal(got[k], params[k]) for k in got)
    full = str(tmp_path / "agent.pt")
    torch.save({k: torch.from_numpy(v) for k, v in params.items()}, full)
    assert set(policy.load_checkpoint(full)) == set(policy.parameter_shapes())
    del reward_only["value.1.bias"]
    torch.save(reward_only, path)
    with pytest.raises(ValueError, match="lacks parameter value.1.bias"):
        policy.load_checkpoint(path)


# What tests/test_ref_modules.py holds forward_batched to, taken from its own table (name, init_parameters arguments, bound):
# 1e-6 relative at default-initialised parameters and at x0.3, 1e-5 at x3 (where a batched reduction's last-bit differences
# are amplified by saturating gates).  Its four sets, and this file's two under the bound of their gain.
_BOUND_OF_GAIN = {kw.get("gain", 1.0): tol for _, kw, tol in trm.PARAM_SETS}
REF_SETS = list(trm.PARAM_SETS) + [("reward-" + n, kw, _BOUND_OF_GAIN[kw["gain"]]) for n, kw in rc.PARAM_SETS.items()]


@needs_refmodules
@pytest.mark.parametrize("name,kw,tol", REF_SETS, ids=[p[0] for p in REF_SETS])
def test_restatement_equals_the_compiled_reference(name, kw, tol):
    """6 recurrent steps of 3 agents, a reset_memory in front of the fourth: update_actions(a) + forward(x) on the compiled
    AgentModel against forward_batched(..., one_hot(a)) in f32 — D relatively and both states absolutely (they lie in
    (-1, 1)) within tests/test_ref_modules.py's bound for forward_batched at that gain: D is AgentModel's value output, so
    that bound applies unchanged.  Measured when this was written: 2.4e-6 on the reward set at weights x3 (bound 1e-5, as for
    that file's own x3 set), below 1e-6 on the sets held to 1e-6."""
    params = policy.init_parameters(**kw)
    B, T = 3, 6
    rng = np.random.default_rng(17)
    obs_seq = [pc.obs_sparse1(rng, B) for _ in range(T // 2)] + [pc.obs_dense30(rng, B) for _ in range(T - T // 2)]
    refs = [refmodules.RefAgentModel(params) for _ in range(B)]
    h = np.zeros((2, B, 160), dtype=np.float32)
    worst = 0.0
    for t, obs in enumerate(obs_seq):
        if t == 3:
            for m in refs:
                m.reset_memory()
            h[:] = 0
        acts = rng.integers(0, 9, size=B)
        disc, reward, h = rc.step_reference(params, obs, h, acts, torch.float32)
        for b in range(B):
            refs[b].update_actions(int(acts[b]))
            _, rv, rh = refs[b].forward(obs[b])
            worst = max(worst, abs(float(disc[b]) - rv) / rv, float(np.max(np.abs(h[:, b] - rh))))
            assert reward[b] == np.log(disc[b]) and reward.dtype == np.float32
    print("%s: %.3g of %.0e" % (name, worst, tol))
    assert worst <= tol, worst


@pytest.mark.parametrize("key", sorted(rc.CASES))
def test_the_f32_restatement_leaves_half_of_the_gates_free(key, capsys):
    case = rc.CASES[key]
    r64, r32 = rc.reference64(key), rc.run_reference(case, torch.float32)
    assert r64.disc[0].dtype == np.float64 and r32.disc[0].dtype == np.float32 and r32.reward[0].dtype == np.float32
    fd = max(pc.gate_fraction(r32.disc[t], r64.disc[t]) for t in range(case.steps))
    fr = max(rc.reward_fraction(r32.reward[t], r64.disc[t]) for t in range(case.steps))
    fh = max(pc.gate_fraction(r32.h[t], r64.h[t], state=True) for t in range(case.steps))
    lo, hi = min(float(d.min()) for d in r64.disc), max(float(d.max()) for d in r64.disc)
    with capsys.disabled():
        print("\n  %-28s %3d agents x %3d steps: f32 uses %.3f of the gate on D, %.3f on the reward, %.3f on the state "
              "(D %.2e .. %.2f)" % (key, case.B, case.steps, fd, fr, fh, lo, hi), end="")
    assert fd <= 0.5 and fr <= 0.5 and fh <= 0.5, (key, fd, fr, fh)
    for t in range(case.steps):
        assert rc.log_ulps(r32.reward[t], r32.disc[t]) <= 2
    if key == "saturated":  # D underflows in f32 (not in f64): log D is -inf, nothing is NaN
        assert hi < 1e-40 and all((d == 0).all() and np.isneginf(r).all() for d, r in zip(r32.disc, r32.reward))
    else:  # the reward gate is in force for every agent of every other case
        assert lo >= rc.D_FLOOR, (key, lo)


def test_the_cases_reach_what_they_are_there_for():
    d3 = np.concatenate([d for d in rc.reference64("sparse1/gain-3").disc])
    d1 = np.concatenate([d for d in rc.reference64("sparse1/gain-1").disc])
    assert d3.min() < 0.05 and d3.max() > 0.9 and 0.1 < d1.min() and d1.max() < 0.9  # x3 reaches both ends, default init neither
    case = rc.CASES["sparse1/gain-3"]
    assert len(set(case.actions().ravel().tolist())) == 9 and 0 <= case.actions().min() and case.actions().max() < 9
    t = rc.LONG_RESET_AT
    assert np.abs(rc.reference64("sparse1/gain-3").h[t - 1][:, list(rc.LONG_RESET)]).max() > 0.1
    # the action matters: another action, another D
    params, obs = rc.parameters("gain-3"), case.observations()[0]
    h = case.memory()
    a = case.actions()[0]
    d_a = rc.step_reference(params, obs, h, a, torch.float64)[0]
    d_b = rc.step_reference(params, obs, h, (a + 1) % 9, torch.float64)[0]
    assert np.abs(d_a - d_b).max() > 1e-3
    # a restarted agent differs from the running one
    r, rr = rc.reference64("partial/gain-1"), rc.reference64("partial-restarted/gain-1")
    restarted = list(rc.PARTIAL_RESET)
    assert np.abs(r.disc[0][restarted] - rr.disc[0][restarted]).max() > 1e-4


def test_reward_gate_is_the_value_gate_through_the_log():
    d = np.array([1e-3, 0.0076, 0.5, 0.98])
    g = pc.gate(d)
    for s in (-1.0, 1.0):
        assert (np.abs(np.log(d + s * g) - np.log(d)) <= g / (d - g)).all()
    assert (rc.reward_gate(d) > g / (d - g)).all()
    assert rc.log_ulps(np.array([-np.inf, np.log(np.float32(0.5))], dtype=np.float32), np.array([0.0, 0.5], dtype=np.float32)) == 0
    with pytest.raises(AssertionError):
        rc.log_ulps(np.array([np.nan], dtype=np.float32), np.array([0.5], dtype=np.float32))


# ---- the committed vectors ---------------------------------------------------------------------------------------------
def _vectors():
    sys.path.insert(0, GOLDEN)
    import make_reward_vectors
    with open(os.path.join(GOLDEN, "reward_vectors.json")) as f:
        return make_reward_vectors, json.load(f)


@needs_refmodules
def test_committed_vectors_are_the_references_outputs():
    gen, have = _vectors()
    assert "libsf_refmodules" in have["_generator"]
    assert gen.run()["sets"] == have["sets"]


def test_restatement_reproduces_the_committed_vectors():
    """D under the value gate's half, log D under the reward gate's half, against the compiled reference's f32 outputs."""
    gen, have = _vectors()
    got = gen.run_restatement()
    assert [s["params"] for s in have["sets"]] == list(gen.PARAM_SETS) and have["agents"] == 8 and have["steps"] == 6
    for g, w in zip(got["sets"], have["sets"]):
        assert g["actions"] == w["actions"] and g["obs_nonzero"] == w["obs_nonzero"]
        for gs, ws in zip(g["steps"], w["steps"]):
            d = np.array(ws["disc"])
            assert d.min() >= rc.D_FLOOR
            assert pc.gate_fraction(gs["disc"], d) <= 0.5 and rc.reward_fraction(gs["reward"], d) <= 0.5
            np.testing.assert_allclose(gs["h_abs_sum"], ws["h_abs_sum"], rtol=5e-5)
