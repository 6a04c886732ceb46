#!/usr/bin/env python3
"""Generates tests/golden/reward_vectors.json from the REFERENCE's network: oracle/_ref/libsf_refmodules.so =
bots/bot-0.5/Modules.hpp:26-180 compiled unedited against the libtorch inside the torch wheel (oracle/ref_modules.py).
bots/bot-1/RewardNet.hpp:26-136 is those lines character for character and RewardModel's head is AgentModel's value
head, so RewardModel::forward(one_hot(a), x) (RewardNet.hpp:161-166) is update_actions(a) + forward(x) on that model
holding the reward model's parameters, its value output being D (tests/test_reward_ref.py checks the text).  For two
seeded parameter sets, 8 agents (one compiled model each) and 6 recurrent steps on seeded 1 % dense observations, two
agents restarted in front of step 3: D, log D (torch.log of the f32 D, what RewardNet::get_reward returns, :257) and a
checksum of the recurrent state.  Everything is regenerated from the seeds recorded here; no image is stored.  Needs the
reference build; the vectors travel.  `run_restatement()` is the same trajectory through oracle/policy_ref.py.

    python tests/golden/make_reward_vectors.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import policy_cases as pc  # noqa: E402
import reward_cases as rc  # noqa: E402

PARAM_SETS = ("gain-1", "gain-3")  # reward_cases.PARAM_SETS: the seeds and gains are recorded in the file
AGENTS, STEPS, OBS_SEED, ACTION_SEED, RESET_AT, RESET = 8, 6, 77, 78, 3, (1, 5)


def trajectory():
    """([obs [8, 32, 31, 31]] x 6, actions [6, 8])"""
    rng = np.random.default_rng(OBS_SEED)
    obs = [pc.obs_sparse1(rng, AGENTS) for _ in range(STEPS)]
    return obs, np.random.default_rng(ACTION_SEED).integers(0, 9, size=(STEPS, AGENTS))


def _record(disc, h):
    disc = np.asarray(disc, dtype=np.float32)
    return {"disc": [float(x) for x in disc], "reward": [float(x) for x in torch.log(torch.from_numpy(disc)).numpy()],
            "h_abs_sum": [float(np.abs(h[g]).sum()) for g in range(2)]}


def _run(generator, one_set):
    obs, acts = trajectory()
    out = {"_generator": generator, "agents": AGENTS, "steps": STEPS, "obs_maker": "policy_cases.obs_sparse1", "obs_seed": OBS_SEED,
           "action_seed": ACTION_SEED, "reset_at": RESET_AT, "reset": list(RESET), "sets": []}
    for name in PARAM_SETS:
        out["sets"].append({"params": name, "init_parameters": rc.PARAM_SETS[name], "actions": [[int(a) for a in r] for r in acts],
                            "obs_nonzero": [int((o != 0).sum()) for o in obs], "steps": one_set(rc.parameters(name), obs, acts)})
    return out


def run():
    """The reference's compiled model itself (one per agent)."""
    import refmodules
    if refmodules.lib() is None:
        raise SystemExit("oracle/_ref/libsf_refmodules.so is not built: run python oracle/ref_modules.py on a machine "
                         "with the reference checkout")

    def one_set(params, obs, acts):
        models = [refmodules.RefAgentModel(params) for _ in range(AGENTS)]
        steps = []
        for t in range(STEPS):
            if t == RESET_AT:
                for b in RESET:
                    models[b].reset_memory()
            outs = []
            for b, m in enumerate(models):
                m.update_actions(int(acts[t][b]))
                outs.append(m.forward(obs[t][b]))
            steps.append(_record([o[1] for o in outs], np.stack([o[2] for o in outs], axis=1)))
        return steps
    return _run("tests/golden/make_reward_vectors.py run(): oracle/_ref/libsf_refmodules.so = the reference's "
                "bots/bot-0.5/Modules.hpp:26-180 compiled unedited (oracle/ref_modules.py), libtorch f32 on the CPU", one_set)


def run_restatement():
    """The same trajectory through oracle/policy_ref.forward_batched (f32)."""
    def one_set(params, obs, acts):
        h = np.zeros((2, AGENTS, 160), dtype=np.float32)
        steps = []
        for t in range(STEPS):
            if t == RESET_AT:
                h = np.array(h)
                h[:, list(RESET)] = 0
            disc, _, h = rc.step_reference(params, obs[t], h, acts[t], torch.float32)
            steps.append(_record(disc, h))
        return steps
    return _run("tests/golden/make_reward_vectors.py run_restatement(): oracle/policy_ref.py", one_set)


if __name__ == "__main__":
    path = os.path.join(HERE, "reward_vectors.json")
    json.dump(run(), open(path, "w"), indent=1)
    print("wrote", path)
