"""The condition on the reference of tests/test_gpu_policy_edges.py, checked on the CPU.  The HIP kernels are held to the
float64 form of the restatement (oracle/policy_ref.py, forward_batched(dtype=torch.float64)); the f32 form is what is
pinned on the reference's own AgentModel (tests/test_ref_modules.py).  For every case the GPU tests run
(tests/policy_cases.py: parameter set x observation maker x horizon) the two forms are run side by side, the same action
fed to both, and the f32 one must stay within HALF of the gate around the f64 one on probabilities, value and state at
every step.  So at least half of each gate is left for a kernel: the reference cannot hide a kernel's error, and a kernel
that passes against f64 is within 1.5 gates of the pinned f32 form.

Measured when this was written (fractions of the gate, f32 against f64; action fed back by arg-max, 16 and 33 agents,
one agent blanked every 7th step): gain 1, 200 steps at 1 % density 0.017 on probabilities / value and 0.09 on the state;
gain 0.3 0.007 / 0.02; gain 3 0.08 / 0.31 to 0.43 (three seeds, 200 steps; 30 % density, 40 steps); gain 4 0.11 / 0.59 and
gain 8 0.30 / 1.15: gain 3 is the largest that holds the condition, so it is the largest the GPU tests use."""
import numpy as np
import pytest
import torch

import policy_cases as pc
from policy_cases import policy_ref


@pytest.mark.parametrize("key", sorted(pc.CASES))
def test_the_f32_restatement_leaves_half_of_the_gate_free(key, capsys):
    case = pc.CASES[key]
    r64 = pc.reference64(key)
    r32 = pc.run_reference(case, torch.float32, actions=r64.action)
    assert r64.probs[0].dtype == np.float64 and r64.h[0].dtype == np.float64 and r32.probs[0].dtype == np.float32
    pv = max(max(pc.gate_fraction(r32.probs[t], r64.probs[t]), pc.gate_fraction(r32.value[t], r64.value[t])) for t in range(case.steps))
    st = max(pc.gate_fraction(r32.h[t], r64.h[t], state=True) for t in range(case.steps))
    lo = min(float(p.min()) for p in r64.probs)
    hi = max(float(p.max()) for p in r64.probs)
    with capsys.disabled():
        print("\n  %-28s %3d agents x %3d steps: f32 uses %.3f of the gate on probabilities / value, %.3f on the state "
              "(probabilities %.1e .. %.2f)" % (key, case.B, case.steps, pv, st, lo, hi), end="")
    assert pv <= 0.5 and st <= 0.5, (key, pv, st)


def test_the_cases_reach_what_they_are_there_for():
    """gain 3 saturates: probabilities below 1e-4 and above 0.9 occur; default init stays flat; resets happen in the
    middle of the long run; the partial batch starts from a running agent's memory."""
    p3 = np.concatenate([p.ravel() for p in pc.reference64("long/gain-3").probs])
    p1 = np.concatenate([p.ravel() for p in pc.reference64("long/gain-1").probs])
    assert p3.min() < 1e-4 and p3.max() > 0.9
    assert p1.min() > 1e-4 and p1.max() < 0.9
    long3 = pc.reference64("long/gain-3")
    t = pc.LONG_RESET_AT
    assert len(set(np.concatenate(long3.action).tolist())) > 3  # the action fed back is not always the same one
    assert np.abs(long3.h[t - 1][:, list(pc.LONG_RESET)]).max() > 0.1
    h, a = pc.CASES["partial/gain-1"].memory()
    assert np.abs(h).min(axis=(0, 2)).max() < 1 and np.abs(h).max() > 0.9 and len(set(a.argmax(axis=1).tolist())) == 9
    assert 10 <= len(pc.PARTIAL_RESET) <= 30 and min(pc.PARTIAL_RESET) < 15


def test_float64_form_is_the_same_function_and_the_default_is_unchanged():
    rng = np.random.default_rng(3)
    params = pc.parameters("gain-1")
    obs = pc.obs_dense30(rng, 3)
    h, a = pc.random_memory(rng, 3)
    p32, v32, h32 = policy_ref.forward_batched(params, obs, h, a)
    q32, w32, g32 = policy_ref.forward_batched(params, obs, h, a, dtype=torch.float32)
    assert p32.dtype == v32.dtype == h32.dtype == np.float32
    assert np.array_equal(p32, q32) and np.array_equal(v32, w32) and np.array_equal(h32, g32)
    p64, v64, h64 = policy_ref.forward_batched(params, obs, h, a, dtype=torch.float64)
    assert p64.dtype == v64.dtype == h64.dtype == np.float64
    np.testing.assert_allclose(p32, p64, rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(h32, h64, rtol=1e-5, atol=1e-6)
    assert not np.array_equal(p32.astype(np.float64), p64)  # (f64 arithmetic, not f32 results converted)


def test_lists_from_dense_follows_the_documented_format():
    """Entries in channel, row, column order; key = channel * 9 | row << 9 | column << 14; the true count with a cut list;
    pov = the five centre cells, channel fastest; the scattered list is the image again."""
    e = pc.edge_images()
    keys, vals, counts, pov = pc.lists_from_dense(e, 2048)
    assert counts.tolist() == [int(np.count_nonzero(x)) for x in e] and counts[0] == 0 and counts[4] == 1922
    assert keys[1, 0] == (31 * 9) | (30 << 9) | (30 << 14) and vals[1, 0] == np.float32(-1.5)
    assert (np.diff(keys[4, :1922].astype(np.int64) & 511) >= 0).all()  # channel is the slowest index
    assert set((keys[4, :1922] & 511).tolist()) == {12 * 9, 13 * 9}
    assert np.array_equal(pc.dense_from_lists(keys, vals, counts), e)
    assert np.array_equal(pov[2, 2 * 32:3 * 32], e[2, :, 15, 15]) and np.array_equal(pov[2, :32], e[2, :, 14, 15])
    assert np.array_equal(pov[2, 32:64], e[2, :, 15, 14]) and not pov[3].any() and pov[2].any()
    k2, v2, c2, _ = pc.lists_from_dense(e, 100)
    assert c2[4] == 1922 and np.array_equal(k2[4], keys[4, :100]) and np.array_equal(v2[4], vals[4, :100])
    x = pc.obs_with_count(np.random.default_rng(1), 129)
    assert np.count_nonzero(x) == 129


def test_action_weights_at_their_edges():
    """v[0] = 0.5 and the rest rescaled by 0.5 / (1 - p[0] + 1e-5) (Agent.hpp:204-211), where the rescale is largest."""
    p = np.array([1 - 1e-7] + [1.25e-8] * 8, dtype=np.float32)
    v = policy_ref.action_weights(p)
    assert v[0] == np.float32(0.5) and abs(v[1] * (1 - float(p[0]) + 1e-5) / 0.5 / 1.25e-8 - 1) < 1e-3
    assert not policy_ref.action_weights(np.array([0.4, 0.6, 0, 0, 0, 0, 0, 0, 0], dtype=np.float32))[2:].any()
