"""The rollout buffer's restatement (tests/rollout_ref.py) on the CPU: the hand-derived vector, the torch form against
uncontracted numpy f32 bit for bit, the committed GPU inputs telling a fused multiply-add from the reference's two roundings,
the divide-by-T statistics, the bookkeeping rules, and the ABI surface of the sf_rollout_* section of
include/strikeforce_policy.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rollout_ref as rr
from strikeforce_amd import build, env, policy, rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def test_hand_derived_returns():
    """T = 4, gamma = 0.5, rewards 8, 4, 2, 1: returns[3] = 0.5, [2] = 0.25 + 1 = 1.25, [1] = 0.625 + 2 = 2.625,
    [0] = 1.3125 + 4 = 5.3125 (Agent.hpp:333-339)."""
    r = np.array([8, 4, 2, 1], dtype=np.float32)
    want = np.array([5.3125, 2.625, 1.25, 0.5], dtype=np.float32)
    assert np.array_equal(rr.returns_torch(r, 0.5), want)
    assert np.array_equal(rr.returns_numpy(r, 0.5), want)


@pytest.mark.parametrize("gamma", rr.RETURNS_GAMMAS)
def test_torch_form_equals_uncontracted_numpy_f32(gamma):
    """10^4 random rollouts (T = 16; rewards = log of a random D), the torch CPU ops against numpy f32 with every product
    rounded before the add: bit for bit."""
    rng = np.random.default_rng(77)
    rewards = rr.log32(rng.uniform(1e-4, 1.0, size=(16, 10000)).astype(np.float32))
    assert np.array_equal(_bits(rr.returns_torch(rewards, gamma)), _bits(rr.returns_numpy(rewards, gamma)))


@pytest.mark.parametrize("T", rr.RETURNS_T)
def test_committed_gpu_inputs_tell_a_fused_multiply_add_apart(T):
    """On the inputs tests/test_gpu_rollout.py feeds the kernel, gamma = 0.99: the torch form equals the uncontracted numpy
    form bit for bit, and either way a compiler could contract the line — fma(gamma, returns[i+1], .) or
    fma(1 - gamma, r, .) — gives different bits in some row: a contracted kernel cannot pass the bit-for-bit test.  (With
    gamma = 0.5 both products are exact and contraction changes nothing: that gamma checks the operation order.)  -inf and
    NaN propagate as IEEE gives them."""
    rewards, values, _ = rr.returns_case(T)
    plain = rr.returns_torch(rewards, 0.99)
    assert np.array_equal(_bits(plain), _bits(rr.returns_numpy(rewards, 0.99)))
    for fused in ("carry", "reward"):
        other = rr.returns_numpy(rewards, 0.99, fused=fused)
        differ = int((_bits(other) != _bits(plain)).sum())
        print("T=%d fused=%s: %d of %d returns differ" % (T, fused, differ, plain.size))
        assert differ > 0
    assert np.isneginf(plain[: T // 2 + 1, 1]).all() and np.isfinite(plain[T // 2 + 1:, 1]).all()
    assert np.isfinite(np.delete(plain, 1, axis=1)).all()
    assert values[T // 2, 2] == 0 and np.isneginf(rr.log32(values)[T // 2, 2])


def test_stats_divide_the_half_sums_by_T():
    """sum_rewards[h] / T and nothing[h] / (T / 2) (Agent.hpp:347-350): T = 4, rewards 1, 2, 3, 5, actions 0, 3, 0, 0."""
    s = rr.stats_ref(np.array([1, 2, 3, 5], dtype=np.float32), np.array([0, 3, 0, 0]))
    assert s.shape == (1, 4) and s.dtype == np.float32
    assert s[0].tolist() == [0.75, 2.0, 0.5, 1.0]
    # sequential f32: 2^24 + 1 + 1 stays 2^24, whereas a pairwise sum would reach 2^24 + 2
    r = np.array([2.0 ** 24, 1, 1, 0, 0, 0], dtype=np.float32)
    assert rr.stats_ref(r, np.zeros(6, dtype=np.int32))[0, 0] == np.float32(2.0 ** 24) / np.float32(6)


def test_bookkeeping_rules():
    """Two agents, T = 2, list_cap = 4: a restart in the middle starts the list again, a full buffer drops ticks and ignores
    restarts, a count above list_cap (and the marker) is stored as it came and counted, entries behind the count keep the
    sentinel, release clears."""
    ref = rr.RefRollout(2, 2, 4)
    rng = np.random.default_rng(0)

    def tick(t, counts, reset):
        keys = rng.integers(0, 1000, size=(2, 5)).astype(np.uint32)
        vals = rng.random((2, 5)).astype(np.float32)
        pov = rng.random((2, rr.HIDDEN)).astype(np.float32)
        probs = np.full((2, 9), 1 / 9, dtype=np.float32)
        one = np.full(2, 0.5, dtype=np.float32)
        ref.record(t, probs, one, np.array([t, t]), one, keys=keys, vals=vals, counts=np.array(counts, dtype=np.uint32), pov=pov, cap=5, disc=one,
                   imitate=np.array([1, 0], dtype=np.uint8), reset=reset)
        return keys

    k0 = tick(0, [1, 5], [0, 0])
    assert ref.fill().tolist() == [1, 1] and ref.missing_states == 1
    k1 = tick(1, [rr.MARKER, 2], [0, 1])  # agent 1 restarts: slot 0 again
    assert ref.fill().tolist() == [2, 1] and ref.missing_states == 2 and ref.tick_of(1, 0) == 1
    assert ref.image["counts"][1, 0] == rr.MARKER and np.array_equal(ref.image["keys"][1, 0], k1[0, :4])
    assert np.array_equal(ref.image["keys"][0, 1, :2], k1[1, :2]) and ref.image["counts"][0, 1] == 2
    assert np.array_equal(ref.image["keys"][0, 1, 2:], k0[1, 2:4])  # (tick 0 wrote four entries there, tick 1 two of them again)
    assert (ref.image["keys"][0, 0, 1:] == rr.SENTINEL).all() and ref.image["keys"][0, 0, 0] == k0[0, 0]
    tick(2, [0, 0], [1, 0])  # agent 0 is ready: dropped, its restart flag ignored
    assert ref.fill().tolist() == [2, 2] and ref.dropped == 1 and ref.ready().all()
    ref.release()
    assert ref.fill().tolist() == [0, 0]
    tick(3, [0, 0], None)
    ref.release(mask=[0, 1])
    assert ref.fill().tolist() == [1, 0]


def test_library_exports_the_rollout_entries():
    build.build(verbose=False)
    L = env.load_library()
    header = open(os.path.join(ROOT, "include", "strikeforce_policy.h")).read()
    declared = set(re.findall(r"\b(sf_rollout_[a-z_]+)\s*\(", header))
    assert declared == set(rollout.EXPORTS), declared ^ set(rollout.EXPORTS)
    for name in declared | {"sf_policy_update_actions"}:
        assert hasattr(L, name), name
    assert "sf_policy_update_actions" in policy.EXPORTS and hasattr(policy._NetBatch, "update_actions")
    assert C.sizeof(rollout.Buffers) == 10 * 8
    assert C.sizeof(rollout.Step) == 4 * 8 + 2 * 4 + 8 * 8 + 2 * 4  # four pointers, cap + agents, eight pointers, two ints


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_rollout_refuses_to_run_without_a_gpu():
    with pytest.raises(env.StrikeForceError, match=r"\(-2\).*no HIP device"):
        rollout.RolloutBatch(4, 4, 8)
    with pytest.raises(env.StrikeForceError, match=r"\(-1\).*T must be even"):
        rollout.RolloutBatch(4, 3, 8)
