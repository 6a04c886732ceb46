"""tests/rollout_gae_ref.py on the CPU: the recursion against a hand-derived vector, against rollout_ref.py's returns in the
reference configuration bit for bit, against textbook GAE in float64 within a bound computed from the inputs; the committed
GPU inputs telling a fused multiply-add at any product apart; the continuing bookkeeping's rules; the ABI surface of
sf_rollout_continue / sf_rollout_gae and the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rollout_gae_ref as gr
import rollout_ref as rr
from strikeforce_amd import build, env, rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def test_hand_derived_gae():
    """T = 4, gamma = lambda = 0.5, rewards 1 2 3 4, values 8 4 2 6, next value 16, a game end at first[2]:
    G3 = 0.5 * 16 + 4 = 12;  G2 = 0.5 * (0.5 * 6 + 0.5 * 12) + 3 = 7.5;  G1 = 2 (its game ended behind it);
    G0 = 0.5 * (0.5 * 4 + 0.5 * 2) + 1 = 2.5.  The delta form: d3 = 4 + 8 - 6 = 6, A3 = 6; d2 = 3 + 3 - 2 = 4, A2 = 4 + 0.25 * 6
    = 5.5; d1 = 2 - 4 = -2, A1 = -2; d0 = 1 + 2 - 8 = -5, A0 = -5 + 0.25 * -2 = -5.5."""
    r, v = np.array([1, 2, 3, 4], dtype=np.float32), np.array([8, 4, 2, 6], dtype=np.float32)
    first = np.array([0, 0, 1, 0], dtype=np.uint8)
    nv = np.array([16], dtype=np.float32)
    G, V, A = gr.gae_numpy(r, v, first, 0.5, 0.5, next_value=nv)
    assert G.tolist() == [2.5, 2.0, 7.5, 12.0] and V.tolist() == v.tolist() and A.tolist() == [-5.5, -2.0, 5.5, 6.0]
    G64, _, A64 = gr.gae_delta_f64(r, v, first, 0.5, 0.5, next_value=nv)
    assert G64.tolist() == G.tolist() and A64.tolist() == A.tolist()
    # the next tick's flag, or no next value, leaves the last slot its reward alone; first[0] cuts nothing
    for kw in (dict(next_value=nv, next_end=np.array([1])), dict()):
        assert gr.gae_numpy(r, v, first, 0.5, 0.5, **kw)[0].tolist() == [2.5, 2.0, 0.5 * (0.5 * 6 + 0.5 * 4) + 3, 4.0]
    again = gr.gae_numpy(r, v, np.array([1, 0, 1, 0], dtype=np.uint8), 0.5, 0.5, next_value=nv)
    assert again[0].tolist() == G.tolist()
    # lambda = 0: one-step returns; lambda = 1: discounted sums up to the game end
    assert gr.gae_numpy(r, v, first, 0.5, 0.0, next_value=nv)[0].tolist() == [1 + 2, 2.0, 3 + 3, 4 + 8]
    assert gr.gae_numpy(r, v, first, 0.5, 1.0, next_value=nv)[0].tolist() == [1 + 1, 2.0, 3 + 0.5 * 12, 12.0]


@pytest.mark.parametrize("gamma", rr.RETURNS_GAMMAS)
def test_reference_configuration_equals_the_returns_restatement(gamma):
    """10^4 random buffers (T = 16; rewards = log of a random D, one of them -inf; values in (0, 1), one of them 0):
    lambda = 1, log_values, reward_scale = 1.f - gamma, no next value, no game end -> rollout_ref's returns, log V and their
    f32 difference, bit for bit (NaNs as NaNs)."""
    rng = np.random.default_rng(78)
    rewards = rr.log32(rng.uniform(1e-4, 1.0, size=(16, 10000)).astype(np.float32))
    values = rng.uniform(1e-4, 1.0, size=(16, 10000)).astype(np.float32)
    rewards[7, 5] = -np.inf
    values[7, 6] = values[7, 5] = 0.0
    scale = np.float32(1) - np.float32(gamma)
    G, V, A = gr.gae_numpy(rewards, values, None, gamma, 1.0, reward_scale=scale, log_values=True)
    want = rr.returns_torch(rewards, gamma)
    logv = rr.log32(values)
    with np.errstate(invalid="ignore"):
        diff = want - logv
    assert _same(G, want).all() and np.array_equal(_bits(V), _bits(logv)) and _same(A, diff).all()
    assert np.isneginf(G[:8, 5]).all() and np.isnan(A[7, 5]) and A[7, 6] == np.inf
    # all-zero flags are no flags
    zero = np.zeros((16, 10000), dtype=np.uint8)
    assert _same(gr.gae_numpy(rewards, values, zero, gamma, 1.0, reward_scale=scale, log_values=True, next_end=zero[0])[0], want).all()


@pytest.mark.parametrize("lam", [0.0, 0.5, 0.95, 1.0])
@pytest.mark.parametrize("gamma", [0.5, 0.99])
@pytest.mark.parametrize("bootstrap", [False, True])
def test_f32_recursion_against_textbook_gae_in_float64(gamma, lam, bootstrap):
    """Finite inputs in [-4, 4], T = 64, 500 agents, one game end in eight slots: the f32 recursion lies within the bound
    rollout_gae_ref.gae_error_bound derives from the inputs (half an ulp per rounded operation, propagated) of the float64
    delta form, plus the float64 form's own rounding (six operations per slot at 2^-53 of magnitudes below 4 * T)."""
    T, n = 64, 500
    rng = np.random.default_rng(int(gamma * 100) * 7 + int(lam * 100))
    r = rng.uniform(-4, 4, size=(T, n)).astype(np.float32)
    v = rng.uniform(-4, 4, size=(T, n)).astype(np.float32)
    first = (rng.random((T, n)) < 0.125).astype(np.uint8)
    kw = dict(next_value=rng.uniform(-4, 4, size=n).astype(np.float32), next_end=(rng.random(n) < 0.3).astype(np.uint8)) if bootstrap else {}
    G, V, A = gr.gae_numpy(r, v, first, gamma, lam, reward_scale=0.3, **kw)
    G64, V64, A64 = gr.gae_delta_f64(r, v, first, gamma, lam, reward_scale=0.3, **kw)
    eg, ea = gr.gae_error_bound(r, v, first, gamma, lam, reward_scale=0.3, **kw)
    own = 6 * T * 2.0 ** -53 * 4 * T
    dg, da = np.abs(G.astype(np.float64) - G64), np.abs(A.astype(np.float64) - A64)
    print("gamma %s lambda %s: returns off by at most %.3g (bound there %.3g), advantages %.3g (%.3g); largest bound %.3g"
          % (gamma, lam, dg.max(), eg.flat[dg.argmax()], da.max(), ea.flat[da.argmax()], eg.max()))
    assert np.array_equal(V, v) and np.array_equal(V64, v.astype(np.float64))
    assert (dg <= eg + own).all() and (da <= ea + own).all()
    assert eg.max() < 1e-4  # (the bound is tight enough to mean something: a few dozen ulps of magnitudes below 100)
    assert first[1:].any() and dg.max() > 0


@pytest.mark.parametrize("T", gr.GAE_T)
def test_committed_gpu_inputs_tell_a_fused_multiply_add_apart(T):
    """tests/test_gpu_rollout_gae.py's inputs, gamma = 0.99, lambda = 0.95, reward_scale = 1.f - gamma, next values given: a
    fused multiply-add at any of the recursion's four products — gamma * boot, reward_scale * reward, (1 - lambda) * V,
    lambda * G — changes bits somewhere, so a contracted kernel cannot pass the bit-for-bit test.  A reward of -inf and a
    log of 0 next to a game end stay on their side of it, and nothing is NaN."""
    rewards, values, _, first, nxt, nv = gr.gae_case(T)
    scale = np.float32(1) - np.float32(0.99)
    for log_values in (False, True):
        kw = dict(reward_scale=scale, log_values=log_values, next_value=nv, next_end=nxt)
        plain = gr.gae_numpy(rewards, values, first, 0.99, 0.95, **kw)[0]
        for site in gr.FUSED_SITES:
            other = gr.gae_numpy(rewards, values, first, 0.99, 0.95, fused=site, **kw)[0]
            differ = int((~_same(other, plain)).sum())
            print("T=%d log_values=%d fused at %s: %d of %d returns differ" % (T, log_values, site, differ, plain.size))
            assert differ > 0, site
    for lam in gr.GAE_LAMBDAS:
        G, V, A = gr.gae_numpy(rewards, values, first, 0.99, lam, reward_scale=scale, log_values=True, next_value=nv, next_end=nxt)
        assert first[T // 2, 2] and first[T // 2, 10]
        assert np.isneginf(G[T // 2, 2]) and np.isfinite(G[: T // 2, 2]).all()  # the -inf reward stays in its own game
        assert np.isneginf(V[T // 2, 10]) and np.isfinite(G[: T // 2, 10]).all() and A[T // 2, 10] == np.inf
        assert not np.isnan(G).any() and not np.isnan(A).any()


def test_continuing_bookkeeping_rules():
    """Two agents, T = 2, no states: a restart flag is stored and never rewinds; a full buffer drops ticks and stores no
    flag; release clears; without flags first is 0."""
    ref = gr.RefRolloutCont(2, 2, 4, store_states=False, store_disc=False, store_imitate=False)
    probs, one = np.full((2, 9), 1 / 9, dtype=np.float32), np.full(2, 0.5, dtype=np.float32)
    tick = lambda t, reset: ref.record(t, probs, one, np.array([t, t]), one, reset=reset)
    tick(0, [0, 1])
    assert ref.fill().tolist() == [1, 1] and ref.first_of(0) == [0] and ref.first_of(1) == [1]
    tick(1, [1, 1])
    assert ref.fill().tolist() == [2, 2] and ref.first_of(0) == [0, 1] and ref.first_of(1) == [1, 1] and ref.ready().all()
    tick(2, [1, 0])
    assert ref.dropped == 2 and ref.first_of(0) == [0, 1] and ref.tick_of(0, 1) == 1
    ref.release(mask=[1, 0])
    tick(3, None)
    assert ref.fill().tolist() == [1, 2] and ref.first_of(0) == [0] and ref.tick_of(0, 0) == 3 and ref.dropped == 3
    assert ref.image["first"][1, 0] == 1  # (what an earlier block left there stays until it is overwritten)


def test_header_declares_the_two_entries_and_the_struct_matches():
    header = open(os.path.join(ROOT, "include", "strikeforce_policy.h")).read()
    assert re.search(r"int sf_rollout_continue\(sf_rollout \*r, uint8_t \*d_first\);", header)
    assert re.search(r"int sf_rollout_gae\(sf_rollout \*r, const sf_rollout_gae_io \*io\);", header)
    assert re.search(r"#define SF_POLICY_ABI_VERSION 1\b", header)
    assert {"sf_rollout_continue", "sf_rollout_gae"} <= set(rollout.EXPORTS)
    body = re.search(r"typedef struct sf_rollout_gae_io \{(.*?)\} sf_rollout_gae_io;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        names += [n.strip(" *\n") for n in re.sub(r"^\s*(const\s+)?\w+\s", "", decl.strip()).split(",") if n.strip()]
    mine = {"lam": "lambda"}
    assert [mine.get(n, n) for n, _ in rollout.GaeIO._fields_] == names, names
    assert C.sizeof(rollout.GaeIO) == 4 * 4 + 3 * 8 + 2 * 4 + 3 * 8  # three floats + an int, three pointers, two ints, three pointers
    assert rollout.GaeIO.d_next_value.offset == 16 and rollout.GaeIO.d_returns.offset == 48
    sig = __import__("inspect").signature(rollout.RolloutBatch.gae)
    assert list(sig.parameters) == ["self", "gamma", "lam", "reward_scale", "log_values", "next_value", "next_mask", "next_words", "out"]
    assert "continuing" in __import__("inspect").signature(rollout.RolloutBatch.__init__).parameters


def test_null_handles_are_refused_without_a_device():
    build.build(verbose=False)
    L = env.load_library()
    rollout._bind(L)
    assert hasattr(L, "sf_rollout_continue") and hasattr(L, "sf_rollout_gae")
    assert L.sf_policy_abi_version() == 1
    io = rollout.GaeIO()
    io.gamma, io.lam, io.reward_scale = 0.99, 0.95, 1.0
    assert L.sf_rollout_gae(None, C.byref(io)) == -1 and b"null rollout" in L.sf_last_error()
    assert L.sf_rollout_continue(None, None) == -1 and b"null rollout" in L.sf_last_error()
