"""sf_policy_load_weights on the device (include/strikeforce_policy.h; strikeforce_amd.policy._NetBatch.load_weights):
new parameters into a live policy or reward model, from device tensors, in stream order — and afterwards every image the
object derives from its parameters, and every output of every entry, is BIT FOR BIT what a fresh object created with those
parameters holds and computes.  Nothing here has a tolerance: the loaded object and the fresh one run the same kernels on
what must be the same bytes.  Parameter sets A and B are policy.init_parameters(71) and (72); observations are
tests/policy_cases.py's 1 % images."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import policy_cases as pc
from strikeforce_amd import env, policy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_NAMES = ("SF_POLICY_LAYERED", "SF_POLICY_FUSED_TAIL", "SF_POLICY_DENSE_CONV0", "SF_POLICY_F32_CONV")
SEED_A, SEED_B = 71, 72
CAP, TICKS = 2048, 3
KINDS = {"policy": (policy.PolicyBatch, policy.parameter_shapes), "reward": (policy.RewardBatch, policy.reward_parameter_shapes)}


def _host(seed):
    return policy.init_parameters(seed)


def _device(seed):
    t = {k: torch.from_numpy(v).cuda() for k, v in _host(seed).items()}
    torch.cuda.synchronize()
    return t


def _dev(a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    torch.cuda.synchronize()
    return t


def _bits(t):
    a = np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t)
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


def _memory(x, B):
    h, a = np.zeros((2, B, 160), dtype=np.float32), np.zeros((B, 9), dtype=np.float32)
    for b in range(B):
        h[:, b], a[b] = x.get_memory(b)
    return h, a


def _set_memory(x, h, a):
    for b in range(h.shape[1]):
        x.set_memory(b, h[:, b], a[b])


def _only(monkeypatch, **switches):
    for n in ENV_NAMES:
        if n != "SF_POLICY_LAYERED":  # (the cnn fixture's)
            monkeypatch.delenv(n, raising=False)
    for k, v in switches.items():
        monkeypatch.setenv(k, v)


class Ticks:
    """TICKS observations of B agents on the device, dense and as lists, and the actions a reward model is given."""

    def __init__(self, B, seed):
        rng = np.random.default_rng(seed)
        self.B = B
        self.obs, self.lists, self.act = [], [], []
        for _ in range(TICKS):
            o = pc.obs_sparse1(rng, B)
            self.obs.append(_dev(o))
            self.lists.append([_dev(x) for x in pc.lists_from_dense(o, CAP)])
            self.act.append(_dev(rng.integers(0, 9, size=B).astype(np.int32)))


def _run(kind, x, entry, ticks, out):
    """Issues TICKS evaluations of `entry` on x, tick t into out[t] (nothing synchronised)."""
    B = ticks.B
    for t in range(TICKS):
        o, li, act = ticks.obs[t], [v.data_ptr() for v in ticks.lists[t]], ticks.act[t]
        if kind == "policy":
            probs, value, cmd, action = out[t]
            if entry == "forward":
                x.forward(o.data_ptr(), B, probs.data_ptr(), value.data_ptr())
            elif entry == "forward_sparse":
                x.forward_sparse(li[0], li[1], li[2], li[3], CAP, B, probs.data_ptr(), value.data_ptr())
            else:
                x.predict_sparse(li[0], li[1], li[2], li[3], CAP, B, probs.data_ptr(), value.data_ptr(), cmd.data_ptr(), seed=9,
                                 d_action_ptr=action.data_ptr())
        else:
            d, r = out[t]
            if entry == "forward":
                x.forward(o.data_ptr(), act.data_ptr(), B, d.data_ptr(), r.data_ptr())
            else:
                x.reward_sparse(li[0], li[1], li[2], li[3], CAP, B, act.data_ptr(), d.data_ptr(), r.data_ptr())


def _outputs(kind, B):
    if kind == "policy":
        return [(torch.zeros((B, 9), device="cuda"), torch.zeros(B, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda"),
                 torch.zeros(B, dtype=torch.int32, device="cuda")) for _ in range(TICKS)]
    return [(torch.zeros(B, device="cuda"), torch.zeros(B, device="cuda")) for _ in range(TICKS)]


def _entries(kind, fused):
    if not fused:
        return ("forward",)  # (the list entries need the fused tail)
    return ("forward", "forward_sparse", "predict_sparse") if kind == "policy" else ("forward", "reward_sparse")


def _load_equals_create(kind, B, fused=True, random_start=True):
    cls = KINDS[kind][0]
    loaded, fresh = cls(_host(SEED_A), B), cls(_host(SEED_B), B)
    before = loaded.weights_digest()
    d_b = _device(SEED_B)
    loaded.load_weights(d_b)
    got, want = loaded.weights_digest(), fresh.weights_digest()
    assert len(got) == len(want) == len(before) and len(set(want)) > len(want) // 2
    assert got == want, [i for i in range(len(want)) if got[i] != want[i]]
    # (A and B differ in every image but the ones that hold no parameter of their own)
    assert sum(1 for a, b in zip(before, want) if a != b) >= len(want) - 2
    ticks = Ticks(B, 500 + B)
    h0, a0 = pc.random_memory(np.random.default_rng(B), B) if random_start else pc.fresh_memory(B)
    for entry in _entries(kind, fused):
        outs = []
        for x in (loaded, fresh):
            if random_start:
                _set_memory(x, h0, a0)
            else:
                x.reset_memory()
            out = _outputs(kind, B)
            _run(kind, x, entry, ticks, out)
            x.synchronize()
            outs.append(out)
        for t in range(TICKS):
            for u, v in zip(outs[0][t], outs[1][t]):
                assert np.array_equal(_bits(u), _bits(v)), (entry, t)
        last = outs[0][TICKS - 1][0].cpu().numpy()
        assert np.isfinite(last).all() and last.std() > 0 or B == 1
        rows = range(B) if B <= 65 else (0, 1, B // 2, B - 1)
        for b in rows:
            (hl, al), (hf, af) = loaded.get_memory(b), fresh.get_memory(b)
            assert np.array_equal(_bits(hl), _bits(hf)) and np.array_equal(al, af), (entry, b)
            assert not np.array_equal(hl, h0[:, b])  # (the state moved: something was evaluated)
    assert loaded.sparse_overflows() == 0 and fresh.sparse_overflows() == 0
    loaded.close(), fresh.close()
    del d_b


# ---- load equals create -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 17, 65])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_load_equals_create(cnn, monkeypatch, kind, B):
    """An object created with A and loaded with B: every digest equals a fresh B object's, and three consecutive ticks of
    every entry (a policy: forward, forward_sparse, predict_sparse; a reward model: forward, reward_sparse), started from
    the same running memory, give the same bits in every output and in the recurrent state."""
    _only(monkeypatch)
    _load_equals_create(kind, B)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_load_equals_create_with_the_separate_tail(cnn, monkeypatch, kind):
    """SF_POLICY_FUSED_TAIL=0: the forward reads gru_w_*, comb_w, res_w, head_w themselves, not k_tail's block."""
    _only(monkeypatch, SF_POLICY_FUSED_TAIL="0")
    _load_equals_create(kind, 17, fused=False)


def test_load_equals_create_with_the_f32_convolutions(monkeypatch):
    """SF_POLICY_F32_CONV=1, layered: conv1 and conv2 read the permuted f32 images whatever the row count."""
    _only(monkeypatch, SF_POLICY_LAYERED="1", SF_POLICY_F32_CONV="1")
    _load_equals_create("policy", 17)


def test_load_equals_create_where_the_split_images_reach_an_output(monkeypatch):
    """Layered, 335 agents: the smallest count at which conv2 takes the bf16-split kernel (335 * 49 = 16 415 >= 16 384 rows;
    conv1 takes it from 73), so conv_w3[1] and conv_w3[2] as the load rebuilt them decide every output."""
    _only(monkeypatch, SF_POLICY_LAYERED="1")
    _load_equals_create("policy", 335, random_start=False)


# ---- stream order -----------------------------------------------------------------------------------------------------------
def test_loads_take_effect_in_stream_order(cnn, monkeypatch):
    """forward (A) -> load B -> forward -> load A -> forward on a stream of its own, nothing synchronised in between, the
    source tensors alive until the one synchronise at the end: the three outputs and the final state equal, bit for bit, a
    fresh A object's tick, a fresh B object's tick from that state, and a fresh A object's tick from that one."""
    _only(monkeypatch)
    B = 17
    x, fa, fb = (policy.PolicyBatch(_host(s), B) for s in (SEED_A, SEED_A, SEED_B))
    d_a, d_b = _device(SEED_A), _device(SEED_B)
    ticks = Ticks(B, 77)
    out = [(torch.zeros((B, 9), device="cuda"), torch.zeros(B, device="cuda")) for _ in range(3)]
    ref = [(torch.zeros((B, 9), device="cuda"), torch.zeros(B, device="cuda")) for _ in range(3)]
    h0, a0 = pc.random_memory(np.random.default_rng(5), B)
    _set_memory(x, h0, a0), _set_memory(fa, h0, a0)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    x.set_stream(stream.cuda_stream)
    for t, params in enumerate((None, d_b, d_a)):
        if params is not None:
            x.load_weights(params)
        x.forward(ticks.obs[t].data_ptr(), B, out[t][0].data_ptr(), out[t][1].data_ptr())
    x.synchronize()
    objs = (fa, fb, fa)
    for t in range(3):
        if t:
            _set_memory(objs[t], *_memory(objs[t - 1], B))
        objs[t].forward(ticks.obs[t].data_ptr(), B, ref[t][0].data_ptr(), ref[t][1].data_ptr())
        objs[t].synchronize()
    for t in range(3):
        assert np.array_equal(_bits(out[t][0]), _bits(ref[t][0])) and np.array_equal(_bits(out[t][1]), _bits(ref[t][1])), t
    assert not np.array_equal(_bits(out[1][0]), _bits(out[0][0]))
    (hx, ax), (hr, ar) = _memory(x, B), _memory(fa, B)
    assert np.array_equal(_bits(hx), _bits(hr)) and np.array_equal(ax, ar)
    assert x.weights_digest() == fa.weights_digest()
    for o in (x, fa, fb):
        o.close()
    del d_a, d_b


# ---- state untouched --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_load_leaves_memory_counters_and_timers_alone(monkeypatch, kind):
    """Two objects do the same — one list forward with one agent whose list does not fit, timers armed, then distinct memory
    on agent 0 and on the last — and one of them is loaded with B: memory of every agent, the overflow count and the timed
    launch counts are what the other holds."""
    for n in ENV_NAMES:
        monkeypatch.delenv(n, raising=False)
    B = 6
    cls = KINDS[kind][0]
    x, twin = cls(_host(SEED_A), B), cls(_host(SEED_A), B)
    rng = np.random.default_rng(3)
    keys, vals, counts, pov = pc.lists_from_dense(pc.obs_sparse1(rng, B), CAP)
    counts[2] = CAP + 1
    li = [_dev(v) for v in (keys, vals, counts, pov)]
    act = _dev(np.arange(B, dtype=np.int32))
    o1, o2 = torch.zeros((B, 9), device="cuda"), torch.zeros(B, device="cuda")
    h, a = pc.random_memory(rng, B)
    d_b = _device(SEED_B)
    for o in (x, twin):
        o.kernel_time_by_kernel(True)
        if kind == "policy":
            o.forward_sparse(li[0].data_ptr(), li[1].data_ptr(), li[2].data_ptr(), li[3].data_ptr(), CAP, B, o1.data_ptr(), o2.data_ptr())
        else:
            o.reward_sparse(li[0].data_ptr(), li[1].data_ptr(), li[2].data_ptr(), li[3].data_ptr(), CAP, B, act.data_ptr(), o2.data_ptr(), None)
        o.set_memory(0, h[:, 0], a[0]), o.set_memory(B - 1, h[:, B - 1], a[B - 1])
    x.load_weights(d_b)
    x.synchronize()
    (hx, ax), (ht, at) = _memory(x, B), _memory(twin, B)
    assert np.array_equal(_bits(hx), _bits(ht)) and np.array_equal(_bits(ax), _bits(at))
    assert np.array_equal(_bits(hx[:, 0]), _bits(h[:, 0])) and np.array_equal(_bits(hx[:, B - 1]), _bits(h[:, B - 1]))
    assert x.sparse_overflows() == twin.sparse_overflows() == 1
    nx, nt = ([n for (_, _, n) in o.kernel_time_by_kernel(False)] for o in (x, twin))
    assert nx == nt == [0, 0, 1, 1]
    x.close(), twin.close()
    del d_b


# ---- unaligned sources, and the accepting side of the pointer guard ------------------------------------------------------------
def _carved(seed, shapes, lead):
    """Every parameter at an odd float offset inside ONE flat device tensor, the first `lead` floats in."""
    host = _host(seed)
    total = lead + sum(int(np.prod(s)) + 2 for s in shapes.values()) + lead
    flat = torch.full((total,), float("nan"), device="cuda")
    t, at = {}, lead | 1
    for name, s in shapes.items():
        n = int(np.prod(s))
        view = flat[at:at + n].view(*s)
        view.copy_(torch.from_numpy(host[name]))
        t[name] = view
        at += n + (1 if n % 2 else 2)  # (odd again)
    torch.cuda.synchronize()
    return flat, t


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_sources_carved_at_odd_offsets_out_of_the_middle_of_one_tensor(cnn, monkeypatch, kind):
    """All parameters as views at odd float offsets (4-byte aligned, nothing more) into one flat tensor, 1 M floats into a
    larger allocation: accepted — every extent lies inside it — and the digests equal those of separate tensors and of a
    fresh object."""
    _only(monkeypatch)
    cls, shapes = KINDS[kind][0], KINDS[kind][1]()
    x, y, fresh = cls(_host(SEED_A), 2), cls(_host(SEED_A), 2), cls(_host(SEED_B), 2)
    flat, views = _carved(SEED_B, shapes, 1 << 20)
    assert all(v.data_ptr() % 8 == 4 for v in views.values()) and all(v.is_contiguous() for v in views.values())
    assert min(v.data_ptr() for v in views.values()) >= flat.data_ptr() + (4 << 20)
    d_b = _device(SEED_B)
    x.load_weights(views), y.load_weights(d_b)
    want = fresh.weights_digest()
    assert x.weights_digest() == want and y.weights_digest() == want
    for o in (x, y, fresh):
        o.close()
    del flat, views, d_b


# ---- repeat -----------------------------------------------------------------------------------------------------------------
def test_repeated_loads_allocate_nothing_after_the_first(cnn, monkeypatch):
    """Load B twice, then A: the digests are create(B)'s, then create(A)'s — the object's own before any load — and the
    second and third load leave the device's free memory where the first left it."""
    _only(monkeypatch)
    x, fb = policy.PolicyBatch(_host(SEED_A), 4), policy.PolicyBatch(_host(SEED_B), 4)
    d_a, d_b = _device(SEED_A), _device(SEED_B)
    own, want_b = x.weights_digest(), fb.weights_digest()  # (the hook's own buffer exists from here on)
    free = []
    for params in (d_b, d_b, d_a):
        x.load_weights(params)
        x.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
        if params is d_b:
            assert x.weights_digest() == want_b
    assert x.weights_digest() == own and own != want_b
    print("free bytes after each load:", free)
    assert free[0] == free[1] == free[2]
    x.close(), fb.close()
    del d_a, d_b


# ---- misuse that host logic decides before any launch ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_misuse_is_refused_before_any_launch(monkeypatch, kind):
    """NULL object, abi_version off by one, a NULL field this kind needs: SF_ERR_ARG each, the digests as before.  A reward
    model with every policy_* field NULL is accepted."""
    for n in ENV_NAMES:
        monkeypatch.delenv(n, raising=False)
    cls, shapes = KINDS[kind][0], KINDS[kind][1]()
    x = cls(_host(SEED_A), 3)
    L = x.L
    d_b = _device(SEED_B)
    before = x.weights_digest()

    def call(change, handle=x.h):
        w, _ = policy.device_weights(d_b, shapes)
        change(w)
        return L.sf_policy_load_weights(handle, C.byref(w))

    assert call(lambda w: None, handle=None) == -1
    assert call(lambda w: setattr(w, "abi_version", policy.POLICY_ABI_VERSION + 1)) == -1
    assert b"abi_version" in L.sf_last_error()
    needed = ["comb_b", "value_w", "value_b"] + ([] if kind == "reward" else ["policy_w", "policy_b"])
    for field in needed:
        assert call(lambda w: setattr(w, field, None)) == -1, field
        assert b"is null" in L.sf_last_error()
    for field, i in [("conv_w", 0), ("conv_w", 3), ("gru_b_hh", 1), ("value_res_w", 2)] + ([] if kind == "reward" else [("policy_res_b", 0)]):
        def drop(w, field=field, i=i):
            getattr(w, field)[i] = None
        assert call(drop) == -1, (field, i)
    x.synchronize()
    assert x.weights_digest() == before
    if kind == "reward":
        w, _ = policy.device_weights(d_b, shapes)
        assert not w.policy_w and not w.policy_b and not any(w.policy_res_w[i] or w.policy_res_b[i] for i in range(3))
    assert call(lambda w: None) == 0  # the unspoilt struct: accepted
    fresh = cls(_host(SEED_B), 3)
    assert x.weights_digest() == fresh.weights_digest() != before
    with pytest.raises(ValueError, match="missing parameter"):
        x.load_weights({k: v for k, v in d_b.items() if k != "value.1.bias"})
    x.close(), fresh.close()
    del d_b


# ---- the example ------------------------------------------------------------------------------------------------------------
def _example(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_rollout.py")] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().splitlines()


FIRST_LINE = (r"^64 arenas x 48 steps, T = 8: [\d.]+ M agent-steps/s without record, [\d.]+ M with; \d+ buffers handed over, \d+ ticks dropped, "
              r"\d+ states whose list did not fit 512 entries$")


def test_example_swaps_parameters_at_the_hand_overs():
    lines = _example("64", "48", "8", "--swap")
    assert re.match(FIRST_LINE, lines[0]), lines
    swap = [ln for ln in lines if ln.startswith("--swap:")]
    assert len(swap) == 1, lines
    m = re.match(r"^--swap: (\d+) loads of both networks' parameters .* ([\d.]+) M agent-steps/s$", swap[0])
    assert m and int(m.group(1)) >= 1 and float(m.group(2)) > 0, swap


def test_example_without_the_flag_prints_what_it_printed_before():
    lines = _example("64", "48", "8")
    assert re.match(FIRST_LINE, lines[0]), lines
    assert len(lines) <= 2 and not any("swap" in ln or "load" in ln for ln in lines), lines
    if len(lines) == 2:
        assert lines[1].startswith("last hand-over: r_avg0 "), lines
