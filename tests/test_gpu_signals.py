"""sf_signals_* on the MI355X (k_signals) through the C-ABI, against the restatement over the oracle (tests/signals_ref.py), bit
for bit: no tolerance anywhere.

Every case of tests/signals_cases.py runs through signals_cases.Checker: after each call the vitals, the delta, the reward's
bits and the status equal the restatement's; the vitals equal sf_dump_arena's own fields; each output is produced again with
the two others NULL (on a signals object of its own, so that its baseline sees the same history); the output buffers are
sentinel-filled with a guard word behind them; the state digests of all arenas are unchanged by the call; a second call
without a step gives all-zero deltas.  d_rebase is NULL or all zero in turn where nothing is announced, and where something
is, the set bytes are 0x80 / 0xFF / 2 in turn (the rule is `!= 0`).  Then the refusals, and the call captured in a graph
behind sf_step_device and replayed twice."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import signals_cases as sc
from oracle_lib import ArenaDump
from reset_sel_ref import ResetSelRef
from signals_ref import SignalsRef
from strikeforce_amd import abi, config, env

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SF_ERR_ARG, SF_ERR_STATE = -1, -4


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class GpuSignals:
    def __init__(self, g):
        self.g, self.s = g, g.signals()

    def step(self, rebase, weights, outs):
        A, n = self.g.cfg.arenas, self.g.cfg.n_agents
        host = sc.out_buffers(A, n, outs)
        d = [None if x is None else dev(x) for x in host]
        rb = None if rebase is None else dev(np.zeros((A, n), dtype=np.uint8) if isinstance(rebase, str) else rebase)
        self.s.step(d[0], d[1], d[2], rb, weights)
        back = [None if x is None else x.cpu().numpy() for x in d]
        return sc.take_buffers(A, n, back[0], back[1], back[2], "device")

    def status(self):
        return self.s.status()

    def close(self):
        self.s.close()


class Gpu(env.ArenaBatch):
    """ArenaBatch with the engine surface of tests/signals_cases.py."""

    snap = None

    def dump(self, a):
        return ArenaDump(*self.dump_raw(a))

    def reset(self, tb, sr):
        A = self.cfg.arenas
        env.ArenaBatch.reset(self, (C.c_uint64 * A)(*tb), (C.c_uint64 * A)(*sr))

    def step_many(self, rows):
        d = dev(rows)
        self.step_device(d.data_ptr(), len(rows))
        self.synchronize()

    def new_signals(self):
        return GpuSignals(self)

    def reset_arenas(self, mask=None, done_too=False, max_steps=0, tb=None, serial=None):
        A, n = self.cfg.arenas, self.cfg.n_agents
        selected = dev(np.full((A, n), 0xA5, dtype=np.uint8))
        m = None if mask is None else dev(np.asarray(mask, dtype=np.uint8))
        t = None if tb is None else dev(np.array(tb, dtype=np.uint64).view(np.int64))
        s = None if serial is None else dev(np.array(serial, dtype=np.uint64).view(np.int64))
        env.ArenaBatch.reset_arenas(self, None if m is None else m.data_ptr(), 1, done_too, max_steps, None if t is None else t.data_ptr(),
                                    None if s is None else s.data_ptr(), selected.data_ptr())
        return selected.cpu().numpy()

    def _snap(self):
        if self.snap is None:
            self.snap = self.snapshot(3)
        return self.snap

    def save(self, slots):
        self._snap().save(np.asarray(slots, dtype=np.int32))

    def load(self, slots):
        self._snap().load(np.asarray(slots, dtype=np.int32))

    def close(self):
        if self.snap is not None:
            self.snap.close()
            self.snap = None
        env.ArenaBatch.close(self)


@pytest.mark.parametrize("name", sc.NAMES)
def test_device_signals_equal_the_restatement(name):
    c = sc.case(name)
    g = Gpu(c.w)
    check = sc.Checker(g, name)
    try:
        sref = sc.run(c, g, check)
        assert check.calls == sum(op[0] == "signals" for op in c.script) and sref.reach
    finally:
        check.close()
        g.close()


def test_python_surface_and_decode():
    c = sc.case("battle3")
    g = Gpu(c.w)
    g.reset(c.script[0][1], c.script[0][2])
    A, n = c.w.cfg.arenas, c.w.cfg.n_agents
    s = g.signals()
    v = torch.zeros((A, n, abi.VITALS_WORDS), dtype=torch.int32, device="cuda")
    d = torch.zeros((A, n, abi.DELTA_WORDS), dtype=torch.int32, device="cuda")
    r = torch.full((A * n,), 5.0, dtype=torch.float32, device="cuda")
    s.step(vitals_ptr=v, delta_ptr=d, reward_ptr=r, weights=env.reward_weights(per_step=1.0))
    x = env.decode_signals(v.cpu().numpy(), d.cpu().numpy())
    assert x["rebased"].all() and x["present"].all() and not x["ended"].any() and (x["hp"] > 0).all() and not r.cpu().numpy().any()
    row = np.full((A, n), ord("+"), dtype=np.uint8)
    row[0, 1] = ord("_")
    g.step(row)
    s.step(v.data_ptr(), d.data_ptr(), r.data_ptr(), None, env.reward_weights(per_step=1.0, died=-2.0))
    x = env.decode_signals(delta=d.cpu().numpy())
    assert x["died"].tolist() == [[False, True, False]] + [[False] * 3] * (A - 1) and (x["flags"][0, 1] == env.SIG_DIED)
    assert r.cpu().numpy().reshape(A, n)[0].tolist() == [1.0, -1.0, 1.0] and x["d_hp"][0, 1] < 0
    assert s.status() == (0, 0)
    s.close(), s.close(), g.close()


def test_refusals_by_state_and_argument():
    c = sc.case("solo-restarts-still")
    g, other = Gpu(c.w), Gpu(sc.case("solo-restarts-still").w)
    L, A = g.L, c.w.cfg.arenas
    h = C.c_void_p()
    assert L.sf_signals_create(None, C.byref(h)) == SF_ERR_ARG and L.sf_signals_create(g.h, None) == SF_ERR_ARG
    assert L.sf_signals_status(None, None) == SF_ERR_ARG and L.sf_signals_destroy(None) == 0
    s = g.signals()
    d = torch.zeros((A, 1, abi.DELTA_WORDS), dtype=torch.int32, device="cuda")
    io = abi.SignalsIO(None, d.data_ptr(), None, None, abi.RewardWeights())
    call = lambda e, sig, i: L.sf_signals_step(e, sig, i)
    assert call(g.h, s.h, C.byref(io)) == SF_ERR_STATE  # before the first sf_reset
    g.reset(c.script[0][1], c.script[0][2]), other.reset(c.script[0][1], c.script[0][2])
    assert call(None, s.h, C.byref(io)) == SF_ERR_ARG and call(g.h, None, C.byref(io)) == SF_ERR_ARG
    assert call(g.h, s.h, None) == SF_ERR_ARG and L.sf_signals_status(s.h, None) == SF_ERR_ARG
    assert call(other.h, s.h, C.byref(io)) == SF_ERR_STATE and b"another environment" in L.sf_last_error()
    g.step_begin()
    assert call(g.h, s.h, C.byref(io)) == SF_ERR_STATE and b"between sf_step_begin" in L.sf_last_error()
    g.step_end(np.full((A, 1), ord("+"), dtype=np.uint8))
    g.synchronize()
    assert not d.cpu().numpy().any()  # nothing was launched by any of them ...
    assert call(g.h, s.h, C.byref(io)) == 0
    assert (d.cpu().numpy()[:, :, 0] & abi.SIG_REBASED).all()  # ... and the baseline was still unset
    s.close(), g.close(), other.close()


def _hip():
    lib = sorted(glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so*")))
    H = C.CDLL(lib[0] if lib else "libamdhip64.so")
    H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    H.hipFree.argtypes = [C.c_void_p]
    H.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    return H


def test_host_pointers_misaligned_and_short_buffers_are_refused_before_any_launch():
    c = sc.case("battle3")
    g = Gpu(c.w)
    g.reset(c.script[0][1], c.script[0][2])
    L, A, n = g.L, c.w.cfg.arenas, c.w.cfg.n_agents
    s = g.signals()
    before = g.digest()
    H, bufs = _hip(), []

    def alloc(nbytes):  # (allocations of their own: the extent check is made against the runtime's allocation)
        p = C.c_void_p()
        assert H.hipMalloc(C.byref(p), nbytes) == 0 and H.hipMemset(p, 0, nbytes) == 0
        bufs.append(p)
        return p.value

    sizes = {"d_vitals": 4 * abi.VITALS_WORDS * A * n, "d_delta": 4 * abi.DELTA_WORDS * A * n, "d_reward": 4 * A * n, "d_rebase": A * n}
    host = np.zeros(4 * abi.VITALS_WORDS * A * n + 64, dtype=np.uint8)
    exact = {}
    for field, nbytes in sizes.items():
        unit = 1 if field == "d_rebase" else 4
        exact[field], short, big = alloc(nbytes), alloc(nbytes - unit), alloc(nbytes + 64)

        def call(p):
            io = abi.SignalsIO(None, None, None, None, abi.RewardWeights())
            setattr(io, field, p)
            return L.sf_signals_step(g.h, s.h, C.byref(io))

        assert call(host.ctypes.data) == SF_ERR_ARG and b"not device memory" in L.sf_last_error(), field
        assert field.encode() in L.sf_last_error() and b"sf_signals_step" in L.sf_last_error()
        assert call(short) == SF_ERR_ARG and b"past the end" in L.sf_last_error(), field  # one element short
        assert call(big + 64 + unit) == SF_ERR_ARG and b"past the end" in L.sf_last_error(), field  # starts too late
        if unit == 4:
            assert call(big + 2) == SF_ERR_ARG and b"aligned" in L.sf_last_error(), field
    torch.cuda.synchronize()
    # the exact extents, each ending on its allocation's last byte; no refused call had launched: this is the first one
    io = abi.SignalsIO(exact["d_vitals"], exact["d_delta"], exact["d_reward"], exact["d_rebase"], abi.RewardWeights())
    assert L.sf_signals_step(g.h, s.h, C.byref(io)) == 0
    d = torch.zeros((A, n, abi.DELTA_WORDS), dtype=torch.int32, device="cuda")
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    g.synchronize()
    assert H.hipMemcpy(d.data_ptr(), exact["d_delta"], sizes["d_delta"], 3) == 0
    assert (d.cpu().numpy()[:, :, 0] & abi.SIG_REBASED).all()
    tail = torch.zeros(A * n + 3, dtype=torch.uint8, device="cuda")  # d_rebase needs no alignment: an odd address is taken
    s.step(delta_ptr=d, rebase_ptr=tail.data_ptr() + 3)
    assert not (d.cpu().numpy()[:, :, 0] & abi.SIG_REBASED).any()
    assert (g.digest() == before).all() and s.status() == (0, 0)
    s.close(), g.close()
    for p in bufs:
        H.hipFree(p)


def test_captured_behind_a_step_launch_and_replayed_twice():
    """The loop a training run captures: k steps and the signals of that launch, no host synchronisation in between."""
    c = sc.case("battle16")
    w, k = c.w, 4
    A, n = w.cfg.arenas, w.cfg.n_agents
    tb, sr = c.script[0][1], c.script[0][2]
    g = Gpu(w)
    stream = torch.cuda.Stream()
    g.set_stream(stream.cuda_stream)
    g.reset(tb, sr)
    src = ResetSelRef(w, tb, sr)
    ref = SignalsRef(src)
    wts = sc.weights()
    rows = config.bench_commands(A, n, k, seed0=99)[0].reshape(k, A, n)
    cmds = dev(rows)
    v = torch.zeros((A, n, abi.VITALS_WORDS), dtype=torch.int32, device="cuda")
    d = torch.zeros((A, n, abi.DELTA_WORDS), dtype=torch.int32, device="cuda")
    r = torch.zeros((A * n,), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = g.signals()
    try:
        s.step(v, d, r, None, wts)  # the first call sets the baseline, outside the graph
        g.synchronize()
        sc.compare("before the capture", (v.cpu().numpy(), d.cpu().numpy(), r.cpu().numpy().reshape(A, n), s.status()),
                   ref.step(None, wts) + (ref.status(),))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            g.step_device(cmds.data_ptr(), k)
            s.step(v, d, r, None, wts)
        torch.cuda.synchronize()
        assert (g.digest() == src.digest()).all()  # (capture launched nothing)
        for i in range(2):
            with torch.cuda.stream(stream):
                graph.replay()
            stream.synchronize()
            for row in rows:
                src.step(row)
            want = ref.step(None, wts) + (ref.status(),)
            sc.compare("replay %d" % i, (v.cpu().numpy(), d.cpu().numpy(), r.cpu().numpy().reshape(A, n), s.status()), want)
            assert (g.digest() == src.digest()).all()
    finally:
        s.close(), g.close(), src.close()
