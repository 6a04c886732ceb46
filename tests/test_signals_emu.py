"""sf_signals_step on the CPU: the product's host code (Env::signals_*, sf_host.hpp) and the kernel's per-agent body
(sf_signals.hpp signals_agent — the text k_signals compiles) over tests/emu's runtime, against the restatement over the
oracle (tests/signals_ref.py), bit for bit: vitals, delta, reward bits and status after every call of every case of
tests/signals_cases.py, each output again with the others NULL, sentinel-filled buffers with guard words, digests unchanged.
The host's refusals, and that a refused call launches nothing.  A stand-alone program (tests/emu/signals_main.cpp)
runs the body over the emulator's states of two whole cases under AddressSanitizer and UBSan; nothing sanitized is loaded
into Python.

The emulator's runtime (tests/emu/sf_emu.cpp) has the launches; here device pointers are host memory.  The pointer checks
of the HIP runtime, stream order and graph capture are covered on the device (tests/test_gpu_signals.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import emu_lib
import signals_cases as sc
from strikeforce_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SF_ERR_ARG, SF_ERR_STATE = -1, -4


class EmuSignals:
    def __init__(self, e):
        self.e, self.L = e, e.L
        self.h = C.c_void_p()
        assert self.L.sfe_signals_create(e.h, C.byref(self.h)) == 0, self.L.sfe_last_error().decode()

    def step_rc(self, io, env=None):
        return self.L.sfe_signals_step((env or self.e).h, self.h, C.byref(io))

    def step(self, rebase, weights, outs):
        A, n = self.e.cfg.arenas, self.e.cfg.n_agents
        v, d, r = sc.out_buffers(A, n, outs)
        rb = np.zeros((A, n), dtype=np.uint8) if isinstance(rebase, str) else rebase
        io = abi.SignalsIO(*[None if x is None else x.ctypes.data for x in (v, d, r, rb)], weights)
        assert self.step_rc(io) == 0, self.L.sfe_last_error().decode()
        return sc.take_buffers(A, n, v, d, r, "emu")

    def status(self):
        out = (C.c_int64 * 4)()
        assert self.L.sfe_signals_status(self.h, C.byref(out)) == 0
        assert out[2] == 0 and out[3] == 0
        return out[0], out[1]

    def close(self):
        if self.h:
            self.L.sfe_signals_destroy(self.h)
            self.h = None


class EmuSig(emu_lib.Emu):
    """emu_lib.Emu plus what signals_cases.run asks of an engine."""

    def __init__(self, workload):
        emu_lib.Emu.__init__(self, workload)
        self.snap = None

    def close(self):
        if self.snap:
            self.L.sfe_snapshot_destroy(self.snap)
            self.snap = None
        emu_lib.Emu.close(self)

    def reset(self, tb, sr):
        A = self.cfg.arenas
        emu_lib.Emu.reset(self, (C.c_uint64 * A)(*tb), (C.c_uint64 * A)(*sr))

    def new_signals(self):
        return EmuSignals(self)

    def reset_arenas(self, mask=None, done_too=False, max_steps=0, tb=None, serial=None):
        A, n = self.cfg.arenas, self.cfg.n_agents
        selected = np.full((A, n), 0xA5, dtype=np.uint8)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        t = None if tb is None else np.array(tb, dtype=np.uint64)
        s = None if serial is None else np.array(serial, dtype=np.uint64)
        sel = abi.ResetSel(None if m is None else m.ctypes.data, 1, 1 if done_too else 0, max_steps, None if t is None else t.ctypes.data,
                           None if s is None else s.ctypes.data, selected.ctypes.data)
        assert self.L.sfe_reset_arenas(self.h, C.byref(sel)) == 0, self.L.sfe_last_error().decode()
        return selected

    def _snap(self):
        if not self.snap:
            self.snap = C.c_void_p()
            assert self.L.sfe_snapshot_create(self.h, 3, C.byref(self.snap)) == 0
        return self.snap

    def save(self, slots):
        assert self.L.sfe_snapshot_save(self.h, self._snap(), np.asarray(slots, dtype=np.int32).ctypes.data) == 0

    def load(self, slots):
        assert self.L.sfe_snapshot_load(self.h, self._snap(), np.asarray(slots, dtype=np.int32).ctypes.data) == 0

    def replay_load(self, streams):
        off = np.zeros(len(streams) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(s) for s in streams])
        flat = np.frombuffer(b"".join(streams) or b"\0", dtype=np.uint8)
        assert self.L.sfe_replay_load(self.h, flat.ctypes.data, off.ctypes.data) == 0, self.L.sfe_last_error().decode()

    def replay_step(self):
        assert self.L.sfe_replay_step(self.h) == 0, self.L.sfe_last_error().decode()


@pytest.mark.parametrize("name", sc.NAMES)
def test_emulated_signals_equal_the_restatement(name):
    c = sc.case(name)
    e = EmuSig(c.w)
    check = sc.Checker(e, name)
    try:
        sref = sc.run(c, e, check)
        assert check.calls == sum(op[0] == "signals" for op in c.script) and sref.reach
    finally:
        check.close()
        e.close()


def test_refusals_launch_nothing():
    c = sc.case("battle3")
    e, other = EmuSig(c.w), EmuSig(c.w)
    s = EmuSignals(e)
    A, n = c.w.cfg.arenas, c.w.cfg.n_agents
    d = np.zeros((A, n, abi.DELTA_WORDS), dtype=np.int32)
    io = abi.SignalsIO(None, d.ctypes.data, None, None, abi.RewardWeights())
    try:
        assert s.step_rc(io) == SF_ERR_STATE and b"before sf_reset" in e.L.sfe_last_error()
        tb, sr = c.script[0][1], c.script[0][2]
        e.reset(tb, sr), other.reset(tb, sr)
        assert s.step_rc(io, env=other) == SF_ERR_STATE and b"another environment" in e.L.sfe_last_error()
        e.step_begin()
        assert s.step_rc(io) == SF_ERR_STATE and b"between sf_step_begin" in e.L.sfe_last_error()
        e.step_end(np.full((A, n), ord("+"), dtype=np.uint8))
        assert e.L.sfe_signals_step(e.h, None, C.byref(io)) == SF_ERR_ARG
        assert e.L.sfe_signals_step(e.h, s.h, None) == SF_ERR_ARG
        assert e.L.sfe_signals_status(s.h, None) == SF_ERR_ARG and e.L.sfe_signals_status(None, None) == SF_ERR_ARG
        assert e.L.sfe_signals_create(e.h, None) == SF_ERR_ARG
        assert e.L.sfe_signals_launches(e.h) == 0 and e.L.sfe_signals_launches(other.h) == 0
        assert not d.any()
        assert s.step_rc(io) == 0 and e.L.sfe_signals_launches(e.h) == 1
        assert (d[:, :, 0] & abi.SIG_REBASED).all()
        none = abi.SignalsIO(None, None, None, None, abi.RewardWeights())  # every output left out: the baseline still moves
        e.step(np.full((A, n), ord("+"), dtype=np.uint8))
        assert s.step_rc(none) == 0 and s.step_rc(io) == 0
        assert not d[:, :, 1:].any() and not (d[:, :, 0] & abi.SIG_REBASED).any()
        assert e.L.sfe_signals_destroy(None) == 0
    finally:
        s.close(), e.close(), other.close()


@pytest.mark.parametrize("name", ["solo-restarts", "battle16"])
def test_body_under_sanitizers(tmp_path, name):
    """The per-agent body in a stand-alone program with its own main, built with ASan and UBSan, over the emulator's states
    of a whole case: the raw buffers k_signals reads, written to one file per call.  Inputs and outputs sit in heap buffers
    of exactly their size; the program's vitals, deltas, reward bits and counters must be the restatement's."""
    exe = str(tmp_path / "signals_main")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "signals_main.cpp")])
    c = sc.case(name)
    e = EmuSig(c.w)
    A, n, H = c.w.cfg.arenas, c.w.cfg.n_agents, c.w.cfg.cap_humans
    files, wants = [], []

    def dump_state(i, engine, pending, wts, want, sref):
        hum, scal = np.zeros(13 * A * H, dtype=np.uint32), np.zeros(A * 24, dtype=np.int32)
        res = np.zeros(A * n * 8, dtype=np.int32)
        assert e.L.sfe_raw_state(e.h, hum.ctypes.data, scal.ctypes.data, res.ctypes.data) == 0
        rb = np.zeros(A * n, dtype=np.int32) if pending is None else np.asarray(pending, dtype=np.int32).reshape(-1)
        files.append(str(tmp_path / ("state%03d.bin" % len(files))))
        with open(files[-1], "wb") as f:
            f.write(np.array([A, H, n], dtype=np.int32).tobytes() + hum.tobytes() + scal.tobytes() + res.tobytes() + rb.tobytes())
        wants.append(want)

    try:
        sc.run(c, e, dump_state)
    finally:
        e.close()
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.split("\n")
    assert lines[4 * len(files)] == "signals_main ok", lines[-3:]
    words = lambda line, tag: np.array([int(x, 16) for x in line.split()[1:]], dtype=np.uint32) if line[0] == tag else None
    unresolved = detected = 0
    for j, (wv, wd, wr, ws) in enumerate(wants):
        assert np.array_equal(words(lines[4 * j], "v"), wv.reshape(-1).view(np.uint32)), (name, j, "vitals")
        assert np.array_equal(words(lines[4 * j + 1], "d"), wd.reshape(-1).view(np.uint32)), (name, j, "delta")
        assert np.array_equal(words(lines[4 * j + 2], "r"), wr.reshape(-1).view(np.uint32)), (name, j, "reward bits")
        unresolved, detected = unresolved + ws[0], detected + ws[1]
        assert lines[4 * j + 3] == "s %d %d" % (unresolved, detected), (name, j, lines[4 * j + 3])
