"""Loader for tests/emu/libsf_emu.so: the device core run on a CPU wave emulator, with every `sfe_` entry point bound
once.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

from strikeforce_amd import abi
from oracle_lib import ROOT, dump_with

_LIBS = {}


def lib(asan=False):
    name = "libsf_emu_asan.so" if asan else "libsf_emu.so"
    if name not in _LIBS:
        d = os.path.join(ROOT, "tests", "emu")
        # make is a no-op when the file __graft_entry__.build() made is up to date with its sources
        subprocess.check_call(["make", "-s", "-C", d, name])
        L = C.CDLL(os.path.join(d, name))
        vp = C.c_void_p
        L.sfe_create.argtypes = [C.POINTER(abi.Config)]
        L.sfe_create.restype = vp
        abi.bind(L, "sfe_")
        abi.bind_snapshot(L, "sfe_")
        abi.bind_signals(L, "sfe_")
        L.sfe_step_many.argtypes = [vp, C.c_char_p, C.c_int32]
        L.sfe_last_error.restype = C.c_char_p
        L.sfe_last_variant.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32)]
        L.sfe_reset_arenas.argtypes = [vp, C.POINTER(abi.ResetSel)]
        L.sfe_episode_log.argtypes = [vp, C.c_int32]
        L.sfe_episode_ring.argtypes = [vp, vp]
        L.sfe_replay_load.argtypes = [vp, vp, vp]
        L.sfe_replay_step.argtypes = [vp]
        L.sfe_replay_status.argtypes = [vp, vp]
        L.sfe_replay_commands.argtypes = [vp, vp]
        L.sfe_fixed_shapes.argtypes = [vp, C.c_int32]
        for n in ("sfe_step_kernel", "sfe_last_parts", "sfe_signals_launches"):
            getattr(L, n).argtypes = [vp]
        L.sfe_scal.argtypes = [vp, C.c_int32, vp]
        L.sfe_raw_state.argtypes = [vp] * 4
        _LIBS[name] = L
    return _LIBS[name]


class Emu:
    """Same call surface as oracle_lib.Oracle."""

    def __init__(self, workload, asan=False):
        self.w = workload
        self.cfg = workload.cfg
        self.L = lib(asan)
        self.h = self.L.sfe_create(C.byref(self.cfg))
        if not self.h:
            raise ValueError("emu rejected the configuration: %s" % self.L.sfe_last_error().decode())

    def close(self):
        if self.h:
            self.L.sfe_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def reset(self, tb, serial):
        assert self.L.sfe_reset(self.h, tb, serial) == 0

    def step(self, cmd):
        cmd = np.ascontiguousarray(cmd, dtype=np.uint8)
        assert cmd.size == self.cfg.arenas * self.cfg.n_agents
        assert self.L.sfe_step(self.h, cmd.ctypes.data_as(C.c_char_p)) == 0

    def step_many(self, cmds):
        cmds = np.ascontiguousarray(cmds, dtype=np.uint8)
        assert self.L.sfe_step_many(self.h, cmds.ctypes.data_as(C.c_char_p), cmds.shape[0]) == 0

    def step_begin(self):
        assert self.L.sfe_step_begin(self.h) == 0

    def step_end(self, cmd):
        cmd = np.ascontiguousarray(cmd, dtype=np.uint8)
        assert cmd.size == self.cfg.arenas * self.cfg.n_agents
        assert self.L.sfe_step_end(self.h, cmd.ctypes.data_as(C.c_char_p)) == 0

    def agent_alive(self):
        out = np.zeros((self.cfg.arenas, self.cfg.n_agents), dtype=np.uint8)
        assert self.L.sfe_agent_alive(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
        return out

    def phase_draws(self, arena=None):
        out = np.zeros((self.cfg.arenas, 6), dtype=np.int32)
        assert self.L.sfe_phase_draws(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))) == 0
        return out if arena is None else [int(x) for x in out[arena]]

    def observe(self):
        out = np.empty((self.cfg.arenas, self.cfg.n_agents, abi.OBS_CHANNELS, abi.OBS_WINDOW, abi.OBS_WINDOW),
                       dtype=np.float32)
        assert self.L.sfe_observe(self.h, out.ctypes.data_as(C.POINTER(C.c_float))) == 0
        return out

    def results(self):
        out = np.zeros((self.cfg.arenas, self.cfg.n_agents, 8), dtype=np.int32)
        assert self.L.sfe_results(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))) == 0
        return out

    def done(self):
        out = np.zeros(self.cfg.arenas, dtype=np.uint8)
        assert self.L.sfe_done(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
        return out

    def digest(self):
        out = np.zeros(self.cfg.arenas, dtype=np.uint64)
        assert self.L.sfe_state_digest(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
        return out

    def dump(self, arena):
        return dump_with(self.L.sfe_dump_arena, self.h, self.cfg, arena)

    KINDS = {"reset": 0, "step": 1, "step_half": 2, "reset_sel": 3}

    def last_variant(self, kind):
        """(NB, HP, BM, ZL): the template arguments of the last launch of k_reset / k_step / k_step_half / k_reset_sel
        ("reset", "step", "step_half", "reset_sel"), as the device's launchers would pick them; (0, 0, 0, 0) before the
        first."""
        out = (C.c_int32 * 4)()
        assert self.L.sfe_last_variant(self.h, self.KINDS[kind], out) == 0
        return tuple(out)
