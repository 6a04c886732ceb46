"""sf_snapshot_save / sf_snapshot_load on the CPU wave emulator: the product's host code (Env::snapshot_*, sf_host.hpp) and
the copy kernel's body (sf_snapshot.hpp SnapCore) against the restatement over the oracle (tests/snapshot_ref.py), with full
dumps, done flags and digests of EVERY arena after each call, for an LDS-plane, two HBM-plane and a large-pool world and for
every game mode; the large pools in both directions (a small state into an arena whose tables were in use past word 0, and
back); bad indices; the blob through the host code; the host's refusals.

The emulator's runtime (tests/emu/sf_emu.cpp) has the launch; here the index arrays are host memory.  The pointer checks
of the HIP runtime and stream order are covered on the device (tests/test_gpu_snapshot.py)."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
import reset_sel_cases as rc
import snapshot_cases as sc
from snapshot_ref import SnapshotRef
from strikeforce_amd import abi

SF_ERR_ARG, SF_ERR_STATE = -1, -4


class EmuSnapshot:
    def __init__(self, e, slots):
        self.e, self.L, self.slots = e, e.L, slots
        self.h = C.c_void_p()
        assert self.L.sfe_snapshot_create(e.h, slots, C.byref(self.h)) == 0, self.L.sfe_last_error().decode()
        d, b = C.c_int64(), C.c_int64()
        assert self.L.sfe_snapshot_slot_bytes(e.h, C.byref(d), C.byref(b)) == 0
        self.device_bytes, self.blob_bytes = d.value, b.value

    def save_rc(self, slot_of_arena):
        return self.L.sfe_snapshot_save(self.e.h, self.h, None if slot_of_arena is None else slot_of_arena.ctypes.data)

    def load_rc(self, slot_of_arena):
        return self.L.sfe_snapshot_load(self.e.h, self.h, None if slot_of_arena is None else slot_of_arena.ctypes.data)

    def save(self, slot_of_arena):
        assert self.save_rc(slot_of_arena) == 0, self.L.sfe_last_error().decode()

    def load(self, slot_of_arena):
        assert self.load_rc(slot_of_arena) == 0, self.L.sfe_last_error().decode()

    def status(self):
        out = (C.c_int32 * 4)()
        assert self.L.sfe_snapshot_status(self.h, C.byref(out)) == 0
        assert out[2] == 0 and out[3] == 0
        return out[0], out[1]

    def export_rc(self, slot, size=None):
        buf = C.create_string_buffer(self.blob_bytes)
        return self.L.sfe_snapshot_export(self.h, slot, C.cast(buf, C.c_void_p), self.blob_bytes if size is None else size), buf.raw

    def export(self, slot):
        rc_, blob = self.export_rc(slot)
        assert rc_ == 0, self.L.sfe_last_error().decode()
        return blob

    def import_rc(self, slot, blob):
        return self.L.sfe_snapshot_import(self.h, slot, C.cast(C.c_char_p(blob), C.c_void_p), len(blob))

    def import_(self, slot, blob):
        assert self.import_rc(slot, blob) == 0, self.L.sfe_last_error().decode()

    def close(self):
        if self.h:
            self.L.sfe_snapshot_destroy(self.h)
            self.h = None


class EmuSnap(emu_lib.Emu):
    def snapshot(self, slots):
        return EmuSnapshot(self, slots)

    def scal(self, a):
        out = np.zeros(24, dtype=np.int32)
        assert self.L.sfe_scal(self.h, a, out.ctypes.data) == 0
        return out


SC_ZWN, SC_PWN = 18, 19  # sf_types.hpp


@pytest.mark.parametrize("name", ["lds-nb1", "hbm-bm", "hbm", "zl", "solo", "kits"])
def test_emulated_copies_equal_the_restatement(name):
    A = 2 if name == "zl" else 3
    w = rc.workload(name, A)
    n = w.cfg.n_agents
    tb, sr = w.seeds()
    e, ref = EmuSnap(w), SnapshotRef(w, tb, sr, slots=4)
    snap = e.snapshot(4)
    assert snap.blob_bytes == snap.device_bytes - 4 + abi.SNAPSHOT_BLOB_HEADER
    e.reset(tb, sr)
    lead = 0 if name == "zl" else 30  # (the large-pool world's players lay exits from the first step on)
    cmds = rc.commands(name, A, n, (rc.ZL_STEPS if name == "zl" else lead) + 80)
    sc.steps_both(e, ref, cmds[:lead], "lead", dumps_at_end=True)
    at = lead
    if name == "zl":  # a small state in slot 3 (tables inside their first 64-slot word), then on to the big one
        for a in range(A):
            z, p = rc.large_pool_reach(ref.dump(a))
            assert z < 64 and p < 64, (a, z, p)
        assert e.scal(0)[SC_ZWN] == 1 and e.scal(0)[SC_PWN] == 1
        sc.save_both(e, snap, ref, [3, -1], "the small state")
        e.step_many(cmds[lead:rc.ZL_STEPS])
        for s in range(lead, rc.ZL_STEPS):
            ref.step(cmds[s])
        at = rc.ZL_STEPS
        for a in range(A):
            z, p = rc.large_pool_reach(ref.dump(a))
            assert z >= 64 and p >= 64, (a, z, p)
        sc.compare_all(e, ref, "the big state")
        sc.save_both(e, snap, ref, [-1, 2], "the big state saved")
        assert sc.load_both(e, snap, ref, [-1, 3], "small into big").tolist() == [False, True]
        assert e.scal(1)[SC_ZWN] == 1 and e.scal(1)[SC_PWN] == 1  # and every slot behind them is clear: the dumps agree
        sc.steps_both(e, ref, cmds[at:at + 10], "behind small into big")
        at += 10
        assert sc.load_both(e, snap, ref, [2, 2], "big into small, and a fork").all()
        assert e.scal(1)[SC_ZWN] == 2 and e.scal(1)[SC_PWN] == 2
        sc.steps_both(e, ref, cmds[at:at + 10], "behind big into small")
        at += 10
    sc.round_trip(e, ref, snap, cmds[at:at + 20], 20, name)
    at += 20
    # a selection with a fork: arena 0 saved into slot 1, the last arena untouched by the save; slot 1 into the others
    sc.steps_both(e, ref, cmds[at:at + 5], "on", dumps_at_end=False)
    at += 5
    sc.save_both(e, snap, ref, [1] + [-1] * (A - 1), "save arena 0 into slot 1")
    sc.steps_both(e, ref, cmds[at:at + 5], "on", dumps_at_end=False)
    at += 5
    took = sc.load_both(e, snap, ref, [-1] + [1] * (A - 1), "fork slot 1 into the others")
    assert took.tolist() == [False] + [True] * (A - 1)
    sc.steps_both(e, ref, cmds[at:at + 20], "the forks on commands of their own")
    assert e.L.sfe_last_parts(e.h) >= 1
    snap.close(), e.close(), ref.close()


@pytest.mark.parametrize("rows,cols", [(9, 7), (10, 7), (12, 6)])
def test_cell_counts_that_take_the_narrow_paths(rows, cols):
    """63 cells: the damage plane goes by dwords, the exit-number plane by 16-bit words, and odd arenas' rows of it start
    off a dword; 70 cells: both by dwords; 72 cells: the exit-number plane 16 bytes at a time, the damage plane by dwords.
    One human (rows of 4 bytes) beside twelve (rows of 48)."""
    from strikeforce_amd import config
    A = 3
    H = 1 if rows == 9 else 12
    cfg = config.make_config(A, rows, cols, H=H, Z=5, B=7, P=3)
    m, p = config.synthetic_map(rows, cols, wall_p=0.05, portal_pairs=1)
    w = config.Workload("narrow", cfg, m, p)
    tb, sr = w.seeds()
    e, ref = EmuSnap(w), SnapshotRef(w, tb, sr, slots=3)
    snap = e.snapshot(3)
    e.reset(tb, sr)
    cmds = rc.commands("solo", A, 1, 100)
    sc.steps_both(e, ref, cmds[:30], "lead")
    sc.round_trip(e, ref, snap, cmds[30:50], 20, "narrow")
    sc.save_both(e, snap, ref, [-1, 2, -1], "the odd arena alone")
    sc.steps_both(e, ref, cmds[50:60], "on", dumps_at_end=False)
    sc.load_both(e, snap, ref, [2, -1, 2], "into its neighbours")
    sc.steps_both(e, ref, cmds[60:90], "forks")
    snap.close(), e.close(), ref.close()


def test_bad_indices_and_blobs():
    A = 5
    w = rc.workload("solo", A)
    tb, sr = w.seeds()
    e, ref = EmuSnap(w), SnapshotRef(w, tb, sr, slots=3)
    snap = e.snapshot(3)
    e.reset(tb, sr)
    cmds = rc.commands("solo", A, 1, 40)
    sc.steps_both(e, ref, cmds[:10], "lead", dumps_at_end=False)
    sc.save_both(e, snap, ref, [0, 1, -1, -1, -1], "two slots filled")
    at_save = e.digest()[1]
    sc.bad_indices(e, ref, snap, "solo")
    # the blob: out and in again, into another slot and another environment of the same configuration, arena count apart
    blob = snap.export(1)
    assert len(blob) == snap.blob_bytes and blob[:4] == b"SFSN"
    assert snap.export_rc(2)[0] == SF_ERR_STATE  # never saved
    assert snap.export_rc(3)[0] == SF_ERR_ARG and snap.export_rc(-1)[0] == SF_ERR_ARG
    assert snap.export_rc(1, snap.blob_bytes - 1)[0] == SF_ERR_ARG
    for bad in (blob[:-1], blob[:10], b"", b"XFSN" + blob[4:], blob[:4] + b"\x02" + blob[5:], blob[:8] + b"\x01" + blob[9:],
                blob[:16] + bytes([blob[16] ^ 1]) + blob[17:]):
        assert snap.import_rc(2, bad) == SF_ERR_ARG, len(bad)
    assert snap.export_rc(2)[0] == SF_ERR_STATE  # the refused imports touched nothing
    assert snap.import_rc(3, blob) == SF_ERR_ARG
    snap.import_(2, sc.sentinel_blob(blob))
    assert snap.export(2) == sc.sentinel_blob(blob)
    snap.import_(2, blob + b"tail bytes are not looked at")
    assert snap.export(2) == blob
    ref.slots[2] = ref.slots[1]
    sc.steps_both(e, ref, cmds[10:20], "on", dumps_at_end=False)
    sc.load_both(e, snap, ref, [2, -1, 2, -1, 1], "the imported slot")
    sc.steps_both(e, ref, cmds[20:30], "behind the import")
    w2 = rc.workload("solo", 2)
    w2.cfg.reseed_stride = A  # (the effective stride is part of the fingerprint: the default is the arena count)
    e2 = EmuSnap(w2)
    snap2 = e2.snapshot(1)
    e2.reset(*w2.seeds())
    snap2.import_(0, blob)
    snap2.load(sc.idx([0, 0]))
    assert (e2.digest() == at_save).all()
    w3 = rc.workload("solo", 2, auto_reset=1)
    w3.cfg.reseed_stride = A
    e3 = EmuSnap(w3)
    snap3 = e3.snapshot(1)
    assert snap3.import_rc(0, blob) == SF_ERR_ARG and b"configuration" in e.L.sfe_last_error()
    for x in (snap, snap2, snap3, e, e2, e3, ref):
        x.close()


def test_refusals():
    w = rc.workload("solo", 2)
    e, other = EmuSnap(w), EmuSnap(w)
    h = C.c_void_p()
    assert e.L.sfe_snapshot_create(e.h, 0, C.byref(h)) == SF_ERR_ARG and e.L.sfe_snapshot_create(e.h, -1, C.byref(h)) == SF_ERR_ARG
    assert e.L.sfe_snapshot_create(e.h, 1, None) == SF_ERR_ARG
    snap, row = e.snapshot(2), sc.idx([0, 1])
    assert snap.save_rc(row) == SF_ERR_STATE and snap.load_rc(row) == SF_ERR_STATE  # before the first sf_reset
    e.reset(*w.seeds()), other.reset(*w.seeds())
    assert snap.save_rc(None) == SF_ERR_ARG and snap.load_rc(None) == SF_ERR_ARG
    assert e.L.sfe_snapshot_save(e.h, None, row.ctypes.data) == SF_ERR_ARG
    assert e.L.sfe_snapshot_save(other.h, snap.h, row.ctypes.data) == SF_ERR_STATE  # another environment's snapshot
    assert e.L.sfe_snapshot_load(other.h, snap.h, row.ctypes.data) == SF_ERR_STATE
    e.step_begin()
    assert snap.save_rc(row) == SF_ERR_STATE and snap.load_rc(row) == SF_ERR_STATE
    e.step_end(np.full((2, 1), ord("+"), dtype=np.uint8))
    stream, off = np.frombuffer(b"++", dtype=np.uint8), np.array([0, 1, 2], dtype=np.int64)
    assert e.L.sfe_replay_load(e.h, stream.ctypes.data, off.ctypes.data) == 0
    assert snap.save_rc(row) == SF_ERR_STATE and snap.load_rc(row) == SF_ERR_STATE  # while a replay is loaded
    assert e.L.sfe_replay_load(e.h, None, None) == 0
    assert snap.save_rc(row) == 0 and snap.load_rc(row) == 0 and snap.status() == (0, 0)
    snap.close(), e.close(), other.close()
