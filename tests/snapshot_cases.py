"""What the sf_snapshot_* tests share (tests/test_snapshot_emu.py on the wave emulator, tests/test_gpu_snapshot.py on the
device): the comparison of an engine with the restatement (tests/snapshot_ref.py) and the scenarios both run.  An engine has
emu_lib.Emu's surface (reset, step, digest, dump, done, results, phase_draws, cfg) and snapshot(slots), which returns an
object with save / load (host int32 arrays) / status / export / import_ / close.  Test helper only."""
import numpy as np

import reset_sel_cases as rc
from strikeforce_amd import abi

SENTINEL = 0xA5
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def idx(entries):
    return np.asarray(entries, dtype=np.int32)


def without_episodes(d):
    x = d.as_dict()
    x["hdr"]["episodes"] = 0
    return x


def compare_all(e, ref, what, dumps=True):
    got, want = e.digest(), ref.digest()
    assert (got == want).all(), (what, np.nonzero(got != want)[0])
    if dumps:
        for a in range(e.cfg.arenas):
            rc.assert_same_state(ref.dump(a), e.dump(a), a, what)
        assert (e.done() == ref.done()).all(), what


def steps_both(e, ref, cmds, what, dumps_at_end=True):
    for s in range(len(cmds)):
        e.step(cmds[s])
        ref.step(cmds[s])
        compare_all(e, ref, "%s, step %d" % (what, s), dumps=False)
    if dumps_at_end:
        compare_all(e, ref, what + ", after the steps")


def save_both(e, snap, ref, slot_of_arena, what):
    """One save on the engine and on the restatement; no arena may change."""
    before = e.digest()
    snap.save(idx(slot_of_arena))
    ref.save(slot_of_arena)
    assert (e.digest() == before).all(), what
    compare_all(e, ref, what)


def load_both(e, snap, ref, slot_of_arena, what):
    """One load on the engine and on the restatement, and everything it must leave: arenas that take no part keep digest
    and dump, the others equal the restatement (all records, `episodes` the destination's), the latch stays, the phase
    draws are the slot's."""
    A = e.cfg.arenas
    before, dumps_before, latch = e.digest(), [e.dump(a) for a in range(A)], e.results()
    took = np.array([0 <= s < len(ref.slots) and ref.slots[s] is not None for s in slot_of_arena], dtype=bool)
    snap.load(idx(slot_of_arena))
    ref.load(slot_of_arena)
    after = e.digest()
    assert (after[~took] == before[~took]).all(), what
    for a in np.nonzero(~took)[0]:
        rc.assert_same_state(dumps_before[a], e.dump(a), a, what + ": took no part")
    compare_all(e, ref, what)
    assert (e.results() == latch).all() and (latch == ref.results()).all(), what
    draws = e.phase_draws()
    for a in np.nonzero(took)[0]:
        assert [int(x) for x in draws[a]] == ref.phase_draws(a), (what, a)
    return took


def sentinel_blob(valid_blob):
    """A blob with valid_blob's header and a payload of sentinel bytes."""
    return valid_blob[:abi.SNAPSHOT_BLOB_HEADER] + bytes([SENTINEL]) * (len(valid_blob) - abi.SNAPSHOT_BLOB_HEADER)


def round_trip(e, ref, snap, cmds, s1, what):
    """Save all, step s1 more, load all: the state of the save is back (but `episodes`), and the same commands again give
    the first pass's digests after every step.  cmds: at least s1 rows."""
    A = e.cfg.arenas
    at_save, dumps = e.digest(), [e.dump(a) for a in range(A)]
    save_both(e, snap, ref, list(range(A)), what + ": save all")
    first = []
    for s in range(s1):
        e.step(cmds[s]), ref.step(cmds[s])
        first.append(e.digest())
        assert (first[-1] == ref.digest()).all(), (what, s)
    assert (first[-1] != at_save).any()
    took = load_both(e, snap, ref, list(range(A)), what + ": load all")
    assert took.all() and (e.digest() == at_save).all()
    for a in range(A):
        d = e.dump(a)
        assert without_episodes(d) == without_episodes(dumps[a]), (what, a)
    for s in range(s1):
        e.step(cmds[s]), ref.step(cmds[s])
        assert (e.digest() == first[s]).all(), (what, "second pass", s)
    compare_all(e, ref, what + ": after the second pass")


def bad_indices(e, ref, snap, what):
    """Indices `slots`, -2, INT32_MIN, INT32_MAX in a save and in a load, and a load from a slot never written: nothing
    changes anywhere, everything is counted, the counters clear.  The snapshot's last slot must be empty."""
    A, slots = e.cfg.arenas, snap.slots
    bad = [slots, -2, I32_MIN, I32_MAX]
    row = [bad[a % 4] for a in range(A)]
    kept = snap.export(0)
    save_both(e, snap, ref, row, what + ": bad indices, save")
    assert snap.export(0) == kept
    load_both(e, snap, ref, row, what + ": bad indices, load")
    assert snap.status() == ref.status() == (0, 2 * A)
    assert not load_both(e, snap, ref, [slots - 1] * A, what + ": a load from an empty slot").any()
    assert snap.status() == ref.status() == (A, 0)
    assert snap.status() == (0, 0)
