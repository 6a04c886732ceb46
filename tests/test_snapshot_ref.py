"""The restatement of sf_snapshot_save / sf_snapshot_load (tests/snapshot_ref.py) against the oracle it is built from: a loaded
arena is the source as it was at the save, the destination's episode count and result latch stay, forks are twins under equal
commands and part under different ones, and skipped indices leave everything alone.  CPU only."""
import numpy as np

import reset_sel_cases as rc
from oracle_lib import diff_dumps
from snapshot_ref import SnapshotRef
from strikeforce_amd import abi


def as_dict_without_episodes(d):
    x = d.as_dict()
    x["hdr"]["episodes"] = 0
    return x


def test_a_loaded_arena_is_the_source_at_the_save():
    A = 3
    w = rc.workload("lds-nb1", A)
    tb, sr = w.seeds()
    ref = SnapshotRef(w, tb, sr, slots=2)
    cmds = rc.commands("lds-nb1", A, 1, 60)
    for s in range(25):
        ref.step(cmds[s])
    at_save, dumps = ref.digest(), [ref.dump(a) for a in range(A)]
    ref.save([1, -1, 0])
    for s in range(25, 45):
        ref.step(cmds[s])
    assert (ref.digest() != at_save).all()
    ref.load([-1, 0, 1])  # arena 1 <- arena 2's state, arena 2 <- arena 0's
    d = ref.digest()
    assert d[0] != at_save[0] and d[1] == at_save[2] and d[2] == at_save[0]
    assert diff_dumps(as_dict_without_episodes(dumps[2]), as_dict_without_episodes(ref.dump(1))) is None
    assert diff_dumps(as_dict_without_episodes(dumps[0]), as_dict_without_episodes(ref.dump(2))) is None
    assert ref.status() == (0, 0)
    ref.close()


def test_a_load_keeps_the_destinations_episode_count_and_latch():
    A = 2
    w = rc.workload("solo", A)
    tb, sr = w.seeds()
    ref = SnapshotRef(w, tb, sr, slots=1)
    cmds = rc.commands("solo", A, 1, 30)
    cmds[9, 1] = ord("_")  # arena 1's game ends at step 10: one episode counted, its record latched
    for s in range(5):
        ref.step(cmds[s])
    ref.save([0, -1])
    for s in range(5, 12):
        ref.step(cmds[s])
    latch = ref.results()
    assert ref.episodes().tolist() == [0, 1] and latch[1, 0, 7] == abi.DIED and ref.done()[1] == 1
    ref.load([-1, 0])  # the running game of arena 0 at step 5 into the finished arena 1
    assert ref.episodes().tolist() == [0, 1] and ref.done().tolist() == [0, 0]
    assert (ref.results() == latch).all()
    h = ref.dump(1).hdr
    assert h.steps == 5 and h.tb == int(tb[0]) and h.serial == int(sr[0])
    cmds[20, 1] = ord("_")
    for s in range(12, 22):
        ref.step(cmds[s])
    assert ref.episodes().tolist() == [0, 2]  # the count went on from the destination's
    ref.close()


def test_forks_are_twins_until_their_commands_differ():
    A = 4
    w = rc.workload("lds-nb1", A)
    tb, sr = w.seeds()
    ref = SnapshotRef(w, tb, sr, slots=1)
    cmds = rc.commands("lds-nb1", A, 1, 80)
    for s in range(20):
        ref.step(cmds[s])
    ref.save([-1, -1, 0, -1])
    ref.load([0, 0, 0, 0])
    assert len(set(ref.digest().tolist())) == 1
    for s in range(20, 40):  # equal commands: arena 2's row for everybody
        ref.step(np.repeat(cmds[s, 2:3], A, axis=0))
        assert len(set(ref.digest().tolist())) == 1, s
    for s in range(40, 80):  # each arena its own
        ref.step(cmds[s])
    assert len(set(ref.digest().tolist())) == A
    ref.close()


def test_skipped_indices_change_nothing_and_are_counted():
    A = 3
    w = rc.workload("solo", A)
    tb, sr = w.seeds()
    ref = SnapshotRef(w, tb, sr, slots=2)
    cmds = rc.commands("solo", A, 1, 10)
    for s in range(10):
        ref.step(cmds[s])
    before = ref.digest()
    ref.load([0, 1, -1])  # nothing saved yet
    assert ref.status() == (2, 0) and (ref.digest() == before).all()
    ref.save([2, -2, -2 ** 31])
    ref.load([2 ** 31 - 1, 0, 1])
    assert ref.status() == (2, 4) and ref.status() == (0, 0) and (ref.digest() == before).all()
    ref.close()
