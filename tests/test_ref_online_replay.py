"""Online `.sf_sample` files against the reference's own writer and reader (oracle/_ref/sf_ref_tick on
oracle/_ref/sf_match_server; skipped where they are not built).  The reference WRITES one layout (gameplay.hpp:1836-1845)
and READS another (:1762-1778,1796-1806): a match its client logs is read here as "logged" and replayed on the oracle to
the client's LIVE state after every iteration; written here as "replay" it is replayed by the reference itself to the
oracle's final world; so is a match played entirely here, with a quit in it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import online_cases as oc
import reftick
from oracle_lib import Oracle, ROOT
from strikeforce_amd import abi, config, replay

SERVER = os.path.join(ROOT, "oracle", "_ref", "sf_match_server")
pytestmark = pytest.mark.skipif(not (reftick.available() and os.path.exists(SERVER)),
                                reason="oracle/_ref/sf_ref_tick / sf_match_server not built (no reference checkout)")


def _generator():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_online_sample
    return make_online_sample


def _reference_replays(sample, f, iterations):
    """The reference's own replay mode on `sample` written in the layout it reads: its final dump."""
    w = oc.workload(sample, f)
    r = reftick.RefTick(w, config.HUMAN_TOKENS, native_caps=False)  # (the records come from the file)
    replay.write_sample(os.path.join(r.dir, "match.sf_sample"), sample, layout="replay")
    _tb, serial = r.reset_native(replay_path="match.sf_sample")
    assert serial == sample.serial
    for _ in range(iterations):
        r.step("+")  # replay mode: human_action takes every command from the file (gameplay.hpp:968-969,984-985)
    d = r.dump()
    assert r.over == 0
    r.close()
    return d


@pytest.mark.parametrize("quit_at", [None, (2, 50)], ids=["plain", "quit"])
def test_a_match_the_reference_logs_replays_here_and_in_the_reference(quit_at, tmp_path):
    g = _generator()
    text, f, live = g.play_match(quit_at)
    p = tmp_path / "logged.sf_sample"
    p.write_text(text)
    s = replay.read_sample(str(p), layout="logged", teams=f["teams"])
    assert len(s.commands) == (3 * 120 if quit_at is None else 3 * 51 + 2 * 69)
    # (a) here, on the oracle, against the reference client's live dumps
    o = Oracle(oc.workload(s, f))
    diffs = []

    def compare(n, sim, _row):
        d = reftick.first_difference(live[n - 1], reftick.arrays_of(sim.dump(0)))
        if d:
            diffs.append((n, d))

    assert replay.replay_lines(s, o, compare) == (120, abi.REPLAY_SAMPLE_ENDED, len(s.commands))
    assert diffs == []
    # (b) the reference replays the file once it is in the layout its reader expects
    d = reftick.first_difference(_reference_replays(s, f, 120), reftick.arrays_of(o.dump(0)))
    assert d is None, d


def test_a_match_played_here_replays_in_the_reference():
    """(c): three players on the oracle, the rival in seat 0 quits in iteration 30; written as "replay"."""
    s = oc.play_and_log(1_700_000_123, 987_654_321, 90, seed=5, quit_at=(0, 30))
    assert len(s.commands) == 3 * 31 + 2 * 59
    o = Oracle(oc.workload(s, oc.BATCH))
    assert replay.replay_lines(s, o) == (90, abi.REPLAY_SAMPLE_ENDED, len(s.commands))
    d = reftick.first_difference(_reference_replays(s, oc.BATCH, 90), reftick.arrays_of(o.dump(0)))
    assert d is None, d


def test_a_levelled_record_is_levelled_up_twice_by_the_file():
    """Human::log_file writes def_Hp / mindamage_def / def_stamina AFTER the level-ups Human::build applied and scan_file
    applies them again (tests/test_ref_replay.py documents it for offline files): the replay of a level-10 account starts
    27 level-ups stronger than the live match did — exactly +1350 Hp, +135 damage, +1350 stamina for each player, and
    nothing else differs after the placement."""
    g = _generator()
    rich = [15000, 1000, 15000, 10, 10, 10, 300000, 60, 0, 0, 0, 1, 1, 1, 34] + [1] * 16 + [56]
    text, f, live = g.play_match(None, record=rich)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "levelled.sf_sample")
        open(path, "w").write(text)
        s = replay.read_sample(path, layout="logged", teams=f["teams"])
    assert all(r[:3] == [15000 + 27 * 50, 1000 + 27 * 5, 15000 + 27 * 50] and r[3:] == rich[3:] for r in s.records)
    o = Oracle(oc.workload(s, f))
    o.reset((C.c_uint64 * 1)(s.tb), (C.c_uint64 * 1)(s.serial))
    ours, ref = reftick.arrays_of(o.dump(0)), live[-1]
    delta = np.asarray(ours["humans"], dtype=np.int64) - np.asarray(ref["humans"], dtype=np.int64)
    delta[:, 3] = 0  # (`profile`: the reference has no such column)
    want = np.zeros_like(delta)
    want[:3, 9], want[:3, 10], want[:3, 11] = 27 * 50, 27 * 50, 27 * 5  # hp, stamina, mindamage (abi.HumanRec)
    assert (delta == want).all(), delta[:3]
    same = dict(ours, humans=ref["humans"])
    assert reftick.first_difference(ref, same) is None
