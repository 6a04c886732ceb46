"""The restatement of sf_reset_arenas (tests/reset_sel_ref.py) against hand-written selections and against the oracle's own
two ways to start a game: a chosen arena is a fresh sfo_reset on its seed with the episode ordinal and the result latch
kept, an arena that is not chosen does not move, and auto_reset = 0 plus `restart what is done, on the next seed` after
every step is auto_reset = 1."""
import ctypes as C

import numpy as np
import pytest

from oracle_lib import Oracle, diff_dumps
from reset_sel_ref import ResetSelRef, choose, seed_stride, single_arena
from strikeforce_amd import config

POISON = 0xDEAD_BEEF_DEAD_BEEF


def test_selectors_alone():
    done, steps = [0, 1, 0, 1, 0], [3, 9, 7, 2, 0]
    assert choose(None, done, steps, False, 0).tolist() == [False] * 5
    assert choose([0, 0, 5, 0, 1], done, steps, False, 0).tolist() == [False, False, True, False, True]
    assert choose(None, done, steps, True, 0).tolist() == [False, True, False, True, False]
    assert choose(None, done, steps, False, 7).tolist() == [False, False, True, False, False]


def test_selectors_combined():
    done, steps = [0, 1, 0, 1, 0], [3, 9, 7, 2, 0]
    assert choose([1, 0, 0, 0, 0], done, steps, True, 0).tolist() == [True, True, False, True, False]
    assert choose([1, 0, 0, 0, 0], done, steps, False, 3).tolist() == [True, False, True, False, False]
    assert choose(None, done, steps, True, 7).tolist() == [False, True, True, True, False]
    assert choose([0, 0, 0, 0, 1], done, steps, True, 7).tolist() == [False, True, True, True, True]


def test_a_done_arena_is_never_chosen_by_max_steps():
    assert choose(None, [1, 1], [100, 5], False, 5).tolist() == [False, False]
    assert choose(None, [1, 0], [100, 100], False, 5).tolist() == [False, True]


def test_steps_boundary():
    assert choose(None, [0, 0, 0], [4, 5, 6], False, 5).tolist() == [False, True, True]
    assert choose(None, [0, 0, 0], [4, 5, 6], False, 0).tolist() == [False, False, False]


def _workload(arenas, auto_reset):
    w = config.baseline_workload("C1", arenas=arenas, auto_reset=auto_reset)
    w.cfg.reseed_stride = 1000
    return w


def test_chosen_is_a_fresh_reset_and_the_others_stand():
    w = _workload(4, 0)
    tb, sr = w.seeds()
    ref = ResetSelRef(w, tb, sr)
    cmds, _ = config.bench_commands(4, 1, 30)
    for s in range(30):
        ref.step(cmds[s])
    before = ref.digest()
    ntb = [POISON, 77, POISON, 99]
    nsr = [POISON, 5, POISON, 6]
    sel = ref.reset_arenas(mask=[0, 1, 0, 1], tb=ntb, serial=nsr)
    assert sel.tolist() == [False, True, False, True]
    after = ref.digest()
    assert after[0] == before[0] and after[2] == before[2] and after[1] != before[1]
    for a in (1, 3):
        fresh = Oracle(single_arena(w))
        fresh.reset((C.c_uint64 * 1)(ntb[a]), (C.c_uint64 * 1)(nsr[a]))
        assert diff_dumps(fresh.dump(0).as_dict(), ref.dump(a).as_dict()) is None
        assert ref.dump(a).hdr.steps == 0 and ref.dump(a).hdr.done == 0
    assert ref.dump(0).hdr.steps == 30


def test_max_steps_cuts_at_the_boundary_and_by_the_next_seed_rule():
    w = _workload(3, 0)
    tb, sr = w.seeds()
    ref = ResetSelRef(w, tb, sr)
    cmds, _ = config.bench_commands(3, 1, 8)
    for s in range(7):
        ref.step(cmds[s])
    assert not ref.reset_arenas(max_steps=8).any()  # steps == max_steps - 1
    ref.step(cmds[7])
    assert ref.reset_arenas(max_steps=8).all()  # steps == max_steps
    for a in range(3):
        h = ref.dump(a).hdr
        assert (h.tb, h.serial, h.steps, h.episodes) == (tb[a] + seed_stride(w.cfg), sr[a], 0, 0)  # a cut game is no episode


def test_episode_ordinal_and_latch_survive_a_restart():
    w = _workload(2, 0)
    tb, sr = w.seeds()
    ref = ResetSelRef(w, tb, sr)
    quit_ = np.full((2, 1), ord("_"), dtype=np.uint8)
    ref.step(quit_)  # the reference's own quit command ends both games as episodes
    assert ref.done().tolist() == [1, 1] and ref.episodes().tolist() == [1, 1]
    latched = ref.results()
    assert (latched[:, 0, 7] != 0).all()
    assert ref.reset_arenas(done_too=True).tolist() == [True, True]
    assert ref.done().tolist() == [0, 0] and ref.episodes().tolist() == [1, 1]
    assert (ref.results() == latched).all()
    ref.step(quit_)
    assert ref.episodes().tolist() == [2, 2]
    assert not ref.reset_arenas(mask=[0, 0]).any() and ref.done().tolist() == [1, 1]


STEPS = 500  # of configs[1], eight arenas: games end at steps 146, 206, 433, 469 — the first hundred with three restarts behind it (asserted below)


def test_done_too_after_every_step_is_auto_reset():
    A = 8
    w1 = config.baseline_workload("C2", arenas=A, auto_reset=1)
    w0 = config.baseline_workload("C2", arenas=A, auto_reset=0)
    tb, sr = w1.seeds()
    auto = Oracle(w1)
    auto.reset(tb, sr)
    ref = ResetSelRef(w0, tb, sr)
    cmds, _ = config.bench_commands(A, 1, STEPS)
    for s in range(STEPS):
        auto.step(cmds[s])
        ref.step(cmds[s])
        sel = ref.reset_arenas(done_too=True)
        assert (sel == (auto.done() != 0)).all(), s
        want, got = auto.digest(), ref.digest()
        assert (want == got).all(), (s, np.nonzero(want != got)[0])
        if sel.any() or s % 100 == 99:
            for a in range(A):
                d = diff_dumps(auto.dump(a).as_dict(), ref.dump(a).as_dict())
                assert d is None, (s, a, d)
    assert ref.restarts.sum() >= 3, ref.restarts
    assert (ref.episodes() == ref.restarts).all()
