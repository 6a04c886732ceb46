"""sf_reset_arenas' device core (sf_core.hpp reset_sel_body, the body of k_reset_sel) on the CPU wave emulator, against the
restatement over the oracle (tests/reset_sel_ref.py): full dumps, phase draws and digests of EVERY arena after each of a
few calls interleaved with steps — the chosen arenas a fresh reset with the episode ordinal kept, the others untouched —
for an LDS-plane, an HBM-plane and a large-pool instance and for every game mode; the host's refusals; and the
auto_reset = 0 + done_too loop against an auto_reset = 1 twin.

The emulator's runtime (tests/emu/sf_emu.cpp) has the launch; here the pointers of sf_reset_sel are host memory.  The
pointer checks of the HIP runtime, stream order and the composition with the policy library are covered on the device
(tests/test_gpu_reset_sel.py)."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
import reset_sel_cases as rc
from reset_sel_ref import ResetSelRef, seed_stride
from strikeforce_amd import abi, config

SF_ERR_ARG, SF_ERR_STATE = -1, -4


class EmuSel(emu_lib.Emu):
    def reset_arenas_rc(self, mask=None, mask_stride=1, done=False, max_steps=0, tb=None, serial=None, selected=None):
        ptr = lambda x: None if x is None else x.ctypes.data
        sel = abi.ResetSel(ptr(mask), mask_stride, 1 if done else 0, max_steps, ptr(tb), ptr(serial), ptr(selected))
        return self.L.sfe_reset_arenas(self.h, C.byref(sel))

    def reset_arenas(self, **kw):
        assert self.reset_arenas_rc(**kw) == 0, self.L.sfe_last_error().decode()


def compare_all(e, ref, what, dumps=True):
    got, want = e.digest(), ref.digest()
    assert (got == want).all(), (what, np.nonzero(got != want)[0])
    if dumps:
        for a in range(e.cfg.arenas):
            rc.assert_same_state(ref.dump(a), e.dump(a), a, what)


def call_both(e, ref, what, mask=None, stride=1, done=False, max_steps=0, seeds_base=None):
    """One sf_reset_arenas call on the emulated device and on the restatement; everything it must leave is asserted."""
    A, n = e.cfg.arenas, e.cfg.n_agents
    before = e.digest()
    hdrs = [ref.hdr(a) for a in range(A)]
    from reset_sel_ref import choose
    sel = choose(mask, [h.done for h in hdrs], [h.steps for h in hdrs], done, max_steps)
    tb = sr = None
    if seeds_base is not None:
        tb, sr = rc.seeds_for(sel, seeds_base, A)
    dmask = None
    if mask is not None:  # the flags at mask_stride, everything between them set: only the arena's own byte may count
        dmask = np.full((A - 1) * stride + 1, 0 if stride == 1 else 1, dtype=np.uint8)
        dmask[::stride] = mask
    selected = np.full((A, n), rc.SENTINEL, dtype=np.uint8)
    e.reset_arenas(mask=dmask, mask_stride=stride, done=done, max_steps=max_steps, tb=tb, serial=sr, selected=selected)
    got = ref.reset_arenas(mask=mask, done_too=done, max_steps=max_steps, tb=tb, serial=sr)
    assert (got == sel).all()
    assert (selected == np.repeat(sel.astype(np.uint8)[:, None], n, axis=1)).all(), (what, selected)
    after = e.digest()
    assert (after[~sel] == before[~sel]).all(), what
    compare_all(e, ref, what)
    draws = e.phase_draws()
    for a in np.nonzero(sel)[0]:
        assert list(draws[a]) == ref.phase_draws(a), (what, a)
    return sel


def steps_both(e, ref, cmds, what, dumps_at_end=True):
    for s in range(len(cmds)):
        e.step(cmds[s])
        ref.step(cmds[s])
        compare_all(e, ref, "%s, step %d" % (what, s), dumps=False)
    if dumps_at_end:
        compare_all(e, ref, what + ", after the steps")


@pytest.mark.parametrize("name", ["lds-nb1", "hbm-bm", "hbm", "zl", "solo", "kits", "b8", "lds-nb2"])
def test_emulated_restart_equals_the_restatement(name):
    A = 2 if name == "zl" else 3
    w = rc.workload(name, A)
    n = w.cfg.n_agents
    tb, sr = w.seeds()
    e, ref = EmuSel(w), ResetSelRef(w, tb, sr)
    e.reset(tb, sr)
    lead = rc.ZL_STEPS if name == "zl" else 30
    cmds = rc.commands(name, A, n, lead + 60)
    e.step_many(cmds[:lead])
    for s in range(lead):
        ref.step(cmds[s])
    if name == "zl":  # the game that is cut had the second 64-slot word of both tables in use
        for a in range(A):
            z, p = rc.large_pool_reach(ref.dump(a))
            assert z >= 64 and p >= 64, (a, z, p)
    compare_all(e, ref, "before the first call")
    sel = call_both(e, ref, "alternating, seeds given", mask=rc.selection("alternating", A), seeds_base=5000)
    assert sel.tolist() == [bool((a + 1) % 2) for a in range(A)]
    assert e.last_variant("reset_sel") == rc.VARIANT[name]
    steps_both(e, ref, cmds[lead:lead + 20], "after call 1")
    call_both(e, ref, "last, by sf_done_device's stride, the next seed", mask=rc.selection("last", A), stride=n)
    steps_both(e, ref, cmds[lead + 20:lead + 40], "after call 2")
    call_both(e, ref, "none", mask=rc.selection("none", A), seeds_base=6000)
    sel = call_both(e, ref, "max_steps", max_steps=25, seeds_base=7000)
    assert sel.any() and not sel.all()  # the arena restarted by call 2 has played 20 steps, the others 40 or more
    call_both(e, ref, "all", mask=rc.selection("all", A), seeds_base=8000)
    steps_both(e, ref, cmds[lead + 40:lead + 60], "after call 5")
    assert (ref.episodes() == [e.dump(a).hdr.episodes for a in range(A)]).all()
    e.close(), ref.close()


def test_done_too_restarts_what_quit_and_keeps_ordinal_and_latch():
    """The reference's own quit command ends a game as an episode; done_too then restarts it: the ordinal goes on counting
    and the result latch keeps the record of the game that ended."""
    A = 4
    w = rc.workload("solo", A)
    tb, sr = w.seeds()
    e, ref = EmuSel(w), ResetSelRef(w, tb, sr)
    e.reset(tb, sr)
    cmds = rc.commands("solo", A, 1, 30)
    cmds[9, 1::2] = ord("_")
    cmds[19, :] = ord("_")
    steps_both(e, ref, cmds[:10], "lead")
    latched = e.results()
    assert (latched == ref.results()).all() and (latched[1::2, 0, 7] == abi.DIED).all()  # ('_' takes the player's Hp)
    sel = call_both(e, ref, "done_too", done=True)
    assert sel.tolist() == [False, True, False, True]
    assert (e.results() == latched).all() and e.done().tolist() == [0, 0, 0, 0]
    steps_both(e, ref, cmds[10:20], "second game")
    assert [e.dump(a).hdr.episodes for a in range(A)] == [1, 2, 1, 2]
    assert call_both(e, ref, "done_too again", done=True, seeds_base=900).all()
    assert (e.results() == ref.results()).all()
    steps_both(e, ref, cmds[20:30], "third game")
    e.close(), ref.close()


def test_done_too_after_every_step_is_auto_reset():
    A, steps = 8, 500  # configs[1]: games end at steps 146, 206, 433 and 469 (tests/test_reset_sel_ref.py)
    w1, w0 = config.baseline_workload("C2", arenas=A, auto_reset=1), config.baseline_workload("C2", arenas=A, auto_reset=0)
    tb, sr = w1.seeds()
    auto, e = emu_lib.Emu(w1), EmuSel(w0)
    auto.reset(tb, sr), e.reset(tb, sr)
    cmds, _ = config.bench_commands(A, 1, steps)
    restarts = 0
    for s in range(steps):
        auto.step(cmds[s]), e.step(cmds[s])
        selected = np.zeros((A, 1), dtype=np.uint8)
        e.reset_arenas(done=True, selected=selected)
        assert (selected[:, 0] == auto.done()).all(), s
        restarts += int(selected.sum())
        if selected.any() or s % 25 == 24:  # (a digest or a dump reads the whole state back: not after every step)
            assert (auto.digest() == e.digest()).all(), s
        if selected.any():
            for a in range(A):
                rc.assert_same_state(auto.dump(a), e.dump(a), a, "step %d" % s)
    assert restarts >= 3
    auto.close(), e.close()


def test_with_auto_reset_the_episode_after_a_restart_takes_the_next_seed():
    A = 3
    w = rc.workload("lds-nb1", A, auto_reset=1)
    w.cfg.timer_frames_per_level = 30  # every Timer game ends at frame 31
    w.cfg.reseed_stride = 1000
    tb, sr = w.seeds()
    e, ref = EmuSel(w), ResetSelRef(w, tb, sr)
    e.reset(tb, sr)
    cmds = rc.commands("lds-nb1", A, 1, 50)
    steps_both(e, ref, cmds[:10], "lead")
    sel = call_both(e, ref, "first and last onto seeds of their own", mask=[1, 0, 1], seeds_base=40_000)
    steps_both(e, ref, cmds[10:50], "two games on")
    for a in range(A):
        h = e.dump(a).hdr
        assert h.episodes >= 2
        if sel[a]:  # 40 000 + a, then one stride per game that ended since
            assert (h.tb - (40_000 + a)) % 1000 == 0 and 1 <= (h.tb - (40_000 + a)) // 1000 <= h.episodes
            assert h.serial == 7 * 40_000 + a
    e.close(), ref.close()


def test_refusals():
    w = rc.workload("solo", 2)
    e = EmuSel(w)
    tb8, mask = np.zeros(2, dtype=np.uint64), np.ones(2, dtype=np.uint8)
    assert e.reset_arenas_rc(done=True) == SF_ERR_STATE  # before the first sf_reset
    e.reset(*w.seeds())
    before = e.digest()
    assert e.reset_arenas_rc(tb=tb8) == SF_ERR_ARG and e.reset_arenas_rc(serial=tb8) == SF_ERR_ARG
    assert e.reset_arenas_rc(mask=mask, mask_stride=0) == SF_ERR_ARG and e.reset_arenas_rc(mask=mask, mask_stride=-1) == SF_ERR_ARG
    assert e.reset_arenas_rc(mask_stride=0) == 0  # (no mask: the stride is not looked at)
    assert e.reset_arenas_rc(max_steps=-1) == SF_ERR_ARG
    assert e.L.sfe_reset_arenas(e.h, None) == SF_ERR_ARG
    e.step_begin()
    assert e.reset_arenas_rc(done=True) == SF_ERR_STATE
    e.step_end(np.full((2, 1), ord("+"), dtype=np.uint8))
    after = e.digest()
    stream = np.frombuffer(b"++", dtype=np.uint8)
    off = np.array([0, 1, 2], dtype=np.int64)
    assert e.L.sfe_replay_load(e.h, stream.ctypes.data, off.ctypes.data) == 0
    assert e.reset_arenas_rc(mask=mask) == SF_ERR_STATE  # while a replay is loaded
    assert e.L.sfe_replay_load(e.h, None, None) == 0
    assert (e.digest() == after).all() and (after != before).any()
    assert e.reset_arenas_rc(mask=mask) == 0
    e.close()
