"""sf_reset_arenas on the MI355X (k_reset_sel) against the restatement over the oracle (tests/reset_sel_ref.py), bit for bit.

Every call here hands the library a sentinel-filled d_selected and seed arrays that hold a poison value at every arena that
is not chosen, so a read of them shows up in the state.  After a call the chosen arenas' dumps (all records, `episodes`
included) and phase draws equal the restatement's, the other arenas' dumps and digests are what they were, and the digests
of all arenas equal the restatement's after each of the steps that follow: the restatement's arenas are independent
oracles, so an arena that was not chosen follows the trajectory of one that never saw the call (one test also keeps a twin
environment that never receives it)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import reset_sel_cases as rc
from oracle_lib import ArenaDump
from reset_sel_ref import ResetSelRef, choose
from strikeforce_amd import abi, config, env

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SF_ERR_ARG, SF_ERR_STATE = -1, -4


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def gdump(g, a):
    return ArenaDump(*g.dump_raw(a))


def compare_all(g, ref, what, dumps=True):
    got, want = g.digest(), ref.digest()
    assert (got == want).all(), (what, np.nonzero(got != want)[0])
    if dumps:
        for a in range(g.cfg.arenas):
            rc.assert_same_state(ref.dump(a), gdump(g, a), a, what)


def call_both(g, ref, what, mask=None, stride=1, d_mask=None, done=False, max_steps=0, seeds_base=None):
    """One call on the device and on the restatement, and everything it must leave.  d_mask: a device buffer to pass as
    the mask instead of an upload of `mask` (sf_done_device's output)."""
    A, n = g.cfg.arenas, g.cfg.n_agents
    before = g.digest()
    dumps_before = [gdump(g, a) for a in range(A)]
    hdrs = [ref.hdr(a) for a in range(A)]
    sel = choose(mask, [h.done for h in hdrs], [h.steps for h in hdrs], done, max_steps)
    tb = sr = None
    if seeds_base is not None:
        tb, sr = rc.seeds_for(sel, seeds_base, A)
    if mask is not None and d_mask is None:  # the flags at mask_stride, every byte between them set
        m = np.full((A - 1) * stride + 1, 0 if stride == 1 else 1, dtype=np.uint8)
        m[::stride] = mask
        d_mask = dev(m)
    d_tb, d_sr = (dev(tb), dev(sr)) if tb is not None else (None, None)
    d_sel = dev(np.full((A, n), rc.SENTINEL, dtype=np.uint8))
    g.reset_arenas(mask_ptr=ptr(d_mask), mask_stride=stride, done=done, max_steps=max_steps, tb_ptr=ptr(d_tb),
                   serial_ptr=ptr(d_sr), selected_ptr=ptr(d_sel))
    g.synchronize()
    assert (ref.reset_arenas(mask=mask, done_too=done, max_steps=max_steps, tb=tb, serial=sr) == sel).all()
    assert (d_sel.cpu().numpy() == np.repeat(sel.astype(np.uint8)[:, None], n, axis=1)).all(), what
    after = g.digest()
    assert (after[~sel] == before[~sel]).all(), what
    for a in np.nonzero(~sel)[0]:
        rc.assert_same_state(dumps_before[a], gdump(g, a), a, what + ": not chosen")
    compare_all(g, ref, what)
    draws = g.phase_draws()
    for a in np.nonzero(sel)[0]:
        assert [int(x) for x in draws[a]] == ref.phase_draws(a), (what, a)
    return sel, d_sel


def steps_both(g, ref, cmds, what):
    for s in range(len(cmds)):
        g.step(cmds[s])
        ref.step(cmds[s])
        compare_all(g, ref, "%s, step %d" % (what, s), dumps=False)
    compare_all(g, ref, what + ", after the steps")


def start(name, arenas, lead, auto_reset=0, tweak=None):
    w = rc.workload(name, arenas, auto_reset=auto_reset)
    if tweak:
        tweak(w.cfg)
    tb, sr = w.seeds()
    g, ref = env.ArenaBatch(w), ResetSelRef(w, tb, sr)
    g.reset(tb, sr)
    cmds = rc.commands(name, arenas, w.cfg.n_agents, lead + 60)
    if lead:
        d = dev(cmds[:lead])
        g.step_device(d.data_ptr(), lead)
        g.synchronize()
        for s in range(lead):
            ref.step(cmds[s])
    return w, g, ref, cmds[lead:]


# ---- shapes --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arenas", [1, 3, 5, 65])
@pytest.mark.parametrize("name", ["solo", "b8"])  # n_agents 1 and 8
def test_selections_strides_and_arena_counts(name, arenas):
    """none / all / first / last / alternating by a mask of stride 1, each followed by steps; then the same five with
    mask_stride = n_agents and sf_done_device's output as the mask: the arenas of the pattern are ended with the quit
    command one step before.  40 steps behind the last call."""
    w, g, ref, cmds = start(name, arenas, 12)
    A, n = arenas, w.cfg.n_agents
    at = 0
    for i, kind in enumerate(rc.SELECTIONS):
        m = rc.selection(kind, A)
        sel, _ = call_both(g, ref, "stride 1, " + kind, mask=m, seeds_base=1000 * (i + 1))
        assert (sel == (m != 0)).all()
        steps_both(g, ref, cmds[at:at + 2], "behind " + kind)
        at += 2
    d_done = dev(np.full((A, n), rc.SENTINEL, dtype=np.uint8))
    for i, kind in enumerate(rc.SELECTIONS):
        m = rc.selection(kind, A)
        quit_ = cmds[at].copy()
        at += 1
        quit_[m != 0, w.cfg.ind] = ord("_")
        g.step(quit_), ref.step(quit_)
        assert (ref.done() == m).all(), kind  # what sf_done_device is about to say
        g.done_device(d_done.data_ptr())
        sel, _ = call_both(g, ref, "sf_done_device's output, " + kind, mask=m, stride=n, d_mask=d_done,
                           seeds_base=None if i % 2 else 50_000 + 1000 * i)
        assert (sel == (m != 0)).all()
    steps_both(g, ref, cmds[at:at + 40], "40 steps on")
    g.close(), ref.close()


# ---- every built instance family, every mode ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(set(rc.FAMILIES + rc.MODES)))
def test_each_instance_family_and_mode(name):
    A = 3 if name == "zl" else 5
    w, g, ref, cmds = start(name, A, rc.ZL_STEPS if name == "zl" else 30)
    if name == "zl":  # on the CPU, through the oracle: the game that is cut had more than 64 zombie slots and exits in use
        for a in range(A):
            z, p = rc.large_pool_reach(ref.dump(a))
            assert z >= 64 and p >= 64, (a, z, p)
    compare_all(g, ref, "before the call")
    call_both(g, ref, "alternating", mask=rc.selection("alternating", A), seeds_base=7000)
    steps_both(g, ref, cmds[:40], "40 steps on")
    sel, _ = call_both(g, ref, "max_steps 41 and the next seed", max_steps=41)
    assert not sel[::2].any()  # (the restarted arenas have played 40 steps)
    call_both(g, ref, "all", mask=rc.selection("all", A), seeds_base=9000)
    steps_both(g, ref, cmds[40:50], "10 steps on")
    g.close(), ref.close()


def test_an_arena_not_chosen_follows_a_twin_that_never_got_the_call():
    A = 5
    w, g, ref, cmds = start("lds-nb1", A, 20)
    twin = env.ArenaBatch(rc.workload("lds-nb1", A))
    twin.reset(*w.seeds())
    lead = rc.commands("lds-nb1", A, 1, 20)
    for s in range(20):
        twin.step(lead[s])
    sel, _ = call_both(g, ref, "first and last", mask=[1, 0, 0, 0, 1], seeds_base=300)
    for s in range(40):
        g.step(cmds[s]), twin.step(cmds[s])
        a, b = g.digest(), twin.digest()
        assert (a[~sel] == b[~sel]).all() and (a[sel] != b[sel]).all(), s
    for a in np.nonzero(~sel)[0]:
        rc.assert_same_state(gdump(twin, a), gdump(g, a), a, "twin")
    g.close(), twin.close(), ref.close()


# ---- episode log --------------------------------------------------------------------------------------------------------------

def _short_timer(cfg):
    cfg.timer_frames_per_level = 30  # every Timer game ends at frame 31 unless the player dies first
    cfg.reseed_stride = 1000


def test_episode_log_ring_latch_and_ordinals_survive_the_call():
    A, depth = 5, 8
    w = rc.workload("lds-nb1", A, auto_reset=1)
    _short_timer(w.cfg)
    tb, sr = w.seeds()
    g, ref = env.ArenaBatch(w), ResetSelRef(w, tb, sr)
    g.enable_episode_log(depth)
    g.reset(tb, sr)
    cmds = rc.commands("lds-nb1", A, 1, 90)
    steps_both(g, ref, cmds[:40], "lead")
    ended = ref.episodes().copy()
    assert (ended >= 2).all()
    ring, latch = g.episode_ring(), g.results()
    sel, _ = call_both(g, ref, "alternating", mask=rc.selection("alternating", A), seeds_base=80_000)
    assert (g.episode_ring() == ring).all() and (g.results() == latch).all() and (latch == ref.results()).all()
    assert (ref.episodes() == ended).all()  # the games that were cut are no episodes
    recs, (written, lost, pending) = g.episodes()  # nothing was delivered before the call: it all still is
    d = env.decode_episodes(recs, 1)
    assert (written, lost, pending) == (int(ended.sum()), 0, 0)
    for a in range(A):
        assert d["episode"][d["arena"] == a].tolist() == list(range(ended[a]))
    steps_both(g, ref, cmds[40:90], "games after the call")
    recs, (written, lost, pending) = g.episodes()
    d = env.decode_episodes(recs, 1)
    now = ref.episodes()
    assert (now >= ended + 2).all() and written == int((now - ended).sum())
    for a in range(A):
        mine = d["arena"] == a
        assert d["episode"][mine].tolist() == list(range(ended[a], now[a]))  # the ordinal goes on
        if sel[a]:  # the seed given, then one stride per game
            assert d["tb"][mine].tolist() == [80_000 + a + 1000 * i for i in range(now[a] - ended[a])]
            assert (d["serial"][mine] == 7 * 80_000 + a).all()
    assert (g.results() == ref.results()).all()
    g.close(), ref.close()


# ---- auto_reset ---------------------------------------------------------------------------------------------------------------

def test_done_too_after_every_step_is_auto_reset_on_the_device():
    A, steps = 8, 500  # configs[1]: games end at steps 146, 206, 433 and 469 (tests/test_reset_sel_ref.py)
    w1, w0 = config.baseline_workload("C2", arenas=A, auto_reset=1), config.baseline_workload("C2", arenas=A, auto_reset=0)
    tb, sr = w1.seeds()
    auto, g = env.ArenaBatch(w1), env.ArenaBatch(w0)
    auto.reset(tb, sr), g.reset(tb, sr)
    cmds, _ = config.bench_commands(A, 1, steps)
    d_cmds = dev(cmds)
    d_sel, d_done = dev(np.zeros((steps, A), dtype=np.uint8)), dev(np.zeros((steps, A), dtype=np.uint8))
    marks = {}
    for s in range(steps):
        auto.step_device(d_cmds[s].data_ptr(), 1), g.step_device(d_cmds[s].data_ptr(), 1)
        g.reset_arenas(done=True, selected_ptr=d_sel[s].data_ptr())
        auto.done_device(d_done[s].data_ptr())
        if s % 25 == 24 or s + 1 in (146, 206, 433, 469):
            marks[s] = (auto.digest(), g.digest(), [gdump(auto, a) for a in range(A)], [gdump(g, a) for a in range(A)])
    auto.synchronize(), g.synchronize()
    sel, done = d_sel.cpu().numpy(), d_done.cpu().numpy()
    assert (sel == done).all() and sel.sum() >= 3
    assert set(np.nonzero(sel.any(axis=1))[0].tolist()) <= set(marks)  # every restart was looked at
    for s, (da, dg, xa, xg) in marks.items():
        assert (da == dg).all(), s
        for a in range(A):
            rc.assert_same_state(xa[a], xg[a], a, "step %d" % s)
    auto.close(), g.close()


def test_with_auto_reset_the_episode_after_a_restart_takes_the_next_seed():
    A = 3
    w, g, ref, cmds = start("lds-nb1", A, 10, auto_reset=1, tweak=_short_timer)
    sel, _ = call_both(g, ref, "first and last onto seeds of their own", mask=[1, 0, 1], seeds_base=40_000)
    steps_both(g, ref, cmds[:40], "two games on")
    for a in range(A):
        h = gdump(g, a).hdr
        assert h.episodes >= 2
        if sel[a]:
            assert (h.tb - (40_000 + a)) % 1000 == 0 and 1 <= (h.tb - (40_000 + a)) // 1000 <= h.episodes
            assert h.serial == 7 * 40_000 + a
    g.close(), ref.close()


# ---- stream order -------------------------------------------------------------------------------------------------------------

def test_step_restart_step_on_a_stream_of_its_own_without_synchronisation():
    A = 65
    w = rc.workload("solo", A)
    tb, sr = w.seeds()
    g, twin = env.ArenaBatch(w), env.ArenaBatch(rc.workload("solo", A))
    g.reset(tb, sr), twin.reset(tb, sr)
    cmds = rc.commands("solo", A, 1, 40)
    m = rc.selection("alternating", A)
    ntb, nsr = rc.seeds_for(m != 0, 2000, A)
    d_cmds, d_m, d_tb, d_sr = dev(cmds), dev(m), dev(ntb), dev(nsr)
    d_sel = dev(np.full((A, 1), rc.SENTINEL, dtype=np.uint8))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    g.set_stream(stream.cuda_stream)
    g.step_device(d_cmds[:20].data_ptr(), 20)
    g.reset_arenas(mask_ptr=d_m.data_ptr(), tb_ptr=d_tb.data_ptr(), serial_ptr=d_sr.data_ptr(), selected_ptr=d_sel.data_ptr())
    g.step_device(d_cmds[20:].data_ptr(), 20)
    g.synchronize()
    twin.step_device(d_cmds[:20].data_ptr(), 20)
    twin.synchronize()
    twin.reset_arenas(mask_ptr=d_m.data_ptr(), tb_ptr=d_tb.data_ptr(), serial_ptr=d_sr.data_ptr())
    twin.synchronize()
    twin.step_device(d_cmds[20:].data_ptr(), 20)
    twin.synchronize()
    assert (g.digest() == twin.digest()).all()
    assert (d_sel.cpu().numpy()[:, 0] == m).all()
    for a in (0, 1, A - 1):
        rc.assert_same_state(gdump(twin, a), gdump(g, a), a, "stream")
    g.set_stream(None)
    g.close(), twin.close()


# ---- composition --------------------------------------------------------------------------------------------------------------

def test_selected_resets_the_policy_memory_and_the_rollout_cursor_of_restarted_agents():
    from strikeforce_amd import policy, rollout
    A = 5
    w, g, ref, _ = start("b8", A, 5)
    n = w.cfg.n_agents
    agents = A * n
    pb = policy.PolicyBatch(policy.init_parameters(seed=3), agents)
    fresh = [pb.get_memory(i) for i in (0, agents - 1)]
    r = np.random.RandomState(4)
    mem = [(r.standard_normal((2, policy.HIDDEN)).astype(np.float32), r.standard_normal(policy.ACTIONS).astype(np.float32))
           for _ in range(agents)]
    for i, (h, a) in enumerate(mem):
        pb.set_memory(i, h, a)
    rb = rollout.RolloutBatch(agents, 4, 1, store_states=False)
    tick = dict(probs=dev(np.full((agents, 9), 1 / 9, dtype=np.float32)), value=dev(np.zeros(agents, dtype=np.float32)),
                action=dev(np.zeros(agents, dtype=np.int32)), reward=dev(np.zeros(agents, dtype=np.float32)))
    args = [tick[k].data_ptr() for k in ("probs", "value", "action", "reward")]
    rb.record(*args), rb.record(*args)
    rb.synchronize()
    sel, d_sel = call_both(g, ref, "alternating", mask=rc.selection("alternating", A), seeds_base=600)
    pb.reset_memory(d_sel.data_ptr())
    pb.synchronize()
    rb.record(*args, d_reset_mask_ptr=d_sel.data_ptr())
    rb.synchronize()
    fill = rb.fill().cpu().numpy()
    for i in range(agents):
        h, a = pb.get_memory(i)
        if sel[i // n]:  # a new game: fresh memory, and the tick went into slot 0
            assert (h == fresh[0][0]).all() and (a == fresh[0][1]).all() and fill[i] == 1
        else:
            assert (h == mem[i][0]).all() and (a == mem[i][1]).all() and fill[i] == 3
    assert (fresh[0][0] == fresh[1][0]).all() and (fresh[0][1] == fresh[1][1]).all()
    pb.close(), rb.close(), g.close(), ref.close()


# ---- misuse -------------------------------------------------------------------------------------------------------------------

def _hip():
    lib = sorted(glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so*")))
    H = C.CDLL(lib[0] if lib else "libamdhip64.so")
    H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    H.hipFree.argtypes = [C.c_void_p]
    return H


def _rc(g, **kw):
    sel = abi.ResetSel(kw.get("mask"), kw.get("stride", 1), kw.get("done", 0), kw.get("max_steps", 0), kw.get("tb"),
                       kw.get("serial"), kw.get("selected"))
    return g.L.sf_reset_arenas(g.h, C.byref(sel))


def test_refusals_by_state_and_argument():
    A = 3
    w = rc.workload("solo", A)
    g = env.ArenaBatch(w)
    good = dev(np.zeros(A, dtype=np.uint64))
    assert _rc(g, done=1) == SF_ERR_STATE  # before the first sf_reset
    g.reset(*w.seeds())
    before = g.digest()
    assert _rc(g, tb=good.data_ptr()) == SF_ERR_ARG and _rc(g, serial=good.data_ptr()) == SF_ERR_ARG
    d_m = dev(np.ones(A, dtype=np.uint8))
    assert _rc(g, mask=d_m.data_ptr(), stride=0) == SF_ERR_ARG and _rc(g, mask=d_m.data_ptr(), stride=-3) == SF_ERR_ARG
    assert _rc(g, max_steps=-1) == SF_ERR_ARG
    assert g.L.sf_reset_arenas(g.h, None) == SF_ERR_ARG and g.L.sf_reset_arenas(None, None) == SF_ERR_ARG
    assert (g.digest() == before).all()
    g.step_begin()
    mid = g.digest()
    assert _rc(g, mask=d_m.data_ptr()) == SF_ERR_STATE
    assert (g.digest() == mid).all()
    g.step_end(np.full((A, 1), ord("+"), dtype=np.uint8))
    after = g.digest()
    g.replay_load(["+"] * A)
    assert _rc(g, mask=d_m.data_ptr()) == SF_ERR_STATE  # while a replay is loaded
    g.replay_load(None)
    assert (g.digest() == after).all()
    assert _rc(g, mask=d_m.data_ptr()) == 0
    g.synchronize()
    assert (g.digest() != after).all()
    g.close()


@pytest.mark.parametrize("n_agents_world", ["solo", "b8"])
def test_host_pointers_and_short_buffers_are_refused_before_any_launch(n_agents_world):
    """Each pointer field as host memory, as a device buffer one byte (d_tb / d_serial: one entry) too short for its
    extent, and d_tb / d_serial off their 8-byte alignment: SF_ERR_ARG and no launch — the digests stay.  The exact extent,
    ending on the allocation's last byte, is accepted."""
    A = 5
    w = rc.workload(n_agents_world, A)
    n = w.cfg.n_agents
    g = env.ArenaBatch(w)
    g.reset(*w.seeds())
    g.step(rc.commands(n_agents_world, A, n, 1)[0])
    before = g.digest()
    H = _hip()
    bufs = []

    def alloc(nbytes):
        p = C.c_void_p()
        assert H.hipMalloc(C.byref(p), nbytes) == 0
        bufs.append(p)
        return p.value

    stride = n
    need = {"mask": (A - 1) * stride + 1, "tb": 8 * A, "serial": 8 * A, "selected": A * n}
    host = {k: np.zeros(need[k] + 8, dtype=np.uint8) for k in need}
    ok = {k: alloc(need[k]) for k in need}
    torch.cuda.synchronize()

    def fields(**over):
        f = dict(mask=None, stride=stride, tb=ok["tb"], serial=ok["serial"], selected=None)
        f.update(over)
        return f

    for k in need:
        assert _rc(g, **fields(**{k: host[k].ctypes.data})) == SF_ERR_ARG, k  # host memory
        assert b"not device memory" in g.L.sf_last_error(), k
        short = alloc(need[k] - (8 if k in ("tb", "serial") else 1))
        assert _rc(g, **fields(**{k: short})) == SF_ERR_ARG, k  # too short
        assert b"past the end" in g.L.sf_last_error(), k
        inside = alloc(need[k] + 64)
        assert _rc(g, **fields(**{k: inside + 64 + (8 if k in ("tb", "serial") else 1)})) == SF_ERR_ARG, k  # starts too late
    for k in ("tb", "serial"):
        big = alloc(need[k] + 16)
        assert _rc(g, **fields(**{k: big + 4})) == SF_ERR_ARG, k
        assert b"aligned" in g.L.sf_last_error(), k
    g.synchronize()
    assert (g.digest() == before).all()
    # the exact extents are accepted (a zeroed mask and done_too off: nothing is chosen, d_selected comes back all zero)
    torch.cuda.synchronize()
    H.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    assert H.hipMemset(ok["mask"], 0, need["mask"]) == 0 and H.hipMemset(ok["selected"], 0xA5, need["selected"]) == 0
    assert _rc(g, **fields(mask=ok["mask"], selected=ok["selected"])) == 0
    g.synchronize()
    out = np.zeros(need["selected"], dtype=np.uint8)
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert H.hipMemcpy(out.ctypes.data, ok["selected"], need["selected"], 2) == 0
    assert (out == 0).all() and (g.digest() == before).all()
    g.close()
    for p in bufs:
        H.hipFree(p)
