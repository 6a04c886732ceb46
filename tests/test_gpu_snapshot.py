"""sf_snapshot_* and sf_policy_memory_rows on the MI355X (k_snapshot, k_memory_rows) against the restatement over the oracle
(tests/snapshot_ref.py), bit for bit: no tolerance anywhere.

After every call the digests, done flags and full dumps of every arena equal the restatement's; arenas and slots that take no
part are compared with what they held before (slots through sf_snapshot_export, over sentinel-filled snapshots).  The
scenarios shared with the emulator flavour are in tests/snapshot_cases.py."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import reset_sel_cases as rc
import snapshot_cases as sc
from oracle_lib import ArenaDump
from snapshot_ref import SnapshotRef
from strikeforce_amd import abi, config, env

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SF_ERR_ARG, SF_ERR_STATE = -1, -4


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Gpu(env.ArenaBatch):
    """ArenaBatch with the engine surface of tests/snapshot_cases.py (dumps as oracle_lib.ArenaDump)."""

    def dump(self, a):
        return ArenaDump(*self.dump_raw(a))


def start(name, arenas, lead, slots, auto_reset=0, tweak=None):
    w = rc.workload(name, arenas, auto_reset=auto_reset)
    if tweak:
        tweak(w.cfg)
    tb, sr = w.seeds()
    g, ref = Gpu(w), SnapshotRef(w, tb, sr, slots)
    g.reset(tb, sr)
    cmds = rc.commands(name, arenas, w.cfg.n_agents, lead + 200)
    if lead:
        d = dev(cmds[:lead])
        g.step_device(d.data_ptr(), lead)
        g.synchronize()
        for s in range(lead):
            ref.step(cmds[s])
    return w, g, ref, g.snapshot(slots), cmds[lead:]


def fill_with_sentinels(g, snap):
    """Every slot a blob of sentinel bytes: slot 0 is saved once for a valid header."""
    snap.save(sc.idx([0] + [-1] * (g.cfg.arenas - 1)))
    blob = sc.sentinel_blob(snap.export(0))
    for s in range(snap.slots):
        snap.import_(s, blob)
    return blob


# ---- 1. round trip -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", rc.FAMILIES)
def test_round_trip_of_every_instance_family(name):
    A = 3
    if name != "zl":
        w, g, ref, snap, cmds = start(name, A, 30, slots=A)
        sc.compare_all(g, ref, "before the save")
        sc.round_trip(g, ref, snap, cmds[:20], 20, name)
        snap.close(), g.close(), ref.close()
        return
    # large pools: the save before and the load after the tables pass slot 64 (asserted from the oracle), both directions
    w, g, ref, snap, _ = start(name, A, 0, slots=2 * A)
    cmds = rc.commands(name, A, w.cfg.n_agents, rc.ZL_STEPS + 10)
    for a in range(A):
        z, p = rc.large_pool_reach(ref.dump(a))
        assert z < 64 and p < 64, (a, z, p)
    small = g.digest()
    sc.save_both(g, snap, ref, list(range(A)), "the small states")
    lead = rc.ZL_STEPS
    d = dev(cmds[:lead])
    g.step_device(d.data_ptr(), lead)
    g.synchronize()
    for s in range(lead):
        ref.step(cmds[s])
    for a in range(A):
        z, p = rc.large_pool_reach(ref.dump(a))
        assert z >= 64 and p >= 64, (a, z, p)
    big = g.digest()
    sc.save_both(g, snap, ref, [A + a for a in range(A)], "the big states")
    assert sc.load_both(g, snap, ref, list(range(A)), "small into big: the words past the first are cleared").all()
    assert (g.digest() == small).all()
    first = []
    for s in range(lead, lead + 10):
        g.step(cmds[s]), ref.step(cmds[s])
        first.append(g.digest())
    sc.compare_all(g, ref, "behind small into big")
    assert sc.load_both(g, snap, ref, [A + a for a in range(A)], "big into small").all()
    assert (g.digest() == big).all()
    sc.steps_both(g, ref, cmds[lead:lead + 10], "behind big into small")
    sc.load_both(g, snap, ref, list(range(A)), "small again")
    for s in range(lead, lead + 10):
        g.step(cmds[s]), ref.step(cmds[s])
        assert (g.digest() == first[s - lead]).all(), s
    snap.close(), g.close(), ref.close()


# ---- 2. selection --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arenas", [1, 3, 65])
@pytest.mark.parametrize("name", ["solo", "b8"])  # n_agents 1 and 8
def test_selections_touch_only_what_they_name(name, arenas):
    A = arenas
    w, g, ref, snap, cmds = start(name, A, 12, slots=A + 1)
    blob = fill_with_sentinels(g, snap)
    at = 0
    for kind in rc.SELECTIONS:
        m = rc.selection(kind, A)
        row = [a + 1 if m[a] else -1 for a in range(A)]  # arena a -> slot a + 1; slot 0 is never named
        ref.slots = [None] * (A + 1)
        for s in range(A + 1):
            snap.import_(s, blob)
        sc.save_both(g, snap, ref, row, "save " + kind)
        for s in range(A + 1):
            got = snap.export(s)
            assert (got == blob) == (s == 0 or not m[s - 1]), (kind, s)  # (a state is never all sentinel bytes)
        sc.steps_both(g, ref, cmds[at:at + 3], "behind save " + kind, dumps_at_end=False)
        at += 3
        for s in range(A + 1):  # the slots nobody named hold a valid state of sentinels: a load from them would show
            if s == 0 or not m[s - 1]:
                ref.slots[s] = None
        took = sc.load_both(g, snap, ref, row, "load " + kind)
        assert (took == (m != 0)).all()
        sc.steps_both(g, ref, cmds[at:at + 3], "behind load " + kind, dumps_at_end=False)
        at += 3
    assert snap.status() == (0, 0)
    snap.close(), g.close(), ref.close()


# ---- 3. fork -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,arenas", [("lds-nb1", 65), ("b8", 3)])
def test_fork_of_one_slot_into_every_arena(name, arenas):
    A = arenas
    w, g, ref, snap, cmds = start(name, A, 25, slots=1)
    sc.save_both(g, snap, ref, [-1] * (A - 1) + [0], "the last arena")
    assert sc.load_both(g, snap, ref, [0] * A, "into all").all()
    assert len(set(g.digest().tolist())) == 1
    n = w.cfg.n_agents
    for s in range(50):  # equal commands: the last arena's row for everybody
        row = np.repeat(cmds[s, A - 1:A], A, axis=0).reshape(A, n)
        g.step(row), ref.step(row)
        d = g.digest()
        assert len(set(d.tolist())) == 1 and (d == ref.digest()).all(), s
    sc.steps_both(g, ref, cmds[50:80], "each fork on commands of its own")
    assert len(set(g.digest().tolist())) > 1
    snap.close(), g.close(), ref.close()


def test_forks_with_auto_reset_restart_on_the_sources_seed_sequence():
    """configs[1] with auto_reset, eight arenas: arena 0's game ends at step 146 (tests/test_reset_sel_ref.py).  Forked at
    step 100 into all eight, each fork on commands of its own, seven of the eight forks have restarted by step 260 (worked
    out from the oracle on the CPU; asserted below from the restatement before the device's state is looked at).  Every
    restart takes the SOURCE's tb plus one stride per game, and the generator warmed before the save (rng2) is the one
    the restart uses."""
    A, lead, steps, src = 8, 100, 170, 0
    w = config.baseline_workload("C2", arenas=A, auto_reset=1)
    w.cfg.reseed_stride = 1000
    tb, sr = w.seeds()
    g, ref = Gpu(w), SnapshotRef(w, tb, sr, 1)
    snap = g.snapshot(1)
    g.reset(tb, sr)
    cmds, _ = config.bench_commands(A, 1, lead + steps)
    sc.steps_both(g, ref, cmds[:lead], "lead", dumps_at_end=False)
    sc.save_both(g, snap, ref, [0 if a == src else -1 for a in range(A)], "the source")
    before = ref.episodes().copy()
    assert sc.load_both(g, snap, ref, [0] * A, "fork").all()
    assert (ref.episodes() == before).all()  # each destination's own count
    for s in range(lead, lead + steps):
        g.step(cmds[s]), ref.step(cmds[s])
        assert (g.digest() == ref.digest()).all(), s
    assert ((ref.episodes() > before).sum() >= 7)
    sc.compare_all(g, ref, "after the restarts")
    for a in range(A):
        h = g.dump(a).hdr
        assert h.tb == int(tb[src]) + 1000 * (h.episodes - before[a]) and h.serial == int(sr[src]), (a, h.tb)
    snap.close(), g.close(), ref.close()


# ---- 4. records survive ----------------------------------------------------------------------------------------------------------

def test_episode_log_ring_latch_and_ordinals_survive_a_load():
    A, depth = 5, 8

    def short_timer(cfg):
        cfg.timer_frames_per_level = 30  # every Timer game ends at frame 31 unless the player dies first
        cfg.reseed_stride = 1000

    w = rc.workload("lds-nb1", A, auto_reset=1)
    short_timer(w.cfg)
    tb, sr = w.seeds()
    g, ref = Gpu(w), SnapshotRef(w, tb, sr, 2)
    snap = g.snapshot(2)
    g.enable_episode_log(depth)
    g.reset(tb, sr)
    cmds = rc.commands("lds-nb1", A, 1, 100)
    sc.steps_both(g, ref, cmds[:10], "lead", dumps_at_end=False)
    sc.save_both(g, snap, ref, [0, -1, -1, -1, 1], "early states of the first and the last arena")
    sc.steps_both(g, ref, cmds[10:50], "games", dumps_at_end=False)
    ended = ref.episodes().copy()
    assert (ended >= 1).all()
    ring, latch = g.episode_ring(), g.results()
    sc.load_both(g, snap, ref, [-1, 0, 1, 0, -1], "the early states into the middle arenas")
    assert (g.episode_ring() == ring).all() and (g.results() == latch).all()
    assert (ref.episodes() == ended).all() and [g.dump(a).hdr.episodes for a in range(A)] == ended.tolist()
    recs, (written, lost, pending) = g.episodes()  # nothing was delivered before the load: it all still is
    d = env.decode_episodes(recs, 1)
    assert (written, lost, pending) == (int(ended.sum()), 0, 0)
    for a in range(A):
        assert d["episode"][d["arena"] == a].tolist() == list(range(ended[a]))
    sc.steps_both(g, ref, cmds[50:100], "games after the load", dumps_at_end=False)
    recs, (written, lost, pending) = g.episodes()
    d = env.decode_episodes(recs, 1)
    now = ref.episodes()
    assert (now > ended).all() and written == int((now - ended).sum())
    for a in range(A):
        assert d["episode"][d["arena"] == a].tolist() == list(range(ended[a], now[a]))  # the ordinals go on
    assert (g.results() == ref.results()).all()
    snap.close(), g.close(), ref.close()


# ---- 5. bad indices --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arenas", [1, 65])
def test_bad_indices_change_nothing_and_are_counted(arenas):
    w, g, ref, snap, cmds = start("solo", arenas, 10, slots=3)
    sc.save_both(g, snap, ref, [0] + [-1] * (arenas - 1), "slot 0 filled")
    sc.bad_indices(g, ref, snap, "solo")
    sc.steps_both(g, ref, cmds[:5], "on")
    snap.close(), g.close(), ref.close()


# ---- 6. checkpoint ---------------------------------------------------------------------------------------------------------------

def test_checkpoint_into_another_environment():
    A, B = 5, 3
    w = rc.workload("lds-nb1", A)
    w.cfg.reseed_stride = 64
    tb, sr = w.seeds()
    g, ref = Gpu(w), SnapshotRef(w, tb, sr, A)
    snap = g.snapshot(A)
    g.reset(tb, sr)
    cmds = rc.commands("lds-nb1", A, 1, 90)
    sc.steps_both(g, ref, cmds[:30], "lead", dumps_at_end=False)
    sc.save_both(g, snap, ref, list(range(A)), "all")
    originals = g.digest()
    blobs = [snap.export(s) for s in range(A)]
    snap.close(), g.close()
    w2 = rc.workload("lds-nb1", B)
    w2.cfg.reseed_stride = 64
    g2 = Gpu(w2)
    g2.reset(*w2.seeds(base_tb=5_000_000, serial=77))
    snap2 = g2.snapshot(B)
    pick = [4, 0, 2]
    for s, a in enumerate(pick):
        snap2.import_(s, blobs[a])
    snap2.load(sc.idx([0, 1, 2]))
    assert (g2.digest() == originals[pick]).all()
    for s in range(30, 80):
        ref.step(cmds[s])
        g2.step(cmds[s][pick])
        assert (g2.digest() == ref.digest()[pick]).all(), s
    for i, a in enumerate(pick):
        assert sc.without_episodes(g2.dump(i)) == sc.without_episodes(ref.dump(a)), a
    # blobs of an environment with another map, level or auto_reset are refused, and the slot is unchanged
    held = snap2.export(0)

    def other(change):
        wo = rc.workload("lds-nb1", 1)
        wo.cfg.reseed_stride = 64
        change(wo)
        go = Gpu(wo)
        go.reset(*wo.seeds())
        so = go.snapshot(1)
        so.save(sc.idx([0]))
        b = so.export(0)
        so.close(), go.close()
        return b

    def other_map(wo):
        i = wo._map.raw.rindex(b".")  # (the workload owns the buffer cfg.map points into)
        wo._map[i] = b"#"

    def other_level(wo):
        wo.cfg.level = 2

    def other_auto_reset(wo):
        wo.cfg.auto_reset = 1

    for change in (other_map, other_level, other_auto_reset):
        b = other(change)
        assert len(b) == len(held)
        with pytest.raises(env.StrikeForceError, match="configuration"):
            snap2.import_(0, b)
        assert snap2.export(0) == held, change.__name__
    for bad in (held[:-1], b"XFSN" + held[4:], held[:4] + b"\x07" + held[5:], held[:8] + bytes([held[8] ^ 1]) + held[9:]):
        with pytest.raises(env.StrikeForceError):
            snap2.import_(0, bad)
        assert snap2.export(0) == held
    snap2.close(), g2.close(), ref.close()


# ---- 7. stream order -------------------------------------------------------------------------------------------------------------

def test_save_step_load_step_on_a_stream_of_its_own_without_synchronisation():
    A = 65
    w = rc.workload("solo", A)
    tb, sr = w.seeds()
    g, twin = Gpu(w), Gpu(rc.workload("solo", A))
    g.reset(tb, sr), twin.reset(tb, sr)
    sg, st = g.snapshot(A), twin.snapshot(A)
    cmds = rc.commands("solo", A, 1, 60)
    d_cmds = dev(cmds)
    d_all = dev(np.arange(A, dtype=np.int32))
    d_back = dev(np.array([(a * 7) % A if a % 3 else -1 for a in range(A)], dtype=np.int32))  # a permutation with holes
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    g.set_stream(stream.cuda_stream)
    g.step_device(d_cmds[:20].data_ptr(), 20)
    sg.save(d_all)
    g.step_device(d_cmds[20:40].data_ptr(), 20)
    sg.load(d_back.data_ptr())
    g.step_device(d_cmds[40:].data_ptr(), 20)
    g.synchronize()
    twin.step_device(d_cmds[:20].data_ptr(), 20)
    twin.synchronize()
    st.save(d_all)
    twin.synchronize()
    twin.step_device(d_cmds[20:40].data_ptr(), 20)
    twin.synchronize()
    st.load(d_back.data_ptr())
    twin.synchronize()
    twin.step_device(d_cmds[40:].data_ptr(), 20)
    twin.synchronize()
    assert (g.digest() == twin.digest()).all()
    for a in (0, 1, 2, A - 1):
        rc.assert_same_state(twin.dump(a), g.dump(a), a, "stream")
    assert sg.status() == (0, 0)
    g.set_stream(None)
    sg.close(), st.close(), g.close(), twin.close()


# ---- 8. closed loop, network memory ------------------------------------------------------------------------------------------------

CAP = 2048


class Loop:
    """observe_sparse -> predict_sparse -> reward_sparse -> step on one stream, every tick's outputs kept on the device."""

    def __init__(self, g, agents):
        self.g, self.agents = g, agents
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        self.keys, self.vals = z((agents, CAP), torch.int32), z((agents, CAP), torch.float32)
        self.counts, self.pov = z(agents, torch.int32), z((agents, 160), torch.float32)
        self.dense = z((agents, 32, 31, 31), torch.float32)
        self.probs, self.value, self.cmd = z((agents, 9), torch.float32), z(agents, torch.float32), z(agents, torch.uint8)
        self.action, self.reward = z(agents, torch.int32), z(agents, torch.float32)

    def tick(self, net, rew, seed):
        lists = (self.keys.data_ptr(), self.vals.data_ptr(), self.counts.data_ptr(), self.pov.data_ptr(), CAP)
        self.g.observe_sparse_device(*lists)
        self.g.observe_overflow_device(self.counts.data_ptr(), CAP, self.dense.data_ptr(), self.pov.data_ptr())
        net.predict_sparse(*lists, self.agents, self.probs.data_ptr(), self.value.data_ptr(), self.cmd.data_ptr(), seed=seed,
                           d_action_ptr=self.action.data_ptr(), d_dense_ptr=self.dense.data_ptr())
        rew.reward_sparse(*lists, self.agents, self.action.data_ptr(), d_reward_ptr=self.reward.data_ptr(),
                          d_dense_ptr=self.dense.data_ptr())
        self.g.step_device(self.cmd.data_ptr(), 1)
        net.synchronize(), rew.synchronize(), self.g.synchronize()
        return [x.cpu().numpy().copy() for x in (self.action, self.probs, self.value, self.reward)] + [self.g.digest()]


def test_closed_loop_resumes_bit_for_bit_from_a_save_of_game_and_network_memory():
    """Policy, reward model and game are saved at tick t, run 20 ticks, are loaded back and run the same 20 ticks again:
    actions, probabilities, values, rewards and digests repeat.  The draw of an action is a hash of (seed, agent, the
    object's draw ordinal), and the ordinal is not memory: the second pass runs on a policy object of its own whose ordinal
    was brought to t by t sf_policy_act calls, its memory coming from the rows alone."""
    from strikeforce_amd import policy
    A, t, more = 5, 6, 20
    w = rc.workload("b8", A)
    n = w.cfg.n_agents
    agents = A * n
    g = Gpu(w)
    g.reset(*w.seeds())
    params = policy.init_parameters(seed=5)
    net, net2, rew = policy.PolicyBatch(params, agents), policy.PolicyBatch(params, agents), policy.RewardBatch(params, agents)
    loop = Loop(g, agents)
    for i in range(t):
        loop.tick(net, rew, 1234)
        net2.act(loop.probs.data_ptr(), agents, loop.cmd.data_ptr(), seed=1234)  # (only its ordinal matters)
    snap = g.snapshot(A)
    rows = dev(np.arange(agents, dtype=np.int32))
    h = [torch.full((agents, 2, 160), 7.0, device="cuda") for _ in range(2)]
    act = [torch.full((agents, 9), 7.0, device="cuda") for _ in range(2)]
    snap.save(np.arange(A, dtype=np.int32))
    net.memory_rows(True, h[0].data_ptr(), act[0].data_ptr(), rows.data_ptr(), agents)
    rew.memory_rows(True, h[1].data_ptr(), act[1].data_ptr(), rows.data_ptr(), agents)
    first = [loop.tick(net, rew, 1234) for _ in range(more)]
    assert any((first[i][4] != first[0][4]).any() for i in range(1, more))
    snap.load(np.arange(A, dtype=np.int32))
    net2.memory_rows(False, h[0].data_ptr(), act[0].data_ptr(), rows.data_ptr(), agents)
    rew.memory_rows(False, h[1].data_ptr(), act[1].data_ptr(), rows.data_ptr(), agents)
    for i in range(more):
        got = loop.tick(net2, rew, 1234)
        for x, y, what in zip(got, first[i], ("actions", "probabilities", "values", "rewards", "digests")):
            assert x.tobytes() == y.tobytes(), (i, what)
    for x in (snap, net, net2, rew, g):
        x.close()


@pytest.mark.parametrize("agents", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind", ["policy", "reward"])
def test_memory_rows_against_get_memory(agents, kind):
    from strikeforce_amd import policy
    params = policy.init_parameters(seed=2)
    pb = (policy.PolicyBatch if kind == "policy" else policy.RewardBatch)(params, agents)
    r = np.random.RandomState(agents)
    mem = [(r.standard_normal((2, policy.HIDDEN)).astype(np.float32), r.standard_normal(policy.ACTIONS).astype(np.float32))
           for _ in range(agents)]
    for i, (hh, a) in enumerate(mem):
        pb.set_memory(i, hh, a)
    rows = agents + 2
    # agent g -> row (agents - 1 - g) + 1; every fifth agent takes no part, by -1 or by an index out of range
    bad = [-1, rows, -2, sc.I32_MIN, sc.I32_MAX]
    row_of = np.array([bad[(g // 5) % 5] if g % 5 == 4 else agents - g for g in range(agents)], dtype=np.int32)
    d_row = dev(row_of)
    d_h, d_a = torch.full((rows, 2, 160), 7.0, device="cuda"), torch.full((rows, 9), 7.0, device="cuda")
    pb.memory_rows(True, d_h.data_ptr(), d_a.data_ptr(), d_row.data_ptr(), rows, agents)
    pb.synchronize()
    hh, aa = d_h.cpu().numpy(), d_a.cpu().numpy()
    named = {int(x): g for g, x in enumerate(row_of) if 0 <= x < rows}
    for row in range(rows):
        if row in named:
            assert (hh[row] == mem[named[row]][0]).all() and (aa[row] == mem[named[row]][1]).all(), row
        else:
            assert (hh[row] == 7.0).all() and (aa[row] == 7.0).all(), row
    # back: every agent that takes part reads row 1 (the last agent's, or agent 0's own if it is alone): a fork
    fork = np.where((row_of >= 0) & (row_of < rows), 1, row_of).astype(np.int32)
    d_fork = dev(fork)
    pb.memory_rows(False, d_h.data_ptr(), d_a.data_ptr(), d_fork.data_ptr(), rows, agents)
    pb.synchronize()
    seven = (np.full((2, policy.HIDDEN), 7.0, dtype=np.float32), np.full(policy.ACTIONS, 7.0, dtype=np.float32))
    src = mem[named[1]] if 1 in named else seven  # (row 1 is nobody's where the last agent takes no part)
    for g in range(agents):
        got_h, got_a = pb.get_memory(g)
        want = src if fork[g] == 1 else mem[g]
        assert (got_h == want[0]).all() and (got_a == want[1]).all(), g
    # refusals: host memory, buffers one element short (allocations of their own: the extent is the allocation's), a
    # misaligned pointer, rows < 1, too many agents, a null buffer
    H = _hip()
    bufs = []

    def alloc(nbytes):
        p = C.c_void_p()
        assert H.hipMalloc(C.byref(p), nbytes) == 0
        bufs.append(p)
        return p.value

    need = (rows * 2 * 160 * 4, rows * 9 * 4, agents * 4)
    ok = [alloc(nb) for nb in need]
    short = [alloc(nb - 4) if nb > 4 else None for nb in need]
    host = np.zeros(rows * 2 * 160, dtype=np.float32)
    torch.cuda.synchronize()
    L = pb.L
    before = [pb.get_memory(g) for g in (0, agents - 1)]

    def call(hp, ap, rp, nrows=rows, n=agents):
        return L.sf_policy_memory_rows(pb.h, 0, C.c_void_p(hp), C.c_void_p(ap), C.c_void_p(rp), nrows, n)

    for k in range(3):
        args = list(ok)
        args[k] = host.ctypes.data
        assert call(*args) == SF_ERR_ARG and b"not device memory" in L.sf_last_error(), k
        if short[k] is not None:
            args[k] = short[k]
            assert call(*args) == SF_ERR_ARG and b"past the end" in L.sf_last_error(), k
        args[k] = ok[k] + 2
        assert call(*args) == SF_ERR_ARG and b"aligned" in L.sf_last_error(), k
        args[k] = None
        assert call(*args) == SF_ERR_ARG, k
    assert call(*ok, nrows=0) == SF_ERR_ARG and call(*ok, n=agents + 1) == SF_ERR_ARG and call(*ok, n=0) == SF_ERR_ARG
    pb.synchronize()
    for g, (hh0, aa0) in zip((0, agents - 1), before):
        got_h, got_a = pb.get_memory(g)
        assert (got_h == hh0).all() and (got_a == aa0).all()
    for p in bufs:
        H.hipFree(p)
    pb.close()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------

def _hip():
    lib = sorted(glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so*")))
    H = C.CDLL(lib[0] if lib else "libamdhip64.so")
    H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    H.hipFree.argtypes = [C.c_void_p]
    return H


def test_refusals_by_state_and_argument():
    A = 3
    w = rc.workload("solo", A)
    g, other = Gpu(w), Gpu(rc.workload("solo", A))
    L = g.L
    h = C.c_void_p()
    assert L.sf_snapshot_create(g.h, 0, C.byref(h)) == SF_ERR_ARG and L.sf_snapshot_create(g.h, -5, C.byref(h)) == SF_ERR_ARG
    assert L.sf_snapshot_create(None, 1, C.byref(h)) == SF_ERR_ARG and L.sf_snapshot_create(g.h, 1, None) == SF_ERR_ARG
    snap = g.snapshot(2)
    d_row = dev(np.array([0, 1, -1], dtype=np.int32))
    save = lambda e, s, p: L.sf_snapshot_save(e, s, C.c_void_p(p))
    load = lambda e, s, p: L.sf_snapshot_load(e, s, C.c_void_p(p))
    for call in (save, load):
        assert call(g.h, snap.h, d_row.data_ptr()) == SF_ERR_STATE  # before the first sf_reset
    g.reset(*w.seeds()), other.reset(*w.seeds())
    before = g.digest()
    for call in (save, load):
        assert call(g.h, snap.h, None) == SF_ERR_ARG and call(g.h, None, d_row.data_ptr()) == SF_ERR_ARG
        assert call(None, snap.h, d_row.data_ptr()) == SF_ERR_ARG
        assert call(other.h, snap.h, d_row.data_ptr()) == SF_ERR_STATE  # another environment's snapshot
    out = (C.c_int32 * 4)()
    assert L.sf_snapshot_status(None, C.byref(out)) == SF_ERR_ARG
    g.step_begin()
    for call in (save, load):
        assert call(g.h, snap.h, d_row.data_ptr()) == SF_ERR_STATE
    g.step_end(np.full((A, 1), ord("+"), dtype=np.uint8))
    after = g.digest()
    g.replay_load(["+"] * A)
    for call in (save, load):
        assert call(g.h, snap.h, d_row.data_ptr()) == SF_ERR_STATE  # while a replay is loaded
    g.replay_load(None)
    with pytest.raises(env.StrikeForceError):
        snap.export(0)  # never saved
    with pytest.raises(ValueError):
        snap.save(np.array([0, 0, -1], dtype=np.int32))  # two arenas into one slot, from a host array
    assert save(g.h, snap.h, d_row.data_ptr()) == 0 and load(g.h, snap.h, d_row.data_ptr()) == 0
    g.synchronize()
    assert (g.digest() == after).all() and (after != before).any() and snap.status() == (0, 0)
    snap.close(), g.close(), other.close()


def test_host_pointers_misaligned_and_short_index_buffers_are_refused_before_any_launch():
    A = 5
    w = rc.workload("solo", A)
    g = Gpu(w)
    g.reset(*w.seeds())
    snap = g.snapshot(A)
    snap.save(np.arange(A, dtype=np.int32))
    g.step(rc.commands("solo", A, 1, 1)[0])
    before = g.digest()
    H = _hip()
    bufs = []

    def alloc(nbytes):
        p = C.c_void_p()
        assert H.hipMalloc(C.byref(p), nbytes) == 0
        bufs.append(p)
        return p.value

    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    host = np.arange(A + 4, dtype=np.int32)
    exact, short, big = alloc(4 * A), alloc(4 * (A - 1)), alloc(4 * A + 64)
    assert H.hipMemcpy(exact, host.ctypes.data, 4 * A, 1) == 0 and H.hipMemcpy(big, host.ctypes.data, 4 * A, 1) == 0
    torch.cuda.synchronize()
    for name in ("sf_snapshot_save", "sf_snapshot_load"):
        call = lambda p: getattr(g.L, name)(g.h, snap.h, C.c_void_p(p))
        assert call(host.ctypes.data) == SF_ERR_ARG and b"not device memory" in g.L.sf_last_error(), name
        assert call(short) == SF_ERR_ARG and b"past the end" in g.L.sf_last_error(), name  # one element short
        assert call(big + 64 + 4) == SF_ERR_ARG and b"past the end" in g.L.sf_last_error(), name  # starts too late
        assert call(big + 2) == SF_ERR_ARG and b"aligned" in g.L.sf_last_error(), name
    g.synchronize()
    assert (g.digest() == before).all()
    assert g.L.sf_snapshot_load(g.h, snap.h, C.c_void_p(exact)) == 0  # the exact extent, ending on the allocation's last byte
    g.synchronize()
    assert (g.digest() != before).all() and snap.status() == (0, 0)
    snap.close(), g.close()
    for p in bufs:
        H.hipFree(p)
