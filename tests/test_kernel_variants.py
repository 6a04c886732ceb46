"""Every built instance of the step kernels against the oracle, with the bullet pool filled to its top word.

k_reset / k_step / k_step_half are templates over <NB, HP, BM, ZL> (sf_api.hip): bullet words, flag plane in HBM, cell
bitmaps in LDS, zombie / exit tables in LDS.  tests/variant_cases.py holds one armed Battle world per instance and
restates the host's choice (expected_variant); here:
- the restatement is checked against the instance the emulated host actually runs, and the code object is checked for
  instances no case selects (CPU);
- every case runs on the emulated device core in lock-step with the oracle (CPU);
- every case runs on the MI355X: one step per launch, long launches, split steps, the episode log, the observation (-m gpu);
- the launch order (k_rank) at arena counts whose last block of 1024 is partial and reversed (-m gpu).
Every case also asserts what it reached, from the oracle's own state: a live bullet in the top word, the pool full, and
games that ended and restarted."""
import numpy as np
import pytest

import variant_cases as vc
from emu_lib import Emu
from oracle_lib import ArenaDump, Oracle, diff_dumps
from strikeforce_amd import config

CASE_IDS = [c["name"] for c in vc.CASES]
KERNELS = ("k_reset", "k_step", "k_step_half")


def same_state(x, y, a, what):
    """The whole state of arena a (header, every slot of every pool, the cell planes): the oracle's dump x against y."""
    equal = bytes(x.hdr) == bytes(y.hdr) and np.array_equal(x.flags, y.flags) and np.array_equal(x.dmg, y.dmg) and \
        np.array_equal(x.pidx, y.pidx)
    for xs, ys in ((x.humans, y.humans), (x.zombies, y.zombies), (x.bullets, y.bullets), (x.portals, y.portals)):
        equal = equal and len(xs) == len(ys) and all(bytes(p) == bytes(q) for p, q in zip(xs, ys))
    if not equal:
        d = diff_dumps(x.as_dict(), y.as_dict())
        assert d is None, "%s, arena %d: %s" % (what, a, d)


class Reach:
    """What a run reached, read from the oracle's dumps: the highest live bullet slot, the most live bullets at once,
    finished episodes."""

    def __init__(self, case):
        self.case, self.top, self.most = case, -1, 0

    def see(self, d):
        live = [i for i, b in enumerate(d.bullets) if b.alive]
        if live:
            self.top = max(self.top, live[-1])
        self.most = max(self.most, len(live))

    def check(self, o, arenas, full=True):
        B = self.case["B"]
        nb = (B + 63) // 64
        eps = sum(o.dump(a).hdr.episodes for a in range(arenas))
        print("%-16s %s  top bullet slot %3d of %3d, most live %3d, episodes %d"
              % (self.case["name"], vc.variant_name(vc.expected_variant(o.cfg)), self.top, B, self.most, eps))
        assert self.top >= 64 * (nb - 1), "no live bullet in the top word (highest slot %d)" % self.top
        if full:
            assert self.most == B, "the bullet pool never ran dry (%d of %d)" % (self.most, B)
        assert eps > 0, "no game ended and restarted"
        return eps


# ---- the host's choice of instance ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASE_IDS)
def test_each_case_runs_the_instance_it_names(name):
    """The instance the (emulated) host launches for k_reset, k_step and k_step_half is expected_variant's."""
    c = vc.BY_NAME[name]
    w = vc.workload(c, 1)
    e = Emu(w)
    want = vc.expected_variant(w.cfg)
    e.reset(*w.seeds())
    assert e.last_variant("reset") == want
    cmds = vc.commands(1, 2)
    e.step(cmds[0])
    assert e.last_variant("step") == want
    e.step_begin()
    e.step_end(cmds[1])
    assert e.last_variant("step_half") == want
    print("%s: %s" % (name, vc.variant_name(want)))


def test_expected_variant_follows_the_size_thresholds():
    """The restatement at the edges of sf_types.hpp's thresholds, on the emulated host."""
    def cfg(F, N, M, B=64, Z=16, P=8):
        return config.make_config(1, N, M, floors=F, H=2, Z=Z, B=B, P=P)

    edges = [(cfg(1, 128, 96), (1, 0, 1, 0)),          # 12 288 cells: the largest LDS plane
             (cfg(1, 97, 128), (1, 1, 1, 0)),          # 12 416: HBM plane, bitmaps
             (cfg(1, 128, 128), (1, 1, 1, 0)),         # 16 384: the largest map with bitmaps
             (cfg(1, 129, 128), (1, 1, 0, 0)),         # 16 512
             (cfg(1, 32, 32, B=65), (2, 0, 1, 0)),
             (cfg(1, 32, 32, B=129), (3, 0, 1, 0)),
             (cfg(1, 32, 32, B=193), (4, 0, 1, 0)),
             (cfg(1, 32, 32, B=5, Z=65), (4, 0, 1, 1)),  # large pools force four bullet words
             (cfg(1, 32, 32, B=5, P=65), (4, 0, 1, 1)),
             (cfg(1, 32, 32, Z=64, P=64), (1, 0, 1, 0))]
    for c, want in edges:
        assert vc.expected_variant(c) == want, (c.floors, c.rows, c.cols, want)
        m, p = config.synthetic_map(c.rows, c.cols, floors=c.floors)
        e = Emu(config.Workload("edge", c, m, p))
        e.reset(*config.Workload("edge", c, m, p).seeds())
        assert e.last_variant("reset") == want


def test_every_built_instance_has_a_case(tmp_path):
    """Each k_reset / k_step / k_step_half instance in the gfx950 code object is the one some case selects: an instance
    added without a case here turns this red."""
    from test_episode_log_codeobj import kernel_notes, short_name
    from strikeforce_amd import build
    so = build.build(verbose=False)
    built = {short_name(k) for k in kernel_notes(so, str(tmp_path))}
    built = {k for k in built if k.split("<")[0] in KERNELS and not k.endswith("+log")}
    named = {}
    for c in vc.CASES:
        v = vc.variant_name(vc.expected_variant(vc.workload(c, 1).cfg))
        for k in KERNELS:
            named.setdefault(k + v, c["name"])
    for k in KERNELS:
        n = sum(1 for x in built if x.split("<")[0] == k)
        hit = sum(1 for x in built if x.split("<")[0] == k and x in named)
        print("%-12s %d/%d instances covered" % (k, hit, n))
    missing = sorted(built - set(named))
    assert not missing, "instances no case in variant_cases.py selects: %s" % missing
    assert set(named) <= built, sorted(set(named) - built)
    assert len(built) == 3 * 15


# ---- the emulated device core (CPU) ------------------------------------------------------------------------------------------

EMU_ARENAS, EMU_STEPS = 4, 200


@pytest.mark.parametrize("name", CASE_IDS)
def test_emulated_core_against_the_oracle(name):
    """Lock-step: the phase draws of every step, the whole state every 10 steps, digests and results at the end."""
    c = vc.BY_NAME[name]
    A = EMU_ARENAS
    w = vc.workload(c, A)
    o, e = Oracle(w), Emu(w)
    tb, sr = w.seeds()
    o.reset(tb, sr), e.reset(tb, sr)
    cmds = vc.commands(A, EMU_STEPS)
    reach = Reach(c)
    for s in range(EMU_STEPS):
        o.step(cmds[s]), e.step(cmds[s])
        pd = e.phase_draws()
        for a in range(A):
            d = o.dump(a)
            reach.see(d)
            assert o.phase_draws(a) == list(pd[a]), "step %d arena %d: phase draws" % (s, a)
            if s % 10 == 9:
                same_state(d, e.dump(a), a, "step %d" % s)
    assert (o.digest() == e.digest()).all()
    assert (o.results() == e.results()).all() and (o.done() == e.done()).all()
    reach.check(o, A)


# two cases per bullet word count, every plane kind among them
SPLIT_IDS = ["lds-B64", "hbm-B64", "hbm_bm-B128", "lds-B128", "hbm-B192", "hbm_bm-B192", "lds-B256", "hbm-B256-zl"]


@pytest.mark.parametrize("name", SPLIT_IDS)
def test_emulated_split_step_against_the_oracle(name):
    """sf_step_begin + sf_step_end on both sides: digests every step, the whole state every 10."""
    c = vc.BY_NAME[name]
    A, steps = 2, 150
    w = vc.workload(c, A)
    o, e = Oracle(w), Emu(w)
    tb, sr = w.seeds()
    o.reset(tb, sr), e.reset(tb, sr)
    cmds = vc.commands(A, steps)
    for s in range(steps):
        o.step_begin(), e.step_begin()
        o.step_end(cmds[s]), e.step_end(cmds[s])
        assert (o.digest() == e.digest()).all(), "step %d" % s
        assert (o.agent_alive() == e.agent_alive()).all()
        if s % 10 == 9:
            for a in range(A):
                same_state(o.dump(a), e.dump(a), a, "step %d" % s)
    assert e.last_variant("step_half") == vc.expected_variant(w.cfg)
    assert sum(o.dump(a).hdr.episodes for a in range(A)) > 0


# ---- the MI355X ----------------------------------------------------------------------------------------------------------

GPU_ARENAS = 4


def _device(w):
    from strikeforce_amd import env
    return env.ArenaBatch(w)


def _gdump(g, a):
    return ArenaDump(*g.dump_raw(a))


def _dev(cmds):
    import torch
    return torch.from_numpy(np.ascontiguousarray(cmds)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_IDS)
def test_device_one_step_per_launch(name):
    """(a) sf_step: the phase draws and the whole state of every arena after every step."""
    c = vc.BY_NAME[name]
    A, steps = GPU_ARENAS, 120
    w = vc.workload(c, A)
    o, g = Oracle(w), _device(w)
    tb, sr = w.seeds()
    o.reset(tb, sr), g.reset(tb, sr)
    cmds = vc.commands(A, steps)
    reach = Reach(c)
    for s in range(steps):
        o.step(cmds[s]), g.step(cmds[s])
        pd = g.phase_draws()
        for a in range(A):
            d = o.dump(a)
            reach.see(d)
            assert o.phase_draws(a) == [int(x) for x in pd[a]], "step %d arena %d: phase draws" % (s, a)
            same_state(d, _gdump(g, a), a, "step %d" % s)
    assert (o.results() == g.results()).all() and (o.done() == g.done()).all()
    reach.check(o, A, full=False)  # (the pools run dry within the emulator test's 200 steps, not always within 120)
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_IDS)
def test_device_long_launches(name):
    """(b) sf_step_device in launches of 20 and of 50 steps, 300 steps: digests and results after every launch; (c)
    sf_step_begin / sf_step_end (k_step_half) for 60 steps, the whole state after every step."""
    c = vc.BY_NAME[name]
    A, steps = GPU_ARENAS, 300
    w = vc.workload(c, A)
    tb, sr = w.seeds()
    cmds = vc.commands(A, steps)
    d = _dev(cmds)
    n = A * vc.AGENTS
    for k in (20, 50):
        o, g = Oracle(w), _device(w)
        o.reset(tb, sr), g.reset(tb, sr)
        for s0 in range(0, steps, k):
            o.step_many(cmds[s0:s0 + k])
            g.step_device(d.data_ptr() + s0 * n, k)
            assert (o.digest() == g.digest()).all(), "k = %d: digests differ after %d steps" % (k, s0 + k)
            assert (o.results() == g.results()).all() and (o.done() == g.done()).all()
        for a in range(A):
            same_state(o.dump(a), _gdump(g, a), a, "k = %d, end" % k)
        assert sum(o.dump(a).hdr.episodes for a in range(A)) >= A * 2
        g.close()
    o, g = Oracle(w), _device(w)
    o.reset(tb, sr), g.reset(tb, sr)
    for s in range(60):
        o.step_begin(), g.step_begin()
        o.step_end(cmds[s]), g.step_end(cmds[s])
        for a in range(A):
            same_state(o.dump(a), _gdump(g, a), a, "split step %d" % s)
        assert (o.agent_alive() == g.agent_alive()).all()
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_IDS)
def test_device_episode_log(name):
    """(d) The episode log (depth 4) in launches of 50: the rings equal the oracle's after every launch (the +log twin of
    the case's k_step instance)."""
    from episode_log_ref import OracleEpisodes
    c = vc.BY_NAME[name]
    A, steps, depth, k = GPU_ARENAS, 300, 4, 50
    w = vc.workload(c, A)
    g = _device(w)
    g.enable_episode_log(depth)
    tb, sr = w.seeds()
    g.reset(tb, sr)
    o = OracleEpisodes(Oracle(w), tb, sr)
    cmds = vc.commands(A, steps)
    d = _dev(cmds)
    for s0 in range(0, steps, k):
        g.step_device(d.data_ptr() + s0 * A * vc.AGENTS, k)
        for s in range(s0, s0 + k):
            o.step(cmds[s])
        ring, want = g.episode_ring(), o.ring(depth)
        assert (ring == want).all(), (s0, np.argwhere(ring != want)[:5])
    assert o.ended().min() >= 2
    g.close()


def _occupied_in_windows(d, n_agents):
    """Per living agent of dump d: cells of its 31 x 31 window that hold a human, a zombie or a bullet."""
    occ = {(h.f, h.r, h.c) for h in d.humans if h.alive} | {(z.f, z.r, z.c) for z in d.zombies if z.alive} | \
          {(b.f, b.r, b.c) for b in d.bullets if b.ref}
    out = []
    for h in d.humans[:n_agents]:
        if h.alive:
            out.append(sum(1 for (f, r, c) in occ if f == h.f and abs(r - h.r) <= 15 and abs(c - h.c) <= 15))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c["name"] for c in vc.OBS_CASES])
def test_device_observation_with_the_pools_full(name):
    """(e) After the pools fill: the dense observation within 1 ulp of the oracle's, and the list form equal to the dense
    form bit for bit or marked crowded (0xffffffff).  Windows of more than 48 occupied cells (the list's crowded path) and,
    on 64 x 64, of more than 64 (the dense kernel's spill path) are asserted to occur."""
    import torch
    c = vc.BY_NAME[name]
    A, CAP = GPU_ARENAS, 2048
    w = vc.workload(c, A)
    o, g = Oracle(w), _device(w)
    tb, sr = w.seeds()
    o.reset(tb, sr), g.reset(tb, sr)
    B = A * vc.AGENTS
    cmds = vc.commands(A, 200)
    d = _dev(cmds)
    d_obs = torch.zeros((B, 32, 31, 31), dtype=torch.float32, device="cuda")
    keys, vals = torch.zeros((B, CAP), dtype=torch.int32, device="cuda"), torch.zeros((B, CAP), device="cuda")
    counts, pov = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros((B, 160), device="cuda")
    crowd, compared, marked = [], 0, 0
    for s0 in range(0, 200, 20):
        o.step_many(cmds[s0:s0 + 20])
        g.step_device(d.data_ptr() + s0 * B, 20)
        assert (o.digest() == g.digest()).all(), s0
        if s0 < 20:
            continue  # (the pools are filling)
        for a in range(A):
            crowd += _occupied_in_windows(o.dump(a), vc.AGENTS)
        x, y = o.observe().reshape(B, -1), g.observe().reshape(B, -1)
        assert np.array_equal(x == 0, y == 0)
        ulp = np.abs(x.view(np.int32).astype(np.int64) - y.view(np.int32).astype(np.int64)).max()
        assert ulp <= 1, "step %d: max ulp %d" % (s0 + 20, ulp)
        g.observe_device(d_obs.data_ptr())
        g.observe_sparse_device(keys.data_ptr(), vals.data_ptr(), counts.data_ptr(), pov.data_ptr(), CAP)
        g.synchronize()
        obs = d_obs.cpu().numpy().reshape(B, -1)
        assert np.array_equal(obs.view(np.uint32), y.view(np.uint32))
        k, v, n = keys.cpu().numpy().view(np.uint32), vals.cpu().numpy(), counts.cpu().numpy().view(np.uint32)
        for b in range(B):
            nz = np.flatnonzero(obs[b])
            if n[b] == 0xFFFFFFFF:
                assert len(np.unique(nz % 961)) > 48
                marked += 1
                continue
            assert n[b] == len(nz)
            ch, r = np.divmod(nz, 961)
            yy, xx = np.divmod(r, 31)
            assert np.array_equal(k[b, :n[b]], (ch * 9) | (yy << 9) | (xx << 14))
            assert np.array_equal(v[b, :n[b]].view(np.uint32), obs[b][nz].view(np.uint32))
            compared += 1
    crowd = np.array(crowd)
    print("%s: windows > 48 occupied cells %d, > 64 %d (of %d); lists compared %d, marked crowded %d"
          % (name, (crowd > 48).sum(), (crowd > 64).sum(), len(crowd), compared, marked))
    assert (crowd > 48).any()
    if c["plane"] == "lds64":
        assert (crowd > 64).any()
    assert compared > 0
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1024, 1500, 2048, 3500])
def test_launch_order_at_ragged_arena_counts(A):
    """k_rank orders the arenas of launches of >= 8 steps once A >= 1024, every second block of 1024 reversed: with
    A = 1500 and 3500 the last block is partial and reversed (1024 and 2048: controls).  300 steps in launches of 20 and
    of 50 (the order is renewed every 100 steps); every arena's digest against the oracle, which runs the arenas 256 at a
    time with the seeds the whole batch gives them (reseed_stride = A)."""
    chunk, steps = 256, 300
    w = config.baseline_workload("C3", arenas=A)
    cmds, _ = config.bench_commands(A, 1, steps)
    d = _dev(cmds)
    got = {}
    for k in (20, 50):
        g = _device(w)
        g.reset(*w.seeds())
        for s0 in range(0, steps, k):
            g.step_device(d.data_ptr() + s0 * A, k)
        g.synchronize()
        got[k] = g.digest()
        g.close()
    for first in range(0, A, chunk):
        n = min(chunk, A - first)
        wc = config.baseline_workload("C3", arenas=n)
        wc.cfg.reseed_stride = A
        o = Oracle(wc)
        o.reset(*wc.seeds(first_arena=first))
        o.step_many(cmds[:, first:first + n])
        want = o.digest()
        for k in (20, 50):
            bad = np.nonzero(want != got[k][first:first + n])[0]
            assert bad.size == 0, "A = %d, k = %d: arenas %s differ from the oracle" % (A, k, (bad[:8] + first).tolist())
        o.close()
