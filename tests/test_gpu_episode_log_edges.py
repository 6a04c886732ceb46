"""The episode log on the MI355X where tests/test_gpu_episode_log.py does not go: every k_step<.., LOG> instance of the code
object, records of 6 and of 16 agents (136 words: wider than a wavefront) through all three writers, arena counts at
which a k_ep_plan thread owns several arenas or none and k_ep_copy's last workgroup is not full, collections cut at every
kind of place, and the histories nobody had run (log switched on late, off and on again at depths 1 and 64, no
auto-reset, seeds that carry into the high word).  The cases and their schedules are tests/episode_log_cases.py; what
they reach is asserted from the oracle alone in tests/test_episode_log_cases.py.  Every comparison is integers, bit for
bit: the rings against the oracle's records behind every launch, every collection against the restatement
(episode_log_ref.collect_like_kernel) of the oracle's rings with the cursors carried by the test.

How many records each multi-agent case collects, and how many of them carry kills or damage of an agent other than 0,
is printed by tests/test_episode_log_cases.py -s, which asserts the least of it."""
import numpy as np
import pytest

import episode_log_cases as ec
from episode_log_ref import collect_like_kernel
from strikeforce_amd import env

pytestmark = pytest.mark.gpu
SENTINEL = -0x5a5a5a5b
ids = lambda cases: [c.name for c in cases]


def device_cmds(cmds):
    import torch
    return torch.from_numpy(np.ascontiguousarray(cmds)).cuda()


def advance(g, case, cmds, d, s0, n):
    """Steps s0 ... s0 + n - 1 through the case's writer."""
    if case.writer == "launch":
        g.step_device(d[s0].data_ptr(), n)
        return
    for s in range(s0, s0 + n):
        if case.writer == "step":
            g.step(cmds[s])
        else:
            g.step_begin(), g.step_end(cmds[s])


def start(case, depth=None):
    """The environment of a case in front of its first logged launch: (env, commands, device commands)."""
    g = env.ArenaBatch(case.workload())
    cmds = case.commands()
    d = device_cmds(cmds)
    if case.on_at == 0:
        g.enable_episode_log(depth or case.depth)
    g.reset(*case.seeds())
    if case.on_at:
        advance(g, case, cmds, d, 0, case.on_at)
        g.enable_episode_log(depth or case.depth)
    return g, cmds, d


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert (got == want).all(), (what, np.argwhere(got != want)[:5])


def run_case(case, g=None, cmds=None, d=None, small_first=None):
    """Behind every launch the raw rings equal the oracle's, and a collection gives written, lost and pending and the
    records the restatement gives from the oracle's rings with the cursors the test carries.  small_first: the first
    sf_episodes call of all, behind the first launch, asks for that many records only, and the uncut one follows it.
    Returns the environment."""
    run = ec.oracle_run(case)
    if g is None:
        g, cmds, d = start(case)
    same(g.episode_ring(), run.o.ring(case.depth, upto=run.first), case.name + ": rings when the log comes on")
    cur, got = run.first.copy(), []
    for i, (s0, n) in enumerate(case.launches()):
        advance(g, case, cmds, d, s0, n)
        ring = run.ring(i)
        same(g.episode_ring(), ring, "%s: rings behind launch %d" % (case.name, i))
        for mr in ([small_first, None] if small_first and i == 0 else [None]):
            want, counts, cur = collect_like_kernel(ring, run.ends[i], cur, mr or 1 << 30)
            recs, c = g.episodes(max_records=mr)
            assert c == counts and (mr is None or c[2] > mr == c[0]), (case.name, i, mr, c, counts)
            same(recs[:c[0]], want, "%s: collection behind launch %d" % (case.name, i))
            got.append(recs[:c[0]])
    same(np.concatenate(got), np.concatenate([r for r, _ in run.collections()]), case.name + ": all records")
    assert g.episodes()[1] == (0, 0, 0)
    return g


# ---- a: every log instance of k_step ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.VARIANTS, ids=ids(ec.VARIANTS))
def test_every_log_instance(case):
    """One 16-agent world per k_step<NB, HP, BM, ZL, LOG = true> of the code object, 5 arenas (k_ep_copy's second workgroup
    has one arena), depth 4, eight launches of 40 steps in which an arena ends 0, 1, 3, 4, 5 or 13 games."""
    g = run_case(case)
    # a generic instance ran, no fixed-shape one.  Which one the host picks for these worlds at 5 arenas with the log on
    # is asserted on the emulated host (test_episode_log_emu.py, last_variant == expected_variant for all 15 worlds)
    assert g.step_kernel() == -1
    res = g.results()  # sf_results is each arena's newest record
    run = ec.oracle_run(case)
    for a in range(ec.WIDE_ARENAS):
        assert (run.o.records[a][-1][env.EPISODE_HDR_WORDS:] == res[a].reshape(-1)).all()
    g.close()


# ---- b: the writers at width ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ec.WRITERS, ids=ids(ec.WRITERS))
def test_writers_at_width(case):
    """KITS (6 agents: 56 words) and MAXCAP (16 agents: 136 words, 128 of them agents' words: the copy loop of
    ep_log_late takes a second pass) through sf_step_device, sf_step and sf_step_begin / sf_step_end."""
    run_case(case).close()


def test_reset_empties_wide_rings():
    """sf_reset with the log on: 5 rings of 64 records of 136 words (8704 words each, 136 passes of k_ep_late's emptying
    loop) hold nothing afterwards, and the next game is episode 0."""
    case = ec.RESET_WIDE
    g = run_case(case)
    assert (g.episode_ring()[:, :, 1] >= 0).sum() == int(ec.oracle_run(case).ends[-1].sum())
    g.reset(*case.seeds())
    ring = g.episode_ring()
    assert ring.shape == (ec.WIDE_ARENAS, 64, 136) and (ring == -1).all()
    assert g.episodes()[1] == (0, 0, 0)
    run_case(case, g, case.commands(), device_cmds(case.commands())).close()  # the same history again, from episode 0


# ---- c: arena counts ------------------------------------------------------------------------------------------------------
class DeviceCollector:
    """sf_episodes_device into a buffer filled with a sentinel: (records, counts), and the rows behind `written` intact."""

    def __init__(self, g, rows):
        import torch
        self.g, self.torch = g, torch
        self.out = torch.empty((rows + 3, g.episode_record_words), dtype=torch.int32, device="cuda")
        self.counts = torch.empty(3, dtype=torch.int32, device="cuda")

    def __call__(self, max_records, null_output=False):
        self.out.fill_(SENTINEL), self.counts.fill_(SENTINEL)
        self.torch.cuda.synchronize()
        self.g.episodes_device(0 if null_output else self.out.data_ptr(), max_records, self.counts.data_ptr())
        self.g.synchronize()
        self.torch.cuda.synchronize()
        c = tuple(int(x) for x in self.counts.cpu())
        out = self.out.cpu().numpy()
        assert 0 <= c[0] <= max_records
        assert (out[c[0]:] == SENTINEL).all(), ("rows behind written", max_records, c)
        return out[:c[0]], c


@pytest.mark.parametrize("case", ec.COUNTS, ids=ids(ec.COUNTS))
def test_arena_counts_and_cuts(case):
    """A in {1, 3, 5, 1023, 1025, 2050}: above 1024 a k_ep_plan thread owns 2 or 3 arenas and the last threads none; 1, 3,
    5, 1023, 1025 and 2050 all leave k_ep_copy's last workgroup part empty.  The collections are
    episode_log_cases.collection_script's: max_records 0 with a null output, 1, a cut between two arenas, inside one
    arena's records, inside a thread's run at an arena that is not its first (A > 1024), the total less one, exactly the
    total; records an earlier cut left pending are overwritten by the next launch and counted lost."""
    run = ec.oracle_run(case)
    A = case.workload().cfg.arenas
    g, cmds, d = start(case)
    collect = DeviceCollector(g, A * case.depth)
    script = ec.collection_script(run)
    for i, (s0, n) in enumerate(case.launches()):
        advance(g, case, cmds, d, s0, n)
        same(g.episode_ring(), run.ring(i), "%s: rings behind launch %d" % (case.name, i))
        for li, kind, mr, want, counts, _ in script:
            if li != i:
                continue
            recs, c = collect(mr, null_output=(kind == "none"))
            print(case.name, i, kind, mr, c)
            assert c == counts, (case.name, i, kind, mr, c, counts)
            same(recs, want, "%s: launch %d, %s" % (case.name, i, kind))
    assert collect(A * case.depth)[1] == (0, 0, 0)
    g.close()


def test_above_4096_arenas():
    """4099 arenas (no multiple of 4; five arenas per k_ep_plan thread, thread 819's run cut to four, 204 threads without
    one): the rings of the three runs of ten arenas the oracle is stepped for equal the oracle's.  The collection as a
    whole (offsets of 4099 arenas, a cut inside a thread's run, rows behind `written`) is restated from the device's own
    rings, the cursors carried by the test.  The cut leaves the records behind it pending over the second launch, which
    overwrites some of them: the next collection counts them lost."""
    A, depth, k = ec.LARGE_ARENAS, ec.COUNT_DEPTH, ec.COUNT_K
    w = ec.c1_workload(A)()
    g = env.ArenaBatch(w)
    g.enable_episode_log(depth)
    g.reset(*w.seeds())
    cmds = ec.count_commands(A, 2)
    for c in ec.LARGE:  # (a window's commands are the big run's)
        f = int(c.name.rsplit("-", 1)[1])
        assert (c.commands() == cmds[:, f:f + 10]).all()
    d = device_cmds(cmds)
    collect = DeviceCollector(g, A * depth)
    cur = np.zeros(A, dtype=np.int64)
    for i in range(2):
        g.step_device(d[i * k].data_ptr(), k)
        ring = g.episode_ring()
        episodes = ring[:, :, 1].max(axis=1) + 1  # (log on from the start: newest episode + 1; 0 where the ring is empty)
        for c in ec.LARGE:
            f = int(c.name.rsplit("-", 1)[1])
            want = ec.oracle_run(c).ring(i).copy()
            want[:, :, 0][want[:, :, 0] >= 0] += f  # (the window's arena numbers are the run's less f)
            same(ring[f:f + 10], want, "%s: rings behind launch %d" % (c.name, i))
            assert (episodes[f:f + 10] == ec.oracle_run(c).ends[i]).all()
        if i == 1:  # pending records of the first launch that the second one has overwritten
            overwritten = (first_episodes > cur) & (episodes - cur > depth)
            assert overwritten.sum() > 100
        first_episodes = episodes
        for kind in (["run"] if i == 0 else ["total-1", "all"]):
            mr = A * depth if kind == "all" else ec.cut(kind, episodes, cur, depth, ec.plan_chunk(A))
            assert mr is not None and mr > 0
            want, counts, cur = collect_like_kernel(ring, episodes, cur, mr)
            recs, cnt = collect(mr)
            assert cnt == counts, (i, kind, mr, cnt, counts)
            same(recs, want, "launch %d, %s" % (i, kind))
            if i == 1 and kind == "total-1":
                assert cnt[1] >= int((episodes - first_cur - depth)[overwritten].sum()) > 0
        first_cur = cur.copy()
    g.close()


# ---- d: histories ---------------------------------------------------------------------------------------------------------
def test_log_switched_on_after_games_have_ended():
    """The cursors start at episode counts 12, 5, 4, 3, 1, 0, 2, 12 (sf_host.hpp episode_log): only later games are
    offered, episode e in slot e & 3 from the first one on.  The first sf_episodes call of the environment asks for 3
    records of the 22 pending and the second for all 32 the rings can hold: the host's staging buffer (sf_host.hpp
    episodes_host) is allocated for 3 records, then freed and regrown, and the 19 records of the second call come through
    the regrown one."""
    run_case(ec.LATE_ON, small_first=3).close()


def test_off_and_on_again_at_depths_1_and_64():
    """Depth 1 (every slot index 0; two launches), off, on again at depth 64 with the episode counts the first fifty steps
    left (17, 9, 7, 4, 1, 2, 14, 17): one launch of 384 steps ends 192, 64, 63, 65, 1 and 0 games in an arena."""
    g = run_case(ec.DEPTH_1)
    g.enable_episode_log(0)
    with pytest.raises(env.StrikeForceError):
        g.episodes()
    case = ec.DEPTH_64
    cmds = case.commands()
    assert (cmds[:case.on_at] == ec.DEPTH_1.commands()).all()
    g.enable_episode_log(64)
    run_case(case, g, cmds, device_cmds(cmds)).close()


def test_without_auto_reset():
    """auto_reset = 0 on KITS, 32 arenas: one record per arena that ends its game, nothing pending afterwards, and the
    state stands still under further steps (split steps too: k_ep_late writes nothing new)."""
    case = ec.NO_RESET
    g = run_case(case)
    run = ec.oracle_run(case)
    ring, digest, done = g.episode_ring(), g.digest(), g.done()
    over = run.ends[-1] == 1
    assert (done.astype(bool) == over).all()
    cmds = case.commands()
    for s in range(3):
        g.step(cmds[s])
        g.step_begin(), g.step_end(cmds[s])
    assert (g.digest()[over] == digest[over]).all()
    now = g.episode_ring()
    same(now[over], ring[over], "rings of the arenas that had ended")
    assert (now[:, 1:] == -1).all()  # no arena has a second record
    r, c = g.episodes()
    assert c[1:] == (0, 0) and (len(r) == 0 or not over[r[:, 0]].any())
    g.close()


@pytest.mark.parametrize("case", ec.SEEDS, ids=ids(ec.SEEDS))
def test_seed_carries_into_the_high_word(case):
    """base tb 2^32 - 3, reseed stride 1, serial 2^32 + 5: the per-episode reseed carries from the low into the high word
    (S.tb_lo / S.tb_hi in k_step's header, the 64-bit tb - reseed of ep_log_late behind the split step)."""
    g = run_case(case)
    d = env.decode_episodes(g.episode_ring(), 1)
    tb = d["tb"].astype(np.uint64)[d["episode"] >= 0]
    assert (tb >= (1 << 32)).any() and (tb < (1 << 34)).all()
    g.close()
