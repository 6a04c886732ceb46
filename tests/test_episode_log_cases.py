"""What the cases of tests/episode_log_cases.py reach, asserted from the oracle alone (no GPU), before
tests/test_gpu_episode_log_edges.py and tests/test_episode_log_emu.py compare anything the device core wrote: how many
games every arena ends between two collections, what the records of the multi-agent cases carry in the words of agents
other than `ind`, the seeds of the carry case, that the variant worlds are one per built log instance of k_step, and that
the restatement of the collection (episode_log_ref.collect_like_kernel) agrees with the plain list of records."""
import numpy as np
import pytest

import episode_log_cases as ec
import variant_cases as vc
from episode_log_ref import collect_like_kernel
from strikeforce_amd import build, env

ids = lambda cases: [c.name for c in cases]
# every case whose arenas and launches are enough for the six counts (see test_the_exceptions_reach_what_they_can)
FULL_REACH = ec.VARIANTS + ec.WRITERS + ec.COUNTS[2:] + ec.LARGE + [ec.LATE_ON, ec.DEPTH_1, ec.DEPTH_64] + ec.SEEDS
MULTI = ec.VARIANTS + ec.WRITERS + [ec.RESET_WIDE, ec.NO_RESET]


def test_lay_quits_lays_what_it_says():
    c = np.full((12, 3, 4), ord("x"), dtype=np.uint8)
    ec.lay_quits(c, [3, 0, 5], others_at=[None, 7, -1], ind=1)
    q = c == ec.QUIT
    assert np.argwhere(q[:, 0]).tolist() == [[2, 1], [5, 1], [8, 1], [11, 1]]
    assert np.argwhere(q[:, 1]).tolist() == [[7, 0], [7, 2], [7, 3]]
    assert np.argwhere(q[:, 2]).tolist() == [[4, 1], [9, 1]]
    c[:] = ord("x")
    ec.lay_quits(c, [2, 2, 0], ind=0, start=4, stop=9)
    assert np.argwhere(c == ec.QUIT).tolist() == [[5, 0, 0], [5, 1, 0], [7, 0, 0], [7, 1, 0]]


@pytest.mark.parametrize("case", FULL_REACH, ids=ids(FULL_REACH))
def test_games_ended_between_two_collections(case):
    """Per arena and launch: 0, 1, depth - 1, depth, depth + 1 and at least 3 x depth."""
    per = ec.oracle_run(case).per_launch()
    print(case.name, sorted(set(per.reshape(-1).tolist())))
    d = case.depth
    assert {0, 1, d - 1, d, d + 1} <= set(per.reshape(-1).tolist())
    assert per.max() >= 3 * d


def test_the_exceptions_reach_what_they_can():
    """One arena over three launches has three counts and three arenas eight (0 ... 3 x depth among them); without
    auto_reset an arena ends one game or none; the 16-agent rings of depth 64 are filled to be emptied by sf_reset, not to
    be collected: every arena has written some slots and none all 64 (no slot has wrapped)."""
    one, three = (ec.oracle_run(c).per_launch() for c in ec.COUNTS[:2])
    d = ec.COUNT_DEPTH
    assert one.shape == (3, 1) and {d, d + 1, 3 * d} == set(one.reshape(-1).tolist())
    assert three.shape == (3, 3) and {0, d - 1, d, d + 1, 3 * d} == set(three.reshape(-1).tolist())
    assert set(ec.oracle_run(ec.NO_RESET).per_launch().reshape(-1).tolist()) == {0, 1}
    ended = ec.oracle_run(ec.RESET_WIDE).ends[-1]
    assert 1 <= ended.min() and 20 <= ended.max() < 64


@pytest.mark.parametrize("case", MULTI, ids=ids(MULTI))
def test_multi_agent_records_carry_words_of_other_agents(case):
    n = case.workload().cfg.n_agents
    run = ec.oracle_run(case)
    recs = np.concatenate([r for r, _ in run.collections()])  # what the rings still hold behind a launch: what is compared
    other, differ, outcomes = ec.multi_agent_reach(recs, n)
    print("%s: %d records collected of %d, %d with kills or damage of an agent other than 0, %d whose agents differ, "
          "outcomes %s" % (case.name, len(recs), len(run.records()), other, differ, sorted(outcomes)))
    assert n >= 6 and other >= 10 and differ >= other
    assert {ec.SF_DIED, ec.SF_WON} <= outcomes
    # (the record is as wide as claimed: 16 agents are 136 words, more than a wavefront has lanes)
    assert recs.shape[1] == env.EPISODE_HDR_WORDS + 8 * n == (136 if n == 16 else 56)


@pytest.mark.parametrize("case", ec.SEEDS, ids=ids(ec.SEEDS))
def test_seed_case_carries_into_the_high_word(case):
    d = env.decode_episodes(ec.oracle_run(case).records(), 1)
    tb = d["tb"].astype(np.uint64)
    assert int(tb.min()) == (1 << 32) - 3 and int(tb.max()) >= (1 << 32) + 16
    assert ((tb < (1 << 32)).sum() >= 3) and ((tb >= (1 << 32)).sum() >= 10)
    assert (d["serial"].astype(np.uint64) == (1 << 32) + 5).all()
    # an arena whose seed crosses 2^32 from one episode to the next (tb = base + arena + episode, stride 1)
    assert ((tb == (1 << 32) - 1) & (d["arena"] == 0)).any() and ((tb == (1 << 32)) & (d["arena"] == 0)).any()


def test_one_variant_world_per_built_log_instance(tmp_path):
    """A log instance of k_step added later must come with a case."""
    import test_episode_log_codeobj as co
    raw = co.kernel_notes(build.build(verbose=False), str(tmp_path))
    names = [n for n in map(co.short_name, raw) if n.startswith("k_step<") and n.endswith("+log")]
    built = {n[len("k_step"):-len("+log")] for n in names}
    cases = [vc.variant_name(vc.expected_variant(c.workload().cfg)) for c in ec.VARIANTS]
    assert len(set(cases)) == len(cases) == 15
    assert set(cases) == built
    # the baseline-configuration cases run instances that are among them
    for c in ec.WRITERS + ec.COUNTS[:1] + [ec.NO_RESET]:
        assert vc.variant_name(vc.expected_variant(c.workload().cfg)) in built


@pytest.mark.parametrize("case", [ec.VARIANTS[0], ec.WRITERS[0], ec.WRITERS[3], ec.COUNTS[2], ec.LATE_ON, ec.DEPTH_64,
                                  ec.NO_RESET, ec.SEEDS[0]], ids=lambda c: c.name)
def test_restatement_equals_the_plain_list(case):
    """Rings deep enough to lose nothing, nothing cut: collect_like_kernel behind every launch, its cursors carried, gives
    exactly OracleEpisodes.since(); and at the case's own depth it loses what the rings could not hold."""
    run = ec.oracle_run(case)
    cur, parts = run.first.copy(), []
    prev = run.first
    for i, ends in enumerate(run.ends):
        ring = run.o.ring(256, upto=ends)
        recs, (written, lost, pending), cur = collect_like_kernel(ring, ends, cur, 1 << 30)
        assert (lost, pending) == (0, 0) and (cur == ends).all()
        assert (recs == run.o.since(prev, upto=ends)).all() and written == len(recs)
        parts.append(recs)
        prev = ends
    got = np.concatenate(parts)
    got = got[np.lexsort((got[:, 1], got[:, 0]))]
    assert (got == run.records()).all() and len(got) == int((run.ends[-1] - run.first).sum())
    per = run.per_launch()
    for (recs, (written, lost, pending)), p in zip(run.collections(), per):
        assert lost == int(np.maximum(p - case.depth, 0).sum()) and pending == 0
        assert written == int(np.minimum(p, case.depth).sum())


def test_without_auto_reset_an_arena_ends_once():
    run = ec.oracle_run(ec.NO_RESET)
    ended = run.ends[-1]
    assert set(ended.tolist()) == {0, 1} and (ended == 0).sum() >= 3 and (ended == 1).sum() >= 24
    d = env.decode_episodes(run.records(), 6)
    assert (d["episode"] == 0).all() and len(set(d["arena"].tolist())) == len(d["arena"])
    assert (run.per_launch() > 0).any(axis=1).all()  # games end in both launches


def test_log_switched_on_late_starts_between_slots():
    run = ec.oracle_run(ec.LATE_ON)
    d = ec.LATE_ON.depth
    assert ((run.first % d != 0) & (run.first > 0)).sum() >= 4 and (run.first == 0).any()
    ring = run.ring(0)
    for a in range(ec.HIST_ARENAS):
        eps = ring[a, :, 1]
        assert (eps[eps >= 0] >= run.first[a]).all()  # nothing that ended before the log was on
        for e in eps[eps >= 0]:
            assert ring[a, e & (d - 1), 1] == e
    first64 = ec.oracle_run(ec.DEPTH_64).first
    assert (first64 % 64 != 0).all()


@pytest.mark.parametrize("case", ec.COUNTS, ids=ids(ec.COUNTS))
def test_cuts_of_the_arena_count_cases(case):
    """The collections the GPU test makes behind each launch (episode_log_cases.collection_script): every kind of cut the
    arena count allows, the cut inside a k_ep_plan thread's run wherever a thread owns more than one arena, and, behind the
    second launch, records lost that an earlier cut had left undelivered."""
    A = case.workload().cfg.arenas
    script = ec.collection_script(ec.oracle_run(case))
    kinds = [(i, kind) for i, kind, *_ in script]
    want = {"none", "total", "total-1", "all"} | ({"one"} if A > 1 else set()) | ({"between", "inside"} if A >= 5 else set())
    want |= {"run"} if A > 1024 else set()
    assert {k for _, k in kinds} >= want, kinds
    assert ("run" in {k for _, k in kinds}) == (A > 1024)
    for i, kind, mr, recs, (written, lost, pending), _ in script:
        assert written == len(recs) == min(mr, written + pending)
        if kind in ("one", "between", "inside", "run", "total-1"):
            assert pending > 0 and written == mr
        if kind == "total":
            assert pending == 0 and written == mr > 0
    # every arena count: records that the first launch's cuts left pending are overwritten in the second launch
    run = ec.oracle_run(case)
    cur0 = [s for s in script if s[0] == 0][-1][5]  # cursors behind the first launch's cuts
    left = run.ends[0] - cur0
    overwritten = (left > 0) & (run.ends[1] - cur0 > case.depth)
    lost1 = [s for s in script if s[0] == 1][0][4][1]
    assert overwritten.sum() >= (10 if A > 1000 else 1)
    assert lost1 >= int((run.ends[1] - cur0 - case.depth)[overwritten].sum()) > 0
    if A > 1024:
        chunk = ec.plan_chunk(A)
        (mr,) = [s[2] for s in script if s[1] == "run"]
        assert chunk == (A + 1023) // 1024 >= 2 and mr > 0
