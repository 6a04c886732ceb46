"""Games recorded ON THE DEVICE as `.sf_sample` command streams (include/strikeforce.h sf_record_*; csrc/sf_record.hpp):
sf_record_step against the reference client's own files and per-iteration digests (tests/golden/online_*), against the
oracle's plays of tests/record_cases.py, against sf_step_device on a twin environment, and round through sf_replay_step;
the edges of the rules; the collection with limits and on a caller's stream.  Small shapes, at most 120 iterations."""
import ctypes as C

import numpy as np
import pytest

import online_cases as oc
import record_cases as rc
from strikeforce_amd import abi, replay

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -4  # SF_ERR_ARG, SF_ERR_STATE


def _env(workload):
    from strikeforce_amd import env
    return env.ArenaBatch(workload)


def _reset(sim, tb, serial):
    n = len(tb)
    sim.reset((C.c_uint64 * n)(*tb), (C.c_uint64 * n)(*serial))


def _rows(cmds):
    import torch
    return torch.from_numpy(np.ascontiguousarray(cmds, dtype=np.uint8)).cuda()


def _record(p, sim, rec, digests=True):
    """the whole play through sf_record_step; the digest after every iteration is the oracle's"""
    d_cmd = _rows(p.cmds)
    _reset(sim, p.tb, p.serial)
    if digests:
        assert (sim.digest() == p.digests[0]).all()
    for t in range(len(p.cmds)):
        rec.step(d_cmd[t])
        if digests:
            assert (sim.digest() == p.digests[t + 1]).all(), t


# ---- 1. the fixture matches and the 24-match batch -----------------------------------------------------------------------
@pytest.mark.parametrize("name", oc.NAMES)
def test_a_fixture_match_is_recorded_as_the_reference_client_logged_it(name, tmp_path):
    p, s, f = rc.fixture_played(name)
    sim = _env(oc.workload(s, f))
    rec = sim.recorder(3 * 120 + 3, 2)
    d_cmd = _rows(p.cmds)
    _reset(sim, p.tb, p.serial)
    got = ["%016x" % int(sim.digest()[0])]
    for t in range(120):
        rec.step(d_cmd[t])
        got.append("%016x" % int(sim.digest()[0]))
    assert got == f["digests"]  # the reference client's own digests, after every iteration
    assert rec.collect()[2] == dict(zip(abi.RECORD_COUNT_FIELDS, [0] * 6))  # the game is still open
    rec.flush()
    games, data, counts = rec.collect()
    assert rc.delivered_games(games, data) == rc.expected_games(p) and data.tobytes() == s.commands.encode()
    assert counts == dict(games=1, bytes=len(s.commands), games_pending=0, bytes_pending=0, games_lost=0, bytes_substituted=0)
    (made,) = replay.samples_from_recording(games, data, s)
    out = str(tmp_path / "again.sf_sample")
    replay.write_sample(out, made, layout="logged")
    assert open(out, "rb").read() == open(oc.path_of(name), "rb").read()


def test_the_24_match_batch():
    p = rc.batch_played()
    sim = _env(p.w)
    rec = sim.recorder(3 * rc.BATCH_ITERS + 8, 2)
    _record(p, sim, rec)
    ended, ended_data, counts = rec.collect()  # before the flush: exactly the games check_end ended
    assert [int(a) for a in ended[:, 0]] == [a for a, gs in enumerate(p.games) if gs[0]["end"] is not None]
    assert counts["games"] == len(ended) == 4 and counts["games_pending"] == 0
    rec.flush()
    games, data, _ = rec.collect()
    assert sorted(rc.delivered_games(ended, ended_data) + rc.delivered_games(games, data)) == rc.expected_games(p)


# ---- 2. round trip through sf_replay_step ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_recorded_games_replay_to_the_same_states(name):
    p = rc.CASES[name]()
    cfg = p.w.cfg
    sim = _env(p.w)
    rec = sim.recorder(3 * len(p.cmds) + 8, 8)
    _record(p, sim, rec)
    rec.flush()
    games, data, counts = rec.collect()
    got = rc.delivered_games(games, data)
    assert got == rc.expected_games(p)
    assert counts["bytes_substituted"] == p.substituted and counts["games_lost"] == 0
    # a second environment, one arena per recorded game, reset on the recorded seeds, fed the delivered bytes and offsets
    n = len(got)
    second = _env(rc.WORKLOADS[name](n, 0))
    _reset(second, [g[2] for g in got], [g[3] for g in got])
    from strikeforce_amd import env
    off = np.concatenate([env.decode_games(games)["offset"], [len(data)]]).astype(np.int64)
    assert second.L.sf_replay_load(second.h, C.c_void_p(data.ctypes.data), C.c_void_p(off.ctypes.data)) == 0
    first = {(g["arena"], g["episode"]): g["first"] for gs in p.games for g in gs}
    longest = max(g[5] for g in got)
    for it in range(1, longest + 2):
        second.replay_step()
        dg = second.digest()
        for j, g in enumerate(got):
            ended = g[6] == abi.RECORD_GAME_ENDED
            # (under auto_reset the recording arena has restarted behind its last iteration: that state is the next game's)
            if it < g[5] or (it == g[5] and not (ended and cfg.auto_reset)):
                assert int(dg[j]) == int(p.digests[first[(g[0], g[1])] + it, g[0]]), (j, it)
    st = second.replay_status()
    for j, g in enumerate(got):
        want = abi.REPLAY_GAME_ENDED if g[6] == abi.RECORD_GAME_ENDED else abi.REPLAY_SAMPLE_ENDED
        assert st[j].tolist() == [want, g[4], g[5], 0], (j, st[j].tolist(), g[:8])  # never TRUNCATED; cursor == lines
    res = second.results()
    for j, g in enumerate(got):
        if g[6] == abi.RECORD_GAME_ENDED:
            assert res[j, 0, 7] == g[7]


# ---- 3. a twin environment stepped with sf_step_device --------------------------------------------------------------------
@pytest.mark.parametrize("name,auto_reset", [("fight", 0), ("fight", 1), ("solo", 1)])
def test_record_step_is_step_device_of_one_iteration(name, auto_reset):
    p = rc.CASES[name]()
    A = p.w.cfg.arenas
    a, b = _env(rc.WORKLOADS[name](A, auto_reset)), _env(rc.WORKLOADS[name](A, auto_reset))
    a.enable_episode_log(8), b.enable_episode_log(8)
    rec = b.recorder(3 * len(p.cmds) + 8, 8)
    d_cmd = _rows(p.cmds)
    _reset(a, p.tb, p.serial), _reset(b, p.tb, p.serial)
    logged = []
    for t in range(len(p.cmds)):
        a.step_device(d_cmd[t].data_ptr(), 1)
        rec.step(d_cmd[t])
        assert (a.digest() == b.digest()).all(), t
        assert (a.results() == b.results()).all() and (a.done() == b.done()).all(), t
        (ra, ca), (rb, cb) = a.episodes(), b.episodes()
        assert tuple(ca) == tuple(cb) and np.array_equal(ra, rb), t
        logged.append(rb)
    from strikeforce_amd import env
    log = env.decode_episodes(np.concatenate([np.asarray(x, dtype=np.int32).reshape(-1) for x in logged]), p.w.cfg.n_agents)
    by_key = {(int(log["arena"][i]), int(log["episode"][i])): i for i in range(len(log["arena"]))}
    games, data, counts = rec.collect()  # no flush: the games check_end ended, and only those
    d = env.decode_games(games)
    assert len(d["arena"]) == len(by_key) > 0 and (d["end"] == abi.RECORD_GAME_ENDED).all()
    for i in range(len(d["arena"])):
        j = by_key[(int(d["arena"][i]), int(d["episode"][i]))]
        assert (d["iterations"][i], d["outcome"][i]) == (log["steps"][j], log["outcome"][j])
        assert (int(d["tb"][i]), int(d["serial"][i])) == (int(log["tb"][j]), int(log["serial"][j]))
        assert int(d["tb"][i]) == p.tb[d["arena"][i]] + int(d["episode"][i]) * A and int(d["serial"][i]) == p.serial[d["arena"][i]]


# ---- 4. edges ------------------------------------------------------------------------------------------------------------------
def _fight(auto_reset=0, arenas=4):
    p = rc.fight_played()
    sim = _env(rc.batch_workload(arenas, auto_reset))
    _reset(sim, p.tb[:arenas], p.serial[:arenas])
    return p, sim, _rows(p.cmds[:, :arenas])


def _summary(games):
    return [tuple(int(x) for x in g[[0, 1, 6, 7, 8]]) for g in games]  # arena, episode, lines, iterations, end


def test_overflow_keeps_whole_iterations():
    p, sim, d_cmd = _fight()
    rec = sim.recorder(2 * 3, 2)
    for t in range(5):
        rec.step(d_cmd[t])
    games, data, counts = rec.collect()
    assert _summary(games) == [(a, 0, 6, 2, abi.RECORD_OVERFLOW) for a in range(4)]
    assert data.tobytes() == b"".join(bytes(p.games[a][0]["stream"][:6]) for a in range(4))
    assert (sim.digest() == p.digests[5, :4]).all()  # the environment plays on
    rec.flush()
    assert rec.collect()[2]["games"] == 0  # nothing is open: an arena records again only from its next first iteration


def test_broken_after_another_entry_point_and_after_a_snapshot_load():
    p, sim, d_cmd = _fight()
    rec = sim.recorder(256, 4)
    snap = sim.snapshot(1)
    for t in range(3):
        rec.step(d_cmd[t])
    snap.save([-1, -1, 0, -1])
    sim.step_device(d_cmd[3].data_ptr(), 1)  # every arena is one iteration ahead of its game
    rec.step(d_cmd[4])
    games, _, _ = rec.collect()
    assert _summary(games) == [(a, 0, 9, 3, abi.RECORD_BROKEN) for a in range(4)]
    assert (sim.digest() == p.digests[5, :4]).all()
    # a fresh game in arena 2 only (a masked restart), then a load of its earlier state under the open game
    import torch
    mask = torch.tensor([0, 0, 1, 0], dtype=torch.uint8, device="cuda")
    sim.reset_arenas(mask_ptr=mask.data_ptr())
    for t in range(5, 9):
        rec.step(d_cmd[t])
    snap.load([-1, -1, 0, -1])  # steps 3 where the open game has 4
    rec.step(d_cmd[9])
    rec.flush()
    games, _, _ = rec.collect()
    assert _summary(games) == [(2, 0, 12, 4, abi.RECORD_BROKEN)]
    snap.close()


def test_cut_and_a_new_game_after_reset_arenas_and_flush():
    p, sim, d_cmd = _fight(auto_reset=1)
    rec = sim.recorder(256, 4)
    for t in range(4):
        rec.step(d_cmd[t])
    import torch
    mask = torch.tensor([0, 1, 0, 0], dtype=torch.uint8, device="cuda")
    sim.reset_arenas(mask_ptr=mask.data_ptr())
    for t in range(4, 6):
        rec.step(d_cmd[t])
    games, _, counts = rec.collect()
    assert _summary(games) == [(1, 0, 12, 4, abi.RECORD_CUT)] and counts["games_pending"] == 0
    rec.flush()
    games, data, _ = rec.collect()
    assert _summary(games) == [(0, 0, 18, 6, abi.RECORD_CUT), (1, 0, 6, 2, abi.RECORD_CUT), (2, 0, 18, 6, abi.RECORD_CUT),
                               (3, 0, 18, 6, abi.RECORD_CUT)]
    from strikeforce_amd import env
    d = env.decode_games(games)
    assert int(d["tb"][1]) == p.tb[1] + 4 and int(d["tb"][0]) == p.tb[0]  # the restart's seed: tb + reseed stride
    assert data[18:24].tobytes() == bytes(int(p.cmds[t, 1, g]) for t in (4, 5) for g in (1, 0, 2))  # `ind` is seat 1
    # a flushed arena records nothing until its next first iteration; `ind` gives up (arena 0, iteration 6): the game that
    # follows is recorded again
    for t in range(6, 12):
        rec.step(d_cmd[t])
    rec.flush()
    games, _, _ = rec.collect()
    assert p.games[0][0]["iterations"] == 7  # (iterations 0 .. 6: the next game's first is iteration 7)
    assert _summary(games) == [(0, 1, 3 * 5, 5, abi.RECORD_CUT)]


def test_index_full_and_a_lone_player():
    p = rc.solo_played()
    sim = _env(p.w)
    rec = sim.recorder(len(p.cmds) + 2, 1)
    _record(p, sim, rec, digests=False)
    games, data, counts = rec.collect()
    want = [g for g in rc.expected_games(p, flushed=False)]
    firsts = [next(g for g in want if g[0] == a) for a in sorted({g[0] for g in want})]
    assert rc.delivered_games(games, data) == firsts
    # every later first iteration of those arenas found the index full (the game their flush would cut included)
    lost = sum(len(p.games[a]) - 1 for a in {g[0] for g in want})
    assert counts["games_lost"] == lost > 0 and rec.collect()[2]["games_lost"] == 0


def test_every_error_code_leaves_the_environment_alone():
    from strikeforce_amd.env import StrikeForceError
    p, sim, d_cmd = _fight()
    other = _env(rc.batch_workload(4, 0))
    fresh = _env(rc.batch_workload(4, 0))
    rec, rec_other = sim.recorder(64, 2), other.recorder(64, 2)
    rec.step(d_cmd[0])
    before = sim.digest()

    def refused(code, fn, *args):
        with pytest.raises(StrikeForceError, match=r"\(%d\)" % code):
            fn(*args)
        assert (sim.digest() == before).all()

    for bad in ((2, 2), (1 << 31, 2), (64, 0), (0, 1), (-1, 1), (64, -3)):  # (n_agents is 3)
        refused(ERR_ARG, sim.recorder, *bad)
    refused(ERR_ARG, lambda: sim._ck(sim.L.sf_record_step(sim.h, rec_other.h, d_cmd[1].data_ptr()), "sf_record_step"))
    refused(ERR_ARG, lambda: sim._ck(sim.L.sf_record_flush(sim.h, rec_other.h), "sf_record_flush"))
    refused(ERR_ARG, rec.step, None)
    refused(ERR_ARG, lambda: sim._ck(sim.L.sf_record_step(sim.h, None, d_cmd[1].data_ptr()), "sf_record_step"))
    refused(ERR_ARG, rec.collect, 0, 4)
    refused(ERR_ARG, rec.collect, 64, 0)
    # outputs of exactly the sizes given (the device allocator's own blocks: a tensor's block may be longer than the tensor)
    import glob
    import os
    import torch
    lib = sorted(glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so*")))
    H = C.CDLL(lib[0] if lib else "libamdhip64.so")
    H.hipMalloc.argtypes, H.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    bufs = []

    def alloc(nbytes):
        q = C.c_void_p()
        assert H.hipMalloc(C.byref(q), nbytes) == 0
        bufs.append(q)
        return q.value

    small, g, c = alloc(16), alloc(4 * 48), alloc(6 * 8)
    host = np.zeros(64, dtype=np.uint8)
    refused(ERR_ARG, rec.collect_device, small, 17, g, 4, c)      # d_bytes shorter than max_bytes
    refused(ERR_ARG, rec.collect_device, small, 16, g, 5, c)      # d_games shorter than max_games
    refused(ERR_ARG, rec.collect_device, small, 16, g + 2, 3, c)  # d_games not aligned
    refused(ERR_ARG, rec.collect_device, small, 16, g, 4, c + 8)  # d_counts starts too late
    refused(ERR_ARG, rec.collect_device, host.ctypes.data, 16, g, 4, c)  # host memory
    refused(ERR_ARG, rec.collect_device, small, 16, g, 4, None)
    rec.collect_device(small, 16, g, 4, c)  # ... and exactly fitting outputs are taken (the games are all still open)
    sim.synchronize()
    for q in bufs:
        H.hipFree(q)
    rec_fresh = fresh.recorder(64, 2)  # (an environment that was never reset)
    refused(ERR_STATE, rec_fresh.step, d_cmd[1])
    refused(ERR_STATE, rec_fresh.flush)
    sim.step_begin()
    mid = sim.digest()
    for fn, args in ((rec.step, (d_cmd[1],)), (rec.flush, ())):
        with pytest.raises(StrikeForceError, match=r"\(%d\)" % ERR_STATE):
            fn(*args)
    assert (sim.digest() == mid).all()
    sim.step_end(p.cmds[1, :4])
    before = sim.digest()
    sim.replay_load(["+"] * 4)
    refused(ERR_STATE, rec.step, d_cmd[2])
    refused(ERR_STATE, rec.flush)
    sim.replay_load(None)
    rec.step(d_cmd[2])  # ... and the recorder still works: the game is BROKEN (iteration 1 went through the split step)
    assert _summary(rec.collect()[0]) == [(a, 0, 3, 1, abi.RECORD_BROKEN) for a in range(4)]
    rec.close(), rec_other.close(), rec_fresh.close()


# ---- 5. collection on the device ----------------------------------------------------------------------------------------------
def test_collect_device_with_limits_then_the_rest_on_a_callers_stream():
    import torch
    p = rc.solo_played()
    sim = _env(p.w)
    rec = sim.recorder(len(p.cmds) + 2, 8)
    want = rc.expected_games(p)
    closed = rc.expected_games(p, flushed=False)
    d_cmd = _rows(p.cmds)
    _reset(sim, p.tb, p.serial)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    sim.set_stream(stream.cuda_stream)
    k = len(closed) // 2
    cut_bytes = sum(g[4] for g in closed[:k]) + closed[k][4] - 1  # the game behind the first k misses one byte of room
    with torch.cuda.stream(stream):
        b1, g1 = torch.full((cut_bytes,), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((len(want), 12), -7, dtype=torch.int32, device="cuda")
        b2, g2 = torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((len(want), 12), -7, dtype=torch.int32, device="cuda")
        c1, c2 = torch.zeros(6, dtype=torch.int64, device="cuda"), torch.zeros(6, dtype=torch.int64, device="cuda")
        for t in range(len(p.cmds)):  # nothing waits between the steps and the collects
            rec.step(d_cmd[t])
        rec.collect_device(b1, cut_bytes, g1, len(want), c1)
        rec.flush()
        rec.collect_device(b2, 4096, g2, len(want), c2)
    stream.synchronize()
    c1, c2 = c1.cpu().tolist(), c2.cpu().tolist()
    assert c1[:4] == [k, sum(g[4] for g in closed[:k]), len(closed) - k, sum(g[4] for g in closed[k:])]
    assert c2[:4] == [len(want) - k, sum(g[4] for g in want) - c1[1], 0, 0]
    got = rc.delivered_games(g1.cpu().numpy()[:k], b1.cpu().numpy()[:c1[1]]) + rc.delivered_games(g2.cpu().numpy()[:c2[0]], b2.cpu().numpy()[:c2[1]])
    assert sorted(got) == want and got[:k] == closed[:k]
    # nothing behind what was delivered is written
    assert (b1.cpu().numpy()[c1[1]:] == 0xEE).all() and (g1.cpu().numpy()[k:] == -7).all() and (b2.cpu().numpy()[c2[1]:] == 0xEE).all()
    sim.set_stream(0)
    sim.synchronize()
