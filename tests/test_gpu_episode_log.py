"""The episode log on the MI355X (strikeforce.h sf_episode_log): every case against the oracle stepped one step at a time
on the same commands (tests/episode_log_ref.py: a record is sfo_results behind its header, with the seed formula
tb = seeds()[a] + episode x stride)."""
import numpy as np
import pytest

from episode_log_cases import lay_quits
from episode_log_ref import OracleEpisodes, collect_like_kernel
from oracle_lib import Oracle
from strikeforce_amd import config, env

pytestmark = pytest.mark.gpu


def workload(which, arenas, stride=0):
    w = config.baseline_workload(which, arenas=arenas)
    if which == "C3":
        w.cfg.timer_frames_per_level = 30  # every Timer episode ends at frame 31 unless the player dies first
    if which == "NATIVEGAME":
        w.cfg.timer_frames_per_level = 20  # level 3: 60 frames, a few dozen steps per game on the LDS zombie table
    w.cfg.reseed_stride = stride
    return w


def device_cmds(cmds):
    import torch
    return torch.from_numpy(np.ascontiguousarray(cmds)).cuda()


def run_launches(which, arenas, steps, k, depth, stride=0, collect=True, quits=None):
    """Steps the GPU in k-step launches and the oracle one step at a time; after every launch the rings must equal the
    oracle's.  Returns (oracle log, GPU env, per-launch collections, ended counts before each launch)."""
    w = workload(which, arenas, stride)
    g = env.ArenaBatch(w)
    g.enable_episode_log(depth)
    tb, sr = w.seeds()
    g.reset(tb, sr)
    o = OracleEpisodes(Oracle(w), tb, sr)
    cmds, _ = config.bench_commands(arenas, w.cfg.n_agents, steps)
    if quits:  # arena a's `ind` gives up every quits[a % len(quits)]-th step (0: never): episode_log_cases.lay_quits
        lay_quits(cmds, [quits[a % len(quits)] for a in range(arenas)], ind=w.cfg.ind)
    d = device_cmds(cmds)
    got, before = [], []
    for s0 in range(0, steps, k):
        before.append(o.ended())
        g.step_device(d[s0].data_ptr(), k)
        for s in range(s0, s0 + k):
            o.step(cmds[s])
        ring = g.episode_ring()
        want = o.ring(depth)
        assert (ring == want).all(), (which, s0, np.argwhere(ring != want)[:5])
        if collect:
            got.append(g.episodes())
    return o, g, got, before


@pytest.mark.parametrize("which,stride", [("C3", 0), ("C2", 1 << 20)])
def test_nothing_lost(which, stride):
    A, depth = 512, 8
    o, g, got, before = run_launches(which, A, 1200, 100, depth, stride)
    assert all(c[1] == 0 and c[2] == 0 for _, c in got)  # lost == 0, nothing left pending
    recs = np.concatenate([r for r, _ in got])
    d = env.decode_episodes(recs, 1)
    per = {a: recs[d["arena"] == a] for a in range(A)}
    for a in range(A):
        want = o.records[a]
        assert len(per[a]) == len(want)
        assert (d["episode"][d["arena"] == a] == np.arange(len(want))).all()  # 0, 1, 2, ... no gaps
        if want:
            assert (per[a] == np.array(want)).all(), a
    # precondition of the case the log exists for: some arena ended >= 2 episodes inside one launch
    ends = np.diff(np.array(before + [o.ended()]), axis=0)
    assert ends.max() >= 2
    assert sum(len(r) for r in o.records) == len(recs) > 0
    # sf_results is each arena's newest record
    res = g.results()
    for a in range(A):
        if o.records[a]:
            assert (o.records[a][-1][env.EPISODE_HDR_WORDS:] == res[a].reshape(-1)).all()
    g.close()


def test_overflow_keeps_the_newest():
    A = 256
    o, g, got, _ = run_launches("C3", A, 600, 600, 2)
    recs, (written, lost, pending) = got[0]
    ended = o.ended()
    assert (ended > 2).all()
    assert lost == int((ended - 2).sum()) and pending == 0 and written == 2 * A
    want = np.concatenate([np.array(o.records[a][-2:]) for a in range(A)])
    assert (recs == want).all()
    g.close()


def test_partial_collection_equals_one_large_call():
    A = 256
    w = workload("C3", A)
    a, b = env.ArenaBatch(w), env.ArenaBatch(w)
    for x in (a, b):
        x.enable_episode_log(8)
        x.reset(*w.seeds())
    cmds, _ = config.bench_commands(A, 1, 100)
    d = device_cmds(cmds)
    a.step_device(d.data_ptr(), 100), b.step_device(d.data_ptr(), 100)
    big, (n, lost, pend) = b.episodes()
    assert lost == 0 and pend == 0 and n > 3 * A
    parts, last = [], None
    while True:
        r, (w_, l_, p_) = a.episodes(max_records=37)
        assert l_ == 0 and (last is None or p_ == last - w_)
        parts.append(r)
        last = p_
        if p_ == 0:
            break
    assert (np.concatenate(parts) == big).all()
    r, c = a.episodes()
    assert len(r) == 0 and c == (0, 0, 0)
    a.close(), b.close()


def test_log_on_perturbs_nothing():
    A = 512
    w = workload("C2", A)
    on, off = env.ArenaBatch(w), env.ArenaBatch(w)
    on.enable_episode_log(4)
    tb, sr = w.seeds()
    on.reset(tb, sr), off.reset(tb, sr)
    cmds, _ = config.bench_commands(A, 1, 600)
    d = device_cmds(cmds)
    for s0 in range(0, 600, 100):
        on.step_device(d[s0].data_ptr(), 100), off.step_device(d[s0].data_ptr(), 100)
        on.episodes()
        assert (on.digest() == off.digest()).all()
        assert (on.results() == off.results()).all() and (on.done() == off.done()).all()
        assert (on.agent_alive() == off.agent_alive()).all()
    # after sf_reset the log starts again at episode 0 with no stale records
    on.reset(tb, sr)
    assert (on.episode_ring() == -1).all()
    assert on.episodes()[1] == (0, 0, 0)
    o = OracleEpisodes(Oracle(w), tb, sr)
    on.step_device(d.data_ptr(), 300)
    for s in range(300):
        o.step(cmds[s])
    r, c = on.episodes()
    assert c[1] == 0 and (r == o.since([0] * A)).all()
    on.close(), off.close()


def test_log_states_and_arguments():
    w = workload("C3", 8)
    g = env.ArenaBatch(w)
    g.reset(*w.seeds())
    with pytest.raises(env.StrikeForceError):
        g.episodes()  # SF_ERR_STATE: the log is off
    for bad in (3, 128, -1):
        with pytest.raises(env.StrikeForceError):
            g.enable_episode_log(bad)
    g.enable_episode_log(4)
    with pytest.raises(env.StrikeForceError):
        g.episodes(max_records=-1)
    g.step_begin()
    with pytest.raises(env.StrikeForceError):
        g.episodes()  # between sf_step_begin and sf_step_end
    g.step_end(np.full(8, ord("+"), dtype=np.uint8))
    g.episodes()
    g.enable_episode_log(0)
    with pytest.raises(env.StrikeForceError):
        g.episode_ring()
    g.close()


@pytest.mark.parametrize("path", ["host_step", "split_step"])
def test_one_step_paths(path):
    A, depth = 64, 8
    w = workload("C3", A)
    g = env.ArenaBatch(w)
    g.enable_episode_log(depth)
    tb, sr = w.seeds()
    g.reset(tb, sr)
    o = OracleEpisodes(Oracle(w), tb, sr)
    cmds, _ = config.bench_commands(A, 1, 100)
    for s in range(100):
        if path == "host_step":
            g.step(cmds[s]), o.step(cmds[s])
        else:
            g.step_begin(), g.step_end(cmds[s]), o.step_split(cmds[s])
        if s % 25 == 24:
            assert (g.episode_ring() == o.ring(depth)).all(), s
    assert o.ended().min() >= 5
    r, c = g.episodes()
    assert c == (len(r), 0, 0) and (r == o.since([0] * A)).all()
    g.close()


@pytest.mark.parametrize("which,arenas,steps", [("C5", 64, 300), ("NATIVEGAME", 8, 300), ("C4", 64, 400)])
def test_kernel_families(which, arenas, steps):
    # random play alone ends 3 (C5) and 6 (C4) games in these runs: the quit schedule makes every configuration deliver
    # records in every launch, at most 8 per arena and launch (nothing lost at depth 8), a quarter of the arenas as before
    o, g, got, _ = run_launches(which, arenas, steps, 100, 8, quits=[15, 25, 50, 0])
    recs = np.concatenate([r for r, _ in got])
    assert all(c[1] == 0 for _, c in got)
    assert all(c[0] >= arenas // 2 for _, c in got)  # every launch delivers records
    recs = recs[np.lexsort((recs[:, 1], recs[:, 0]))]  # (collections come launch by launch: arena-major within each)
    assert (recs == o.since([0] * arenas)).all()
    assert len(recs) >= arenas * (steps // 100) and (o.ended()[np.arange(arenas) % 4 != 3] >= 2 * (steps // 100)).all()
    if which == "NATIVEGAME":
        assert o.ended().min() >= 2
    g.close()


def test_collection_reproduced_on_the_host_and_in_a_graph():
    import torch
    A, depth, k = 128, 4, 20
    w = workload("C3", A)
    a, b = env.ArenaBatch(w), env.ArenaBatch(w)
    s = torch.cuda.Stream()
    a.set_stream(s.cuda_stream)
    for x in (a, b):
        x.enable_episode_log(depth)
        x.reset(*w.seeds())
    rw = a.episode_record_words
    cmds, _ = config.bench_commands(A, 1, k)
    d = device_cmds(cmds)
    out = torch.zeros((A * depth, rw), dtype=torch.int32, device="cuda")
    counts = torch.zeros(3, dtype=torch.int32, device="cuda")
    # the loop a training run captures: k steps, then the new records, no host synchronisation in between
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        a.step_device(d.data_ptr(), k)
        a.episodes_device(out.data_ptr(), 100, counts.data_ptr())
    torch.cuda.synchronize()
    a.reset(*w.seeds())  # (capture launched nothing: start both from the same state)
    cur = np.zeros(A, dtype=np.int64)
    total = 0
    for _ in range(8):
        ring_before_cursors = cur.copy()
        with torch.cuda.stream(s):
            graph.replay()
        s.synchronize()
        b.step_device(d.data_ptr(), k)
        ring = b.episode_ring()
        episodes = np.array([b.dump_raw(i)[0].episodes for i in range(A)])
        want, wc, cur = collect_like_kernel(ring, episodes, ring_before_cursors, 100)
        c = tuple(int(x) for x in counts.cpu())
        assert c == wc
        assert (out[:c[0]].cpu().numpy() == want).all()
        total += c[0]
    assert total > 100
    a.close(), b.close()


def test_episodes_allgather_one_rank():
    import torch
    A, depth = 64, 4
    w = workload("C3", A)
    g = env.ArenaBatch(w)
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    g.enable_episode_log(depth)
    g.reset(*w.seeds())
    g.comm_init(env.ArenaBatch.comm_unique_id(), 0, 1)
    cmds, _ = config.bench_commands(A, 1, 300)
    d = device_cmds(cmds)
    out = [torch.full((A * depth * g.episode_record_words,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    for i, s0 in enumerate(range(0, 300, 50)):
        g.step_device(d[s0].data_ptr(), 50)
        g.episodes_allgather(out[i & 1].data_ptr())
        want = g.episode_ring().reshape(-1)
        g.comm_wait(host_too=True)
        assert (out[i & 1].cpu().numpy() == want).all()
    assert (want.reshape(A, depth, -1)[:, :, 1] >= 0).all()
    g.close()
