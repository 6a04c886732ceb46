"""The host side of the episode log on synthetic buffers: env.decode_episodes, shard.fresh_episodes, the host
restatement of the collection kernel, and two gloo ranks that tell fresh records from stale ones across two gathers."""
import os
import socket
import subprocess
import sys

import numpy as np

from episode_log_ref import collect_like_kernel
from strikeforce_amd import env, shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rings(world, A, depth, agents, episodes, tb0=1_700_000_000, stride=1000):
    """Rings as the kernels leave them after `episodes[w][a]` ends: episode e in slot e & (depth - 1), -1 where empty."""
    rw = env.episode_record_words(agents)
    g = np.full((world, A, depth, rw), -1, dtype=np.int32)
    for w in range(world):
        for a in range(A):
            for e in range(episodes[w][a]):
                tb = tb0 + (w * A + a) + e * stride + (1 << 33)
                rec = [a, e, tb & 0xffffffff, tb >> 32, 7, 1, 10 + e, 2] + [100 * w + 10 * a + e] * (8 * agents)
                g[w, a, e & (depth - 1)] = np.array(rec, dtype=np.uint64).astype(np.uint32).view(np.int32)
    return g


def test_decode_episodes_names_every_word():
    g = rings(1, 3, 4, 2, [[2, 0, 5]])[0]
    d = env.decode_episodes(g, 2)
    assert d["results"].shape == (12, 2, 8) and d["tb"].dtype == np.uint64
    keep = d["episode"] >= 0
    assert sorted(zip(d["arena"][keep], d["episode"][keep])) == [(0, 0), (0, 1), (2, 1), (2, 2), (2, 3), (2, 4)]
    i = int(np.nonzero((d["arena"] == 2) & (d["episode"] == 3))[0][0])
    assert d["tb"][i] == 1_700_000_000 + 2 + 3 * 1000 + (1 << 33) and d["serial"][i] == 7 + (1 << 32)
    assert d["steps"][i] == 13 and d["outcome"][i] == 2 and (d["results"][i] == 23).all()


def test_fresh_episodes_across_two_gathers():
    first = rings(2, 3, 4, 1, [[1, 0, 3], [2, 6, 0]])
    recs, cur = shard.fresh_episodes(first, np.zeros((2, 3), dtype=np.int64))
    d = env.decode_episodes(recs, 1)
    # arena 1 of rank 1 ended 6 episodes in a ring of 4: episodes 0 and 1 are gone, 2..5 are fresh
    assert list(zip(d["arena"], d["episode"])) == [(0, 0), (2, 0), (2, 1), (2, 2), (0, 0), (0, 1), (1, 2), (1, 3), (1, 4), (1, 5)]
    assert (cur == [[1, 0, 3], [2, 6, 0]]).all()
    second = rings(2, 3, 4, 1, [[1, 2, 3], [4, 6, 1]])
    recs, cur2 = shard.fresh_episodes(second, cur)
    d = env.decode_episodes(recs, 1)
    assert list(zip(d["arena"], d["episode"])) == [(1, 0), (1, 1), (0, 2), (0, 3), (2, 0)]
    assert (cur2 == [[1, 2, 3], [4, 6, 1]]).all()
    recs, cur3 = shard.fresh_episodes(second, cur2)
    assert len(recs) == 0 and (cur3 == cur2).all()


def test_collection_restated_on_the_host_orders_caps_and_counts():
    g = rings(1, 4, 4, 1, [[3, 0, 6, 2]])[0]
    episodes = [3, 0, 6, 2]
    recs, counts, cur = collect_like_kernel(g, episodes, [0, 0, 0, 0], 5)
    d = env.decode_episodes(recs, 1)
    assert list(zip(d["arena"], d["episode"])) == [(0, 0), (0, 1), (0, 2), (2, 2), (2, 3)]
    assert counts == (5, 2, 4) and list(cur) == [3, 0, 4, 0]
    recs, counts, cur = collect_like_kernel(g, episodes, cur, 100)
    d = env.decode_episodes(recs, 1)
    assert list(zip(d["arena"], d["episode"])) == [(2, 4), (2, 5), (3, 0), (3, 1)]
    assert counts == (4, 0, 0) and list(cur) == episodes


WORKER = r"""
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np, torch, torch.distributed as dist
from strikeforce_amd import shard
from test_episode_log_host import rings
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
cur = np.zeros((world, 3), dtype=np.int64)
seen = []
for counts in ([[1, 0, 2], [0, 3, 1]], [[2, 1, 2], [5, 3, 1]]):
    local = torch.from_numpy(rings(world, 3, 4, 1, counts)[rank])
    g = shard.gather_episode_rings(local, world)
    recs, cur = shard.fresh_episodes(g, cur)
    seen.append(recs)
if rank == 1:
    np.save({out!r}, np.concatenate(seen))
    np.save({out!r} + ".cur.npy", cur)
dist.barrier()
dist.destroy_process_group()
"""


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_gloo_ranks_take_each_record_once(tmp_path):
    out = str(tmp_path / "seen.npy")
    script = tmp_path / "worker.py"
    script.write_text(WORKER.format(root=ROOT, out=out))
    e = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE="2", OMP_NUM_THREADS="1")
    procs = [subprocess.Popen([sys.executable, str(script)], env=dict(e, RANK=str(r), LOCAL_RANK=str(r))) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    d = env.decode_episodes(np.load(out), 1)
    # first gather: everything; second: only what ended since (rank 1 arena 0 went from 0 to 5 ends: 1..4 kept, 0 lost)
    got = list(zip(d["tb"] - (1 << 33) - 1_700_000_000 - d["episode"] * 1000, d["episode"]))
    want = [(0, 0), (2, 0), (2, 1), (4, 0), (4, 1), (4, 2), (5, 0),
            (0, 1), (1, 0), (3, 1), (3, 2), (3, 3), (3, 4)]
    assert [(int(a), int(b)) for a, b in got] == want
    assert (np.load(out + ".cur.npy") == [[2, 1, 2], [5, 3, 1]]).all()
