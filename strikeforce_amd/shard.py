"""Multi-GPU sharding of the arena batch: contiguous arena ranges per rank, no data-path
collective; the only exchange is the all-gather of the end-of-episode result records (the latched one per arena, or
the episode log's rings: every finished episode)."""
import ctypes as C


def shard_seeds(workload, rank, base_tb=1_700_000_000, serial=123_456_789):
    """Seeds of rank `rank`'s arenas: global arena id g = rank * arenas + i gets tb = base + g."""
    return workload.seeds(base_tb=base_tb, serial=serial, first_arena=rank * workload.cfg.arenas)


def command_seed(workload, rank, seed0=12345):
    """First LCG seed of the random-action agent for this rank's (arena, agent) pairs."""
    return seed0 + rank * workload.cfg.arenas * workload.cfg.n_agents


def gather_results(local, world):
    """All-gather of the [arenas][agents][8] int32 result records (torch tensor on the rank's device).
    Returns a [world * arenas][agents][8] tensor; RCCL over xGMI under backend 'nccl', gloo on CPU."""
    import torch
    import torch.distributed as dist
    if world == 1:
        return local
    flat = local.contiguous().reshape(-1)
    out = torch.empty(world * flat.numel(), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, flat)
    return out.reshape((world * local.shape[0],) + tuple(local.shape[1:]))


def gather_episode_rings(local, world):
    """All-gather of the raw episode-log rings ([arenas][depth][record words] int32, torch tensor on the rank's device:
    what ArenaBatch.episode_ring returns, or a device copy).  Returns a [world][arenas][depth][record words] tensor, the
    layout of sf_episodes_allgather; RCCL over xGMI under backend 'nccl', gloo on CPU."""
    import torch
    import torch.distributed as dist
    if world == 1:
        return local.unsqueeze(0)
    flat = local.contiguous().reshape(-1)
    out = torch.empty(world * flat.numel(), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out, flat)
    return out.reshape((world,) + tuple(local.shape))


def fresh_episodes(gathered, cursors):
    """The records of gathered rings ([world][arenas][depth][record words], numpy or torch) that are newer than a
    consumer's cursors (int64 [world][arenas]: the first episode not seen yet, 0 at the start), in (rank, arena,
    episode) order, and the advanced cursors.  A ring holds each arena's last `depth` episodes and a gather does not
    move anything on the device, so the consumer keeps these cursors itself; an empty slot (episode -1) is never fresh.
    Episodes that ended more than `depth` ago between two gathers are not in the ring any more: new cursor minus old
    cursor minus records returned of an arena counts them.  sf_reset on a rank restarts its episode numbers at 0 (and
    empties its rings): reset that rank's row of cursors to 0 together with it, or its new records stay hidden until
    they pass the old count."""
    import numpy as np
    g = gathered.cpu().numpy() if hasattr(gathered, "cpu") else np.asarray(gathered)
    if g.ndim != 4:
        raise ValueError("gathered rings must be [world][arenas][depth][record words]")
    cur = np.asarray(cursors, dtype=np.int64)
    if cur.shape != g.shape[:2]:
        raise ValueError("cursors must be [world][arenas]")
    ep = g[:, :, :, 1].astype(np.int64)
    fresh = ep >= cur[:, :, None]
    w, a, _ = np.nonzero(fresh)
    e = ep[fresh]
    order = np.lexsort((e, a, w))
    recs = g[fresh][order]
    new = np.maximum(cur, ep.max(axis=2) + 1)
    return recs, new
