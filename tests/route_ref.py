"""Routing agents to several networks restated (include/strikeforce_policy.h, sf_route_*), no GPU: the slot rule, the gather
of one tick's environment-order buffers into each network's rows and the scatter of the networks' rows back.

Every commanded human of the reference owns its network (bots/bot-0.5/Custom.hpp:161-165, bots/bot-1/Agent.hpp:84-101); a
route is that ownership for a batch.  Buffers are handled as bit patterns (uint32 views of 32-bit data, uint8 as it is):
what a copy must not write keeps whatever the caller put there, a sentinel in the tests."""
import numpy as np

HIDDEN, ACTIONS = 160, 9
DENSE = 32 * 31 * 31
MARKER = 0xFFFFFFFF
SENTINEL = 0x7FC0DEAD  # a quiet NaN nobody computes (tests/rollout_ref.py's pattern)
SENTINEL_U8 = 0xAD
ROW_FIELDS = ("cmd", "action", "probs", "value", "reward", "disc")


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype.itemsize == 4 else x


def slots(assign, nets):
    """-> (slot [agents] int, -1 for nobody's; agents_of: per network the list of its agents by slot).  Agent a's slot is
    its rank among the agents of its network in ascending a."""
    seen = [0] * nets
    slot, agents_of = [], [[] for _ in range(nets)]
    for a, k in enumerate(assign):
        k = int(k)
        if k < 0:
            slot.append(-1)
            continue
        assert k < nets
        slot.append(seen[k])
        seen[k] += 1
        agents_of[k].append(a)
    return np.array(slot, dtype=np.int64), agents_of


def empty_dst(n, cap, dense=False):
    """One network's rows, sentinel-filled (bit patterns)."""
    s32 = lambda *shape: np.full((n,) + shape, SENTINEL, dtype=np.uint32)
    d = dict(keys=s32(cap), vals=s32(cap), counts=s32(), pov=s32(HIDDEN), reset=np.full(n, SENTINEL_U8, dtype=np.uint8))
    if dense:
        d["dense"] = s32(DENSE)
    return d


def gather(assign, nets, src, dst):
    """src: keys, vals [agents][cap], counts [agents], pov [agents][160], optional dense [agents][30752], optional reset
    [agents] (any non-zero = restarted).  dst[k]: empty_dst()'s dict, or None (skipped); written in place."""
    slot, _ = slots(assign, nets)
    cap = src["keys"].shape[1]
    counts = bits(src["counts"])
    for a, k in enumerate(assign):
        if k < 0 or dst[k] is None:
            continue
        d, s = dst[k], slot[a]
        cnt = int(counts[a])
        n = min(cnt, cap)
        d["keys"][s, :n] = bits(src["keys"])[a, :n]
        d["vals"][s, :n] = bits(src["vals"])[a, :n]
        d["counts"][s] = cnt
        d["pov"][s] = bits(src["pov"])[a]
        d["reset"][s] = 1 if (src.get("reset") is not None and src["reset"][a]) else 0
        if cnt > cap and src.get("dense") is not None and "dense" in d:
            d["dense"][s] = bits(src["dense"]).reshape(len(assign), DENSE)[a]


def scatter(assign, nets, rows, env):
    """rows[k]: {field: [n_k]... array or None}; env: {field: [agents]... array or None}, written in place for assigned
    agents, field by field where both sides have it."""
    slot, _ = slots(assign, nets)
    for f in ROW_FIELDS:
        if env.get(f) is None:
            continue
        for a, k in enumerate(assign):
            if k < 0 or rows[k].get(f) is None:
                continue
            env[f][a] = bits(rows[k][f])[slot[a]]
