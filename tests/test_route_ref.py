"""tests/route_ref.py against hand-written assignments, and gather followed by scatter as the identity (no GPU).
strikeforce_amd.policy.route_slots, the host form of the same rule, is held to it too."""
import numpy as np
import pytest

import route_ref as ref
from strikeforce_amd import policy

HAND = {
    "all-to-one": ([0, 0, 0, 0], 1, [0, 1, 2, 3], [[0, 1, 2, 3]]),
    "alternating": ([0, 1, 0, 1, 0], 2, [0, 0, 1, 1, 2], [[0, 2, 4], [1, 3]]),
    "a-network-with-no-agents": ([2, 0, 2, 0], 3, [0, 0, 1, 1], [[1, 3], [], [0, 2]]),
    "nobody's": ([-1, 1, -1, 0, 1, -1], 2, [-1, 0, -1, 0, 1, -1], [[3], [1, 4]]),
    "all-nobody's": ([-1, -1, -1], 2, [-1, -1, -1], [[], []]),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_slot_rule_on_hand_written_assignments(name):
    assign, nets, slot, agents_of = HAND[name]
    got_slot, got_agents = ref.slots(assign, nets)
    assert got_slot.tolist() == slot and got_agents == agents_of
    lib_slot, lib_agents = policy.route_slots(assign, nets)
    assert lib_slot.tolist() == slot and [x.tolist() for x in lib_agents] == agents_of


def test_slot_rule_130_agents_over_3_networks():
    assign = [a % 3 for a in range(130)]
    slot, agents_of = ref.slots(assign, 3)
    assert slot.tolist() == [a // 3 for a in range(130)]
    assert [len(x) for x in agents_of] == [44, 43, 43]
    assert agents_of[1] == list(range(1, 130, 3))
    # an uneven one: network 0 the first 7, then network 2 on every fifth agent, the rest network 1
    assign = [0 if a < 7 else 2 if a % 5 == 0 else 1 for a in range(130)]
    slot, agents_of = ref.slots(assign, 3)
    assert agents_of[0] == list(range(7)) and agents_of[2] == list(range(10, 130, 5))
    assert slot[10] == 0 and slot[15] == 1 and slot[7] == 0 and slot[8] == 1 and slot[9] == 2 and slot[11] == 3
    for k in range(3):
        assert [int(slot[a]) for a in agents_of[k]] == list(range(len(agents_of[k])))
    lib_slot, lib_agents = policy.route_slots(assign, 3)
    assert np.array_equal(lib_slot, slot) and [x.tolist() for x in lib_agents] == agents_of


def _source(agents, cap, rng):
    counts = np.array([(0, 1, 3, 4, 5, cap - 1, cap, cap + 1, ref.MARKER)[a % 9] for a in range(agents)], dtype=np.uint32)
    return dict(keys=rng.integers(0, 2 ** 32, size=(agents, cap), dtype=np.uint32), vals=rng.standard_normal((agents, cap)).astype(np.float32),
                counts=counts, pov=rng.standard_normal((agents, ref.HIDDEN)).astype(np.float32),
                dense=rng.standard_normal((agents, ref.DENSE)).astype(np.float32), reset=(rng.uniform(size=agents) < 0.3).astype(np.uint8))


@pytest.mark.parametrize("agents,nets", [(1, 1), (17, 2), (130, 3)])
def test_gather_writes_what_the_header_says(agents, nets):
    cap, rng = 8, np.random.default_rng(agents)
    assign = [(-1 if a % 7 == 3 else a % nets) for a in range(agents)]
    src = _source(agents, cap, rng)
    slot, agents_of = ref.slots(assign, nets)
    dst = [ref.empty_dst(len(agents_of[k]) + 2, cap, dense=True) for k in range(nets)]
    ref.gather(assign, nets, src, dst)
    for k in range(nets):
        d = dst[k]
        for s, a in enumerate(agents_of[k]):
            cnt = int(src["counts"][a])
            n = min(cnt, cap)
            assert np.array_equal(d["keys"][s, :n], src["keys"][a, :n]) and (d["keys"][s, n:] == ref.SENTINEL).all()
            assert np.array_equal(d["vals"][s, :n], src["vals"][a, :n].view(np.uint32)) and (d["vals"][s, n:] == ref.SENTINEL).all()
            assert d["counts"][s] == cnt and d["reset"][s] == src["reset"][a]
            assert np.array_equal(d["pov"][s], src["pov"][a].view(np.uint32))
            if cnt > cap:
                assert np.array_equal(d["dense"][s], src["dense"][a].view(np.uint32))
            else:
                assert (d["dense"][s] == ref.SENTINEL).all()
        for name in ("keys", "vals", "counts", "pov", "dense"):  # rows behind count(k)
            assert (d[name][len(agents_of[k]):] == ref.SENTINEL).all()
        assert (d["reset"][len(agents_of[k]):] == ref.SENTINEL_U8).all()


@pytest.mark.parametrize("agents,nets", [(5, 2), (65, 2), (130, 3)])
def test_gather_then_scatter_of_copied_rows_is_the_identity_on_assigned_agents(agents, nets):
    """The environment's rows are gathered by the slot rule (what a network would answer if it answered its input), scattered
    into sentinel-filled environment rows: assigned agents get their own row back, the others keep the sentinel."""
    rng = np.random.default_rng(7 * agents)
    assign = [(-1 if a % 5 == 4 else (a * a) % nets) for a in range(agents)]
    _, agents_of = ref.slots(assign, nets)
    truth = dict(cmd=rng.integers(32, 127, size=agents).astype(np.uint8), action=rng.integers(0, 9, size=agents).astype(np.int32),
                 probs=rng.uniform(size=(agents, 9)).astype(np.float32), value=rng.uniform(size=agents).astype(np.float32),
                 reward=rng.standard_normal(agents).astype(np.float32), disc=rng.uniform(size=agents).astype(np.float32))
    rows = [{f: truth[f][agents_of[k]] for f in ref.ROW_FIELDS} for k in range(nets)]
    env = {f: np.full(truth[f].shape, ref.SENTINEL_U8 if f == "cmd" else ref.SENTINEL, dtype=np.uint8 if f == "cmd" else np.uint32)
           for f in ref.ROW_FIELDS}
    ref.scatter(assign, nets, rows, env)
    mine = np.array(assign) >= 0
    for f in ref.ROW_FIELDS:
        assert np.array_equal(env[f][mine], ref.bits(truth[f])[mine]), f
        assert (env[f][~mine] == (ref.SENTINEL_U8 if f == "cmd" else ref.SENTINEL)).all(), f
    # a field missing on either side is skipped
    env2 = {f: np.full_like(env[f], 1) for f in ref.ROW_FIELDS}
    env2["value"] = None
    rows2 = [dict(r, reward=None) for r in rows]
    ref.scatter(assign, nets, rows2, env2)
    assert (env2["reward"] == 1).all() and np.array_equal(env2["disc"][mine], ref.bits(truth["disc"])[mine])
