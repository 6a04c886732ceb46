"""The continuations of tests/state_put_cases.py, from the oracle alone: they are long enough to tell a wrong hidden word
from a right one.  `tiny` ends at least two games per arena under auto_reset (20-step Timer games), so a wrong seed digit
or a wrong arming of the next episode's generator cannot pass the GPU tests; `battle` arena 1, finished when the put happens,
stays finished."""
import numpy as np

import state_put_cases as pc
import state_records_cases as sc


def test_tiny_ends_at_least_two_games_per_arena():
    dig, eps, done, results, hdrs = pc.oracle_continuation("tiny")
    assert len(pc.continuation("tiny")) == 45 and sc.case("tiny").w.cfg.auto_reset == 1
    assert (eps[1] - eps[0] >= 2).all(), (eps[1] - eps[0]).tolist()
    assert len({int(h.tb) for h in hdrs}) == len(hdrs)  # every arena on a seed of its own after the restarts
    assert (dig[1:] != dig[:-1]).all()  # every step moves every arena


def test_battle_arena_one_stays_done():
    dumps, _ = sc.oracle_dumps("battle")
    assert dumps[1].hdr.done == 1 and dumps[0].hdr.done == 0
    dig, eps, done, results, hdrs = pc.oracle_continuation("battle")
    assert hdrs[1].done == 1 and done[1] == 1 and (dig[:, 1] == dig[0, 1]).all()  # it stands still
    assert (dig[1:, 0] != dig[:-1, 0]).all()


def test_the_continuations_have_the_documented_lengths_and_other_seeds():
    for name in sc.NAMES:
        rows = pc.continuation(name)
        c = sc.case(name)
        assert rows.shape == (45 if name == "tiny" else 40, c.w.cfg.arenas, c.w.cfg.n_agents) and rows.dtype == np.uint8
        assert pc.SEED + sc.NAMES.index(name) not in [x[4] for x in sc.CASES]
