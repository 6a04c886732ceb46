"""The cases of tests/state_records_cases.py, from the oracle alone: together they hold every state the device decoder must
get right, their shapes are the ones the traversal can go wrong at, and the digest restated in tests/state_records_ref.py
equals the oracle's — so the expected arrays and the restated digest that the device tests compare with stand on the oracle.
These are conditions on the cases, not measurements."""
import numpy as np
import pytest

import state_records_cases as sc
import state_records_ref as ref


def test_the_cases_hold_every_listed_state():
    held = {}
    for name in sc.NAMES:
        dumps, _ = sc.oracle_dumps(name)
        for k, v in sc.features(dumps, sc.case(name).w.cfg).items():
            held[k] = held.get(k, False) or bool(v)
    assert all(held.values()), [k for k, v in held.items() if not v]
    # with the large pools, the zombie extent is above 64 in EVERY arena of the case made for it
    dumps, _ = sc.oracle_dumps("swarm")
    assert all(ref.arena_arrays(d)["counts"][5] > 64 for d in dumps)
    # an exit pool with a gap: an inactive exit below the extent
    assert any(ref.arena_arrays(d)["counts"][7] > ref.arena_arrays(d)["counts"][3] for d in sc.oracle_dumps("large")[0])


def test_the_cases_have_the_shapes_the_traversal_can_go_wrong_at():
    cfgs = [sc.case(n).w.cfg for n in sc.NAMES]
    assert {c.arenas for c in cfgs} == {1, 3, 65}
    assert {c.cap_humans for c in cfgs} == {8, 10, 22} and {c.cap_zombies for c in cfgs} == {24, 64, 200}
    assert {c.cap_bullets for c in cfgs} == {64, 128} and {c.cap_portals for c in cfgs} == {16, 109}
    assert {(c.floors, c.rows, c.cols) for c in cfgs} == {(1, 9, 7), (1, 64, 64), (3, 20, 30), (1, 128, 128)}


@pytest.mark.parametrize("name", sc.NAMES)
def test_restated_digest_and_counts_stand_on_the_oracle(name):
    dumps, digests = sc.oracle_dumps(name)
    for a, d in enumerate(dumps):
        arr = ref.arena_arrays(d)
        assert ref.digest_of(arr) == int(digests[a]), (name, a)
        c = arr["counts"]
        assert c[1] == sum(z.alive for z in d.zombies) and c[2] == sum(b.alive for b in d.bullets)
        assert all(0 <= c[j] <= c[4 + j] for j in range(4)), c
        if c[5]:
            assert d.zombies[c[5] - 1].alive and not any(z.alive for z in d.zombies[c[5]:])


def test_expected_rows_cuts_and_ids():
    dumps, digests = sc.oracle_dumps("tiny")
    arrs = [ref.arena_arrays(d) for d in dumps]
    e = ref.expected(arrs, [2, 0, 0, -1, 3], (1, 0, 5, 16), digests)
    assert e["humans"].shape == (5, 1, 28) and e["zombies"].shape == (5, 0, 7) and e["bullets"].shape == (5, 5, 11)
    assert np.array_equal(e["hdr"][1], e["hdr"][2]) and np.array_equal(e["hdr"][0], arrs[2]["hdr"])
    assert not e["hdr"][3].any() and not e["cell_portal"][4].any() and (e["counts"][3:] == -1).all() and not e["digest"][3:].any()
    assert np.array_equal(e["counts"][0], arrs[2]["counts"])  # (over the whole pools, whatever the cuts)
