"""What the worlds of tests/obs_cases.py reach, asserted from the oracle alone (no GPU): every world gets to the limit of the
observation kernels that its name claims, with windows on both sides of it, before tests/test_gpu_obs_edges.py compares
anything the device wrote.  The window statistics themselves are held against the oracle's dump on the way (who stands
where: obs_cases.window_stats(check=True))."""
import pytest

import obs_cases as oc
import obs_flavour
import obs_matrix
import variant_cases as vc

P, S = obs_flavour.PRODUCT, obs_flavour.SMALL
_cache = {}


def report(name, lim):
    key = (name, id(lim))
    if key not in _cache:
        _cache[key] = obs_matrix.oracle_report(oc.WORLDS[name], lim)
        print({k: v for k, v in _cache[key].items() if v})
    return _cache[key]


def test_the_limits_are_the_kernels():
    """obs_flavour.PRODUCT restates sf_obs_kernels.hpp's defaults, and the small flavour satisfies its static asserts."""
    import os
    import re
    src = open(os.path.join(obs_flavour.CSRC, "sf_obs_kernels.hpp")).read()
    got = {m.group(1): m.group(2) for m in re.finditer(r"#define (SF_O\w+) (.+)", src)}
    assert got == {"SF_OBS_REC_MAX": "72", "SF_OBS_LIST_MAX": "256", "SF_OBS_STAGED": "(2 * OBS_W2)", "SF_OL_REC": "48",
                   "SF_OL_POWQ": "384", "SF_OL_CELLS": "640"}
    assert (P["rec"] + 8, P["list"], P["staged"], P["ol_rec"], P["ol_powq"], P["ol_cells"]) == (72, 256, 2 * oc.W2, 48, 384, 640)
    assert S["ol_rec"] * 33 >= oc.W2 + 3 and S["ol_cells"] % 64 == 0 and S["staged"] <= 2 * oc.W2 and S["rec"] + 8 <= 255
    assert all(S[k] < P[k] for k in P)


def test_walls_reaches_the_cell_limit_on_both_sides():
    """OL_CELLS = 640: windows at exactly 640 (the last one listed) and 641 (the first one marked), the tenth compaction
    pass (577..640), lists longer than the largest cap (2048) and every list longer than the small cap (64), and more
    non-zeros than mode 3 of the dense kernel stages (1922) in windows it does not spill."""
    r = report("walls", P)
    assert r["cells_at_limit"] > 0 and r["cells_one_over"] > 0
    assert r["last_pass"] > 100 and r["marked_by_cells"] > 100 and r["marked_by_records"] == 0
    assert r["marked"] == r["marked_by_cells"] and r["windows"] - r["marked"] > 1000
    assert r["nz_min"] > 64 and r["over_cap_64"] == r["windows"] - r["marked"]
    assert r["nz_max"] > 2048  # (such a window has more than 640 cells: its list is marked, so over_cap_2048 stays 0)
    assert r["over_staged"] > 100 and r["dense_spill"] == 0
    assert r["no_observer"] > 0  # agents died


def test_spill_reaches_the_record_limits_and_the_delta_edges():
    """variant_cases' crowded 64 x 64 world: windows beyond 64 own records (the dense kernel's spill), between 49 and 64
    (marked by the list kernel only); and, in the calls obs_cases.delta_plan runs as differences: spilled windows, windows
    that come back from a spill, observers that died.  Games end and restart."""
    r = report("spill", P)
    assert r["dense_spill"] > 50 and r["marked_by_records"] > r["dense_spill"] and r["marked_by_cells"] == 0
    assert r["windows"] - r["marked"] > 1000
    assert r["spilled_in_incremental"] > 20 and r["back_from_spill"] > 0 and r["observer_died"] > 0
    assert r["episodes"] > 0 and r["no_observer"] > 0


def test_crowded_is_the_hbm_plane_with_marked_windows():
    r = report("crowded", P)
    assert vc.expected_variant(oc.WORLDS["crowded"].workload().cfg)[1:3] == (1, 1)
    assert r["marked_by_records"] > 0 and r["windows"] - r["marked"] > 100 and r["episodes"] > 0


@pytest.mark.parametrize("name,Z,zombies", [("herd", 1024, 128), ("pools100", 100, 64), ("pools256", 256, 64), ("pools257", 257, 64)])
def test_pool_worlds_fill_their_zombie_tables(name, Z, zombies):
    """Zombie tables of more than 64 slots: staged in several passes of 256 words (100 slots = 300 words), the last staged
    size (256), the first one read where it lies (257), and 1024; live zombies beyond the first 64-slot word (beyond the
    second for 1024), which is what the list kernel's zlim = 64 * SC_ZWN has to cover.  Games end and restart."""
    w = oc.WORLDS[name]
    cfg = w.workload().cfg
    r = report(name, P)
    assert cfg.cap_zombies == Z and vc.expected_variant(cfg)[3] == 1
    assert r["zombies_max"] > zombies and r["episodes"] > 0 and r["windows"] > 60 and r["marked"] == 0


@pytest.mark.parametrize("name,variant", [("C4", (1, 1, 1, 0)), ("NATIVE", (4, 0, 1, 0)), ("FLOORS", (1, 0, 1, 0))])
def test_baseline_worlds(name, variant):
    """C4 (128 x 128: the flag plane in HBM, blocks and portals), the reference's own dimensions, three floors."""
    w = oc.WORLDS[name]
    assert vc.expected_variant(w.workload().cfg) == variant
    r = report(name, P)
    assert r["windows"] > 40 and r["marked"] == 0 and r["dense_spill"] == 0


def test_no_world_reaches_the_product_pow_queues():
    """Why the small flavour exists: no window here has more than 256 non-table values within 64 own records, nor more
    than 384 queued values within 48 (a human carries at most 9 such values, a bullet or zombie 2-3)."""
    for name in ("walls", "spill", "crowded"):
        r = report(name, P)
        assert r["dense_queue_over"] == 0 and r["list_queue_over"] == 0


def test_kits_straddles_every_small_limit():
    """The flavour's limits on KITS, windows on both sides of each: own records of the dense kernel (16) and of the list
    kernel (30), non-empty cells (128; and the last compaction pass, 65..128), the two pow queues (16) over the limit
    WITHIN the record limit, mode 3's staging area (256 non-zeros) and the small cap (360)."""
    r = report("KITS", S)
    n, un = r["windows"], r["windows"] - r["marked"]
    assert 100 < r["dense_spill"] < n - 100                 # own > 16 / <= 16
    assert 100 < r["marked_by_records"] < n - 100           # own > 30 / <= 30
    assert 20 < r["marked_by_cells"] < n - 100              # cells > 128 / <= 128
    assert r["last_pass"] > 100 and un - r["last_pass"] > 50   # listed with 65..128 cells / with at most 64
    assert 100 < r["dense_queue_over"] < n - r["dense_spill"] - 100  # q_dense > 16 with own <= 16 / <= 16
    assert 100 < r["list_queue_over"] < un - 50             # q_list > 16 in a listed window / <= 16
    assert 50 < r["over_staged"] < n - 50                   # nz > 256 unspilled / the rest
    assert 100 < r["over_cap_360"] < un - 100               # listed, longer than the cap / within it


def test_c3_straddles_the_small_queues():
    """C3 is sparser: it never exceeds 30 own records or 128 cells, and is on both sides of the dense kernel's 16 records,
    both pow queues, the staging area and the small cap."""
    r = report("C3", S)
    n = r["windows"]
    assert r["marked"] == 0 and 0 < r["dense_spill"] < n
    assert 0 < r["dense_queue_over"] < n and 20 < r["list_queue_over"] < n - 20
    assert 0 < r["over_staged"] < n and 20 < r["over_cap_200"] < n - 20
