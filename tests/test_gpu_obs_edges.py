"""The observation kernels (k_observe modes 0-4, k_observe_redo, k_observe_list; sf_obs_kernels.hpp) at every limit, fallback and
write mode, against the oracle.  The CPU wave emulator only calls sf_obs.hpp's per-cell functions, so the kernels' own
machinery — record tables, pow queues, compaction passes, non-zero bitmaps, delta bookkeeping, spill paths — is checked
here and nowhere else.

tests/obs_matrix.py is the matrix (dense from the host and the device call against the oracle; delta calls against the
plain call before every step; list against dense with the crowded marker asserted if and only if the oracle's window
statistics say so; the overflow redo into a NaN-filled buffer).  tests/obs_cases.py holds the worlds, and
tests/test_obs_cases.py asserts on the CPU what each of them reaches.  Here:
- the product build on every world, in this process;
- the list as mode 3 of the dense kernel (SF_OBS_LIST_BLOCK=1) on the wall-dense world, whose windows of more than 1922
  non-zeros take that mode's unstaged branch: a child process, because the switch is read once per process;
- the small-limits build (tests/obs_flavour.py) on KITS and C3, where ordinary play overflows both pow queues within the
  record limits and straddles every other limit: one child process per world with SF_LIBRARY_PATH set.
Every test prints its report (windows compared, how many took each path by the reference statistics, largest ulp
difference, seconds) and asserts that the paths it is there for were taken.

Measured on an MI355X (live windows compared / marked by the list kernel / other paths by the reference statistics; the
largest ulp difference from the oracle was 0 everywhere; the whole file takes 30 s):
  product  walls     12538 / 1080 (all by cells)   44 at exactly 640 cells, 145 at 641, 3274 in the tenth pass, every list
                                                   over cap 64, 13618 rows redone; under SF_OBS_LIST_BLOCK 2007 unstaged
  product  spill      7513 / 1449 (all by records) 464 spilled by the dense kernel; in incremental delta calls 347 spilled,
                                                   25 back from a spill, 15 observers died; 9 episodes ended
  product  crowded     874 / 6                     1 spilled; HBM plane with bitmaps
  product  herd         66 / 0                     Z = 1024, up to 169 live zombies
  product  pools100 / 256 / 257   150 / 0 each     up to 90 live zombies; 1228 delta calls each
  product  C4 72 / 0, NATIVE 48 / 0, FLOORS 206 / 0
  small    KITS       1354 / 339 (336 by records, 47 by cells)  823 spilled, 275 over the dense pow queue within 16 records,
                                                   891 over the list's pow queue unmarked, 375 over mode 3's staging area,
                                                   902 in the last pass, 353 over cap 360, 1031 rows redone
  small    C3          240 / 0                     8 spilled, 8 / 78 over the dense / list pow queue, 103 over cap 200
The list kernel's in-place x^(1/5) past its queue, which skips the host-built table, gave the dense kernel's bits in every one
of those windows: ocml's pow and the host's agree on the table's inputs on this hardware, so the kernel is left as it is."""
import json
import os
import subprocess
import sys

import pytest

import obs_cases as oc
import obs_flavour
import obs_matrix

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))


def _show(what, rep):
    print("OBS-EDGES %s %s" % (what, json.dumps({k: v for k, v in rep.items() if v or k == "max_ulp"})))


def _reached(name, r):
    """The paths the world is there for, from the run's reference statistics (the same claims as tests/test_obs_cases.py)."""
    listed = r["windows"] - r["marked"]
    if name == "walls":
        assert r["cells_at_limit"] > 0 and r["cells_one_over"] > 0 and r["last_pass"] > 100 and r["marked_by_cells"] > 100
        assert r["over_cap_64"] == listed > 1000 and r["redone_rows"] >= 2 * r["marked"] + listed
    elif name == "spill":
        assert r["dense_spill"] > 50 and r["marked"] > r["dense_spill"] and listed > 1000
        assert r["spilled_in_incremental"] > 20 and r["back_from_spill"] > 0 and r["observer_died"] > 0 and r["episodes"] > 0
    elif name == "crowded":
        assert r["marked"] > 0 and listed > 100 and r["episodes"] > 0
    elif name in ("herd", "pools100", "pools256", "pools257"):
        assert listed == r["windows"] > 60 and r["episodes"] > 0
    elif name in ("C4", "NATIVE", "FLOORS"):
        assert listed == r["windows"] > 40
    elif name == "KITS":
        assert r["dense_spill"] > 100 and r["dense_queue_over"] > 100 and r["list_queue_over"] > 100 and r["over_staged"] > 50
        assert r["marked_by_records"] > 100 and r["marked_by_cells"] > 20 and r["last_pass"] > 100 and r["over_cap_360"] > 100
        assert r["spilled_in_incremental"] > 100 and listed > 500
    elif name == "C3":
        assert r["dense_spill"] > 0 and r["dense_queue_over"] > 0 and r["list_queue_over"] > 20 and r["over_cap_200"] > 20
        assert listed == r["windows"] > 200
    assert r["incremental_calls"] > 0 and r["delta_calls"] > 20 and r["max_ulp"] <= 1


@pytest.mark.parametrize("name", oc.PRODUCT_WORLDS)
def test_the_product_build_at_its_limits(name):
    rep = obs_matrix.run(oc.WORLDS[name], obs_flavour.PRODUCT)
    _show("product %s" % name, rep)
    _reached(name, rep)


def _child(args, extra_env, seconds):
    """One world of the matrix in a fresh process (the library reads its path and switches once); its report."""
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.join(TESTS, "obs_matrix.py")] + args
    p = subprocess.run(cmd, env=dict(os.environ, **extra_env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, "%s exited with %d:\n%s" % (" ".join(args), p.returncode, p.stdout[-4000:])
    reports = [ln for ln in p.stdout.splitlines() if ln.startswith("REPORT ")]
    assert len(reports) == 1, p.stdout[-2000:]
    return json.loads(reports[0][len("REPORT "):])


def test_the_list_as_mode_3_of_the_dense_kernel_unstaged():
    """SF_OBS_LIST_BLOCK=1 on the wall-dense world: windows of more than 1922 non-zeros (641 or more wall cells) leave
    through mode 3's unstaged branch, the others through the staging area; every list equals the dense row (no window here
    has more than 64 own records, so none is marked)."""
    rep = _child(["walls", "product", "--list-block"], {"SF_OBS_LIST_BLOCK": "1"}, 900)
    _show("product walls SF_OBS_LIST_BLOCK", rep)
    assert rep["over_staged"] > 100 and rep["windows"] - rep["over_staged"] > 1000 and rep["dense_spill"] == 0
    assert rep["max_ulp"] <= 1 and rep["cells_one_over"] > 0


@pytest.mark.parametrize("name", oc.FLAVOUR_WORLDS)
def test_the_small_limits_build(name):
    """Every fallback that play cannot reach at the product's limits, on ordinary worlds: the marker's "if and only if" and
    every path count use the flavour's limits."""
    rep = _child([name, "small"], {"SF_LIBRARY_PATH": obs_flavour.lib()}, 900)
    _show("small %s" % name, rep)
    _reached(name, rep)
