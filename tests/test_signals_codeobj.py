"""k_signals in the built gfx950 code object, through tests/test_rollout_codeobj.py's reader (llvm-readelf --notes on every
bundle of the library): one instance, no scratch, no LDS, no spilled register.  VGPR / SGPR counts are printed (pytest -s),
not asserted."""
import os
import subprocess

import pytest

import test_rollout_codeobj as rollout
import test_snapshot_codeobj as snap
from strikeforce_amd import build


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    so = build.build(verbose=False)
    tmp = str(tmp_path_factory.mktemp("signals_codeobj"))
    raw, bundles = rollout.bundle_notes(so, tmp)  # (leaves every bundle's code object behind: b<n>/gfx950.co)
    assert bundles == len(build.SOURCES)
    out = {}
    for n in range(bundles):
        for mangled, v in snap.all_notes(os.path.join(tmp, "b%d" % n, "gfx950.co")).items():
            if "k_signals" in mangled:
                out[subprocess.check_output(["c++filt", mangled], text=True).strip()] = v
    return out


def test_k_signals_is_there_once_without_scratch_or_lds(notes):
    assert len(notes) == 1, sorted(notes)
    (name, n), = notes.items()
    print(name, {k: n[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                                   "sgpr_spill_count", "vgpr_spill_count")})
    assert n["private_segment_fixed_size"] == 0, n
    assert n["group_segment_fixed_size"] == 0, n
    assert n["sgpr_spill_count"] == 0 and n["vgpr_spill_count"] == 0, n
