"""k_record, k_record_plan and k_record_copy in the built gfx950 code object, through tests/test_rollout_codeobj.py's reader
(llvm-readelf --notes on every bundle of the library): one instance each, no scratch, no spilled register, LDS only in
the plan kernel (its scan).  VGPR / SGPR counts are printed (pytest -s), not asserted."""
import os
import subprocess

import pytest

import test_rollout_codeobj as rollout
import test_snapshot_codeobj as snap
from strikeforce_amd import build


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    so = build.build(verbose=False)
    tmp = str(tmp_path_factory.mktemp("record_codeobj"))
    raw, bundles = rollout.bundle_notes(so, tmp)  # (leaves every bundle's code object behind: b<n>/gfx950.co)
    assert bundles == len(build.SOURCES)
    out = []
    for n in range(bundles):
        for mangled, v in snap.all_notes(os.path.join(tmp, "b%d" % n, "gfx950.co")).items():
            if "k_record" in mangled:
                out.append((subprocess.check_output(["c++filt", mangled], text=True).strip(), v))
    return out


def test_the_three_kernels_are_there_once_without_scratch_or_spills(notes):
    assert sorted(n.split("(")[0] for n, _ in notes) == ["sf::k_record", "sf::k_record_copy", "sf::k_record_plan"], [n for n, _ in notes]
    for name, n in notes:
        print(name, {k: n[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                                       "sgpr_spill_count", "vgpr_spill_count")})
        assert n["private_segment_fixed_size"] == 0, (name, n)
        assert n["sgpr_spill_count"] == 0 and n["vgpr_spill_count"] == 0, (name, n)
        if "k_record_plan" in name:  # two int64 scan arrays of 1024 and four totals
            assert n["group_segment_fixed_size"] == 2 * 1024 * 8 + 4 * 8, (name, n)
        else:
            assert n["group_segment_fixed_size"] == 0, (name, n)
