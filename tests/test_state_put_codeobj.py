"""k_put_init, k_put_check and k_put_write in the built gfx950 code object, through tests/test_rollout_codeobj.py's reader
(llvm-readelf --notes on every bundle of the library): one instance each, no scratch, no spilled register, at most 128
VGPRs; the check and the write hold exactly the transpose buffer in LDS (64 human records of 28 words at the odd row
stride of 29), the init none.  VGPR / SGPR counts are printed (pytest -s)."""
import os
import subprocess

import pytest

import test_rollout_codeobj as rollout
import test_snapshot_codeobj as snap
from strikeforce_amd import build


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    so = build.build(verbose=False)
    tmp = str(tmp_path_factory.mktemp("put_codeobj"))
    raw, bundles = rollout.bundle_notes(so, tmp)  # (leaves every bundle's code object behind: b<n>/gfx950.co)
    assert bundles == len(build.SOURCES)
    out = {}
    for n in range(bundles):
        for mangled, v in snap.all_notes(os.path.join(tmp, "b%d" % n, "gfx950.co")).items():
            if "k_put_" in mangled:
                out[subprocess.check_output(["c++filt", mangled], text=True).strip()] = v
    return out


def test_the_three_kernels_are_there_once_without_scratch_or_spills(notes):
    assert sorted(n.split("(")[0] for n in notes) == ["sf::k_put_check", "sf::k_put_init", "sf::k_put_write"], sorted(notes)
    for name, n in notes.items():
        print(name, {k: n[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                                       "sgpr_spill_count", "vgpr_spill_count")})
        assert n["private_segment_fixed_size"] == 0, (name, n)
        assert n["sgpr_spill_count"] == 0 and n["vgpr_spill_count"] == 0, (name, n)
        assert n["vgpr_count"] <= 128, (name, n)
        assert n["group_segment_fixed_size"] == (0 if "k_put_init" in name else 64 * 29 * 4), (name, n)
