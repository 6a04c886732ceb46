"""k_action_mask and k_act_masked in the built gfx950 code object, through tests/test_rollout_codeobj.py's reader
(llvm-readelf --notes on every bundle of the library): one instance each, no scratch, no LDS, no spilled register.  VGPR / SGPR
counts are printed (pytest -s), not asserted.  Only the notes are read, no instruction text."""
import os
import subprocess

import pytest

import test_rollout_codeobj as rollout
import test_snapshot_codeobj as snap
from strikeforce_amd import build

KERNELS = ("k_action_mask", "k_act_masked")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    so = build.build(verbose=False)
    tmp = str(tmp_path_factory.mktemp("action_mask_codeobj"))
    raw, bundles = rollout.bundle_notes(so, tmp)  # (leaves every bundle's code object behind: b<n>/gfx950.co)
    assert bundles == len(build.SOURCES)
    out = {k: {} for k in KERNELS}
    for n in range(bundles):
        for mangled, v in snap.all_notes(os.path.join(tmp, "b%d" % n, "gfx950.co")).items():
            for k in KERNELS:
                if k in mangled:
                    out[k][subprocess.check_output(["c++filt", mangled], text=True).strip()] = v
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernel_is_there_once_without_scratch_lds_or_spills(notes, kernel):
    assert len(notes[kernel]) == 1, sorted(notes[kernel])
    (name, n), = notes[kernel].items()
    print(name, {k: n[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                                   "sgpr_spill_count", "vgpr_spill_count")})
    assert n["private_segment_fixed_size"] == 0, n
    assert n["group_segment_fixed_size"] == 0, n
    assert n["sgpr_spill_count"] == 0 and n["vgpr_spill_count"] == 0, n
