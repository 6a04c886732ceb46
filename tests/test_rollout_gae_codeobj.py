"""The continuing record kernel and the two GAE kernels in the built code object, through tests/test_rollout_codeobj.py's
reader: they are there under names of their own, use no scratch, spill nothing and stay within 128 VGPRs; the five
kernels of the per-game rollout are still the plain functions tests/test_rollout_codeobj.py looks up."""
import subprocess

import pytest

import test_rollout_codeobj as rcodeobj
from strikeforce_amd import build

KERNELS = ("k_rollout_record_cont", "k_rollout_gae_v", "k_rollout_gae")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    so = build.build(verbose=False)
    raw, bundles = rcodeobj.bundle_notes(so, str(tmp_path_factory.mktemp("rollout_gae_codeobj")))
    assert bundles == len(build.SOURCES)
    out = {}
    for mangled, v in raw.items():
        if "k_rollout" in mangled:
            dm = subprocess.check_output(["c++filt", mangled], text=True).strip()
            out[dm.split("(")[0].split("::")[-1]] = v
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_gae_kernels_are_there_without_scratch_or_spills(notes, kernel):
    assert kernel in notes, (kernel, sorted(notes))
    n = notes[kernel]
    print(kernel, n)
    assert n["private_segment_fixed_size"] == 0 and n["sgpr_spill_count"] == 0, (kernel, n)
    assert n["vgpr_count"] <= 128, (kernel, n)
    if kernel == "k_rollout_record_cont":
        assert n.get("group_segment_fixed_size", 0) == 0, n  # no LDS


def test_the_per_game_kernels_keep_their_names(notes):
    for kernel in ("k_rollout_record", "k_rollout_returns", "k_rollout_release", "k_rollout_ready"):
        assert kernel in notes, (kernel, sorted(notes))
