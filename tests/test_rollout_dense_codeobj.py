"""sf_rollout_dense's kernels in the built code object, through tests/test_rollout_codeobj.py's reader: one instance per
element type under its own name, no scratch, no spills, at most 128 VGPRs; the eight kernels the rollout buffer already
had are still there under their names."""
import subprocess

import pytest

import test_rollout_codeobj as rcodeobj
from strikeforce_amd import build

KERNELS = ("k_rollout_dense<0>", "k_rollout_dense<1>", "k_rollout_dense<2>")  # f32, bf16, f16
EXISTING = ("k_rollout_record", "k_rollout_returns", "k_rollout_release", "k_rollout_ready", "k_update_actions",
            "k_rollout_record_cont", "k_rollout_gae_v", "k_rollout_gae")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    so = build.build(verbose=False)
    raw, bundles = rcodeobj.bundle_notes(so, str(tmp_path_factory.mktemp("rollout_dense_codeobj")))
    assert bundles == len(build.SOURCES)
    out = {}
    for mangled, v in raw.items():
        if "k_rollout" in mangled or "k_update_actions" in mangled:
            dm = subprocess.check_output(["c++filt", mangled], text=True).strip()
            out[dm.split("(")[0].split("::")[-1]] = v
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_dense_kernels_are_there_without_scratch_or_spills(notes, kernel):
    assert kernel in notes, (kernel, sorted(notes))
    n = notes[kernel]
    print(kernel, n)
    assert n["private_segment_fixed_size"] == 0 and n["sgpr_spill_count"] == 0, (kernel, n)
    assert n["vgpr_count"] <= 128, (kernel, n)


def test_the_existing_rollout_kernels_keep_their_names(notes):
    for kernel in EXISTING:
        assert kernel in notes, (kernel, sorted(notes))
