"""sf_policy_load_weights' kernels in the built code object, through tests/test_rollout_codeobj.py's reader
(llvm-readelf --notes on every gfx950 bundle of the library): k_load_stage and k_digest are there, use no scratch, spill
nothing and use no LDS; the table k_load_stage walks fits the kernel arguments."""
import subprocess

import pytest

import test_rollout_codeobj as bundles
from strikeforce_amd import build

KERNELS = ("k_load_stage", "k_digest")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    so = build.build(verbose=False)
    raw, n = bundles.bundle_notes(so, str(tmp_path_factory.mktemp("policy_load_codeobj")))
    assert n == len(build.SOURCES)
    out = {}
    for mangled, v in raw.items():
        if "k_load_stage" in mangled or "k_digest" in mangled:
            dm = subprocess.check_output(["c++filt", mangled], text=True).strip()
            out[dm.split("(")[0].split("::")[-1]] = v
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_load_kernels_are_there_without_scratch_or_spills(notes, kernel):
    assert kernel in notes, (kernel, sorted(notes))
    n = notes[kernel]
    print(kernel, n)
    assert n["private_segment_fixed_size"] == 0 and n["sgpr_spill_count"] == 0, (kernel, n)
    assert n["vgpr_count"] <= 64, (kernel, n)  # (eight waves per SIMD: a gather and a store per thread, nothing to hold)
