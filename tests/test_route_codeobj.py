"""The route kernels in the built code object, through tests/test_rollout_codeobj.py's per-bundle reader (llvm-readelf
--notes on the gfx950 code objects of the library): both are there, use no scratch and spill nothing."""
import subprocess

import pytest

import test_rollout_codeobj as bundles
from strikeforce_amd import build

KERNELS = ("k_route_gather", "k_route_scatter")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    so = build.build(verbose=False)
    raw, count = bundles.bundle_notes(so, str(tmp_path_factory.mktemp("route_codeobj")))
    assert count == len(build.SOURCES)
    out = {}
    for mangled, v in raw.items():
        if "k_route" in mangled:
            dm = subprocess.check_output(["c++filt", mangled], text=True).strip()
            out[dm.split("(")[0].split("::")[-1]] = v
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_route_kernels_are_there_without_scratch_or_spills(notes, kernel):
    assert kernel in notes, (kernel, sorted(notes))
    n = notes[kernel]
    print(kernel, n)
    assert n["private_segment_fixed_size"] == 0 and n["sgpr_spill_count"] == 0, (kernel, n)
    assert n["vgpr_count"] <= 128, (kernel, n)  # (four waves per SIMD at the least: these kernels wait on memory)
