"""The fixed-shape step kernels in the built code object (llvm-readelf --notes, as tests/test_episode_log_codeobj.py reads
them): every k_step_fixed instance found (one per line of sf_types.hpp FixedShapes), none with scratch, none with more
registers than the generic instance it stands in for."""
import re
import subprocess

import pytest

from strikeforce_amd import build
from test_episode_log_codeobj import BEFORE, kernel_notes

@pytest.fixture(scope="module")
def fixed(tmp_path_factory):
    so = build.build(verbose=False)
    out = {}
    for mangled, note in kernel_notes(so, str(tmp_path_factory.mktemp("codeobj"))).items():
        m = re.match(r"void sf::k_step_fixed<(.+?)\s*>\(", subprocess.check_output(["c++filt", mangled], text=True).strip())
        if m:
            out[m.group(1)] = note
    return out


def test_fixed_instances_use_no_scratch_and_no_more_registers(fixed):
    assert fixed, "no k_step_fixed instance in the code object"
    for shape, n in fixed.items():
        nb = (int(shape.split("<")[1].split(",")[5]) + 63) // 64  # FixedShape<F, N, M, H, Z, B, ..>: bullet words
        v0, s0 = BEFORE["k_step<%d,0,1,0>" % nb]  # the generic instance of a fixed shape: flag plane and bitmaps in LDS
        print("%s: vgpr %d (generic %d), sgpr spills %d (generic %d)" % (shape, n["vgpr_count"], v0, n["sgpr_spill_count"], s0))
        assert n["private_segment_fixed_size"] == 0, shape
        assert n["vgpr_count"] <= v0 and n["sgpr_spill_count"] < s0, (shape, n)
