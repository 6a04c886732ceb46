"""The two fixed-shape step kernels in the built code object after their step loop was made leaner (sf_core.hpp, the parts
under SH::FIXED): no scratch, and no more VGPRs or SGPR spills than the same kernels had in the parent commit.  The
parent's numbers were read from a build of the parent commit (llvm-readelf --notes, as tests/test_episode_log_codeobj.py
reads them)."""
import re
import subprocess

import pytest

from strikeforce_amd import build
from test_episode_log_codeobj import kernel_notes

# FixedShape<..> arguments as c++filt prints them: (vgpr_count, sgpr_spill_count) in the parent commit
PARENT = {
    "1, 64, 64, 8, 24, 64, 1, 1, 1, 1, 0": (122, 93),  # BASELINE configs[2]
    "1, 64, 64, 1, 16, 32, 0, 1, 1, 1, 0": (95, 71),   # BASELINE configs[1]
}


@pytest.fixture(scope="module")
def fixed(tmp_path_factory):
    so = build.build(verbose=False)
    out = {}
    for mangled, note in kernel_notes(so, str(tmp_path_factory.mktemp("codeobj"))).items():
        m = re.match(r"void sf::k_step_fixed<sf::FixedShape<(.+?)>\s*>\(", subprocess.check_output(["c++filt", mangled], text=True).strip())
        if m:
            out[m.group(1)] = note
    return out


@pytest.mark.parametrize("shape", sorted(PARENT))
def test_fixed_instance_keeps_the_parents_register_budget(fixed, shape):
    assert shape in fixed, "no k_step_fixed<FixedShape<%s>> in the code object (%s)" % (shape, sorted(fixed))
    n, (v0, s0) = fixed[shape], PARENT[shape]
    print("FixedShape<%s>: vgpr %d (parent %d), sgpr spills %d (parent %d), scratch %d"
          % (shape, n["vgpr_count"], v0, n["sgpr_spill_count"], s0, n["private_segment_fixed_size"]))
    assert n["private_segment_fixed_size"] == 0
    assert n["vgpr_count"] <= v0
    assert n["sgpr_spill_count"] <= s0
