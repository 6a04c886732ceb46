"""k_reset_sel in the built gfx950 code object (llvm-readelf --notes): there is one instance for every variant k_reset is
built for, and none needs more scratch than the k_reset instance of the same variant in the same library — the parent's
kernel compiled by the same build is the yardstick.  VGPR / SGPR counts are printed (pytest -s), not asserted."""
import re
import subprocess

import pytest

from strikeforce_amd import build
from test_episode_log_codeobj import kernel_notes


def variant_of(mangled):
    dm = subprocess.check_output(["c++filt", mangled], text=True).strip()
    m = re.match(r"void sf::(k_reset|k_reset_sel)<(\d+), (\w+), (\w+), (\w+)>\(", dm)
    if not m:
        return None
    return m.group(1), "<%s,%s>" % (m.group(2), ",".join("1" if m.group(i) == "true" else "0" for i in (3, 4, 5)))


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    so = build.build(verbose=False)
    out = {"k_reset": {}, "k_reset_sel": {}}
    for k, v in kernel_notes(so, str(tmp_path_factory.mktemp("codeobj"))).items():
        kv = variant_of(k)
        if kv:
            out[kv[0]][kv[1]] = v
    return out


def test_every_reset_variant_has_its_selective_instance(notes):
    assert len(notes["k_reset"]) == 15  # NB 1..4 x three plane variants, and the three large-pool ones (sf_types.hpp)
    assert set(notes["k_reset_sel"]) == set(notes["k_reset"])


def test_no_instance_needs_more_scratch_than_k_reset(notes):
    rows = []
    for v in sorted(notes["k_reset"]):
        r, s = notes["k_reset"][v], notes["k_reset_sel"][v]
        rows.append("%-10s k_reset: vgpr %3d sgpr spills %3d scratch %4d | k_reset_sel: vgpr %3d sgpr spills %3d scratch %4d"
                    % (v, r["vgpr_count"], r["sgpr_spill_count"], r["private_segment_fixed_size"],
                       s["vgpr_count"], s["sgpr_spill_count"], s["private_segment_fixed_size"]))
    print("\n".join(rows))
    for v in notes["k_reset"]:
        assert notes["k_reset_sel"][v]["private_segment_fixed_size"] <= notes["k_reset"][v]["private_segment_fixed_size"], v
