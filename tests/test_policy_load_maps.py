"""The index maps sf_policy_load_weights' kernel evaluates (csrc/sf_policy_stage_map.hpp: destination index -> source index
or "zero", and the f32 -> 3 x bf16 split), on the CPU: tests/policy_load/map_main.cpp is built with AddressSanitizer and
UBSan and run as a child process.  It builds every image through the maps, one destination element at a time as the kernel's
threads do, and compares it BIT FOR BIT with the image sf_policy_stage.hpp's functions build for sf_policy_create — at the
network's real shapes, at the small shapes of tests/test_policy_stage.py and at odd ones, with split inputs that tie, round up
into the next exponent or into infinity, are zero, denormal or infinite.  Sources lie in heap blocks of exactly their size: a
map that points outside one is a sanitizer report, which ends the program with a non-zero status."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "policy_load", "map_main.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

# case -> elements of its image (halves for a split image)
CASES = {
    "tiles/gru": 480 * 160, "tiles/gru/plain": 480 * 160, "tiles/res": 160 * 160, "tiles/res/plain": 160 * 160,
    "tiles/comb-padded": 160 * 352, "tiles/policy-head-padded": 16 * 160, "tiles/value-head-padded": 16 * 160,
    "tiles/32x32": 1024, "tiles/32x32/plain": 1024, "tiles/16x352": 16 * 352, "tiles/16x352/plain": 16 * 352, "tiles/odd-corner": 32 * 48,
    "pad/comb": 160 * 352, "pad/policy-head": 16 * 160, "pad/value-head": 16 * 160, "pad/policy-bias": 16, "pad/value-bias": 16, "pad/odd": 77,
    "conv0/160x288": 160 * 288, "conv0/5x7": 35, "conv0/1x9": 9,
    "perm/160x160": 160 * 160 * 9, "perm/3x5": 135, "perm/7x1": 63,
    "split/conv-permuted": 160 * 1440 * 3, "split/320x32": 320 * 32 * 3, "split/specials": 90,
}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("policy_load")
    out = str(d / "map_main")
    r = subprocess.run(["g++"] + FLAGS + [SRC, "-o", out], capture_output=True, text=True)
    if r.returncode:
        probe = d / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++"] + FLAGS + [str(probe), "-o", str(d / "probe")], capture_output=True).returncode:
            pytest.skip("g++ cannot link the sanitizer runtimes")
        pytest.fail("map_main.cpp does not build:\n" + r.stderr)
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr  # (a mismatch or a sanitizer report)
    return r.stdout.splitlines()


def test_every_image_built_through_the_maps_equals_the_staged_one_bit_for_bit(lines):
    assert not [ln for ln in lines if ln.startswith("MISMATCH")], lines
    got = {}
    for ln in lines:
        ok, name, n = ln.split()
        assert ok == "ok"
        got[name] = int(n)
    assert got == CASES


def test_the_map_header_is_plain_cxx_and_the_kernels_use_it():
    """The header is HIP-free (this program built it with g++), and sf_policy_load.hpp — the kernels — includes it and
    restates no layout of its own: every map call there goes through smap::."""
    csrc = os.path.join(ROOT, "strikeforce_amd", "csrc")
    hdr = open(os.path.join(csrc, "sf_policy_stage_map.hpp")).read()
    assert "hip/" not in hdr and "#include <hip" not in hdr
    load = open(os.path.join(csrc, "sf_policy_load.hpp")).read()
    assert '#include "sf_policy_stage_map.hpp"' in load
    for fn in ("split_of_permute", "split3", "conv0_transpose", "conv_permute", "tiles_of_pad", "pad"):
        assert "smap::%s(" % fn in load, fn
    assert '#include "sf_policy_load.hpp"' in open(os.path.join(csrc, "sf_policy.hip")).read()
