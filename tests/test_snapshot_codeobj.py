"""The snapshot kernels in the built gfx950 code object, through tests/test_rollout_codeobj.py's reader (llvm-readelf --notes on
every bundle of the library): k_snapshot has one instance per direction — not one per <NB, HP, BM, ZL> — and k_memory_rows is
there; none uses scratch, LDS or a spilled register.  VGPR / SGPR counts are printed (pytest -s)."""
import os
import re
import subprocess

import pytest

import test_episode_log_codeobj as codeobj
import test_rollout_codeobj as rollout
from strikeforce_amd import build

KERNELS = ("k_snapshot<true>", "k_snapshot<false>", "k_memory_rows<true>", "k_memory_rows<false>")


def all_notes(co):
    """kernel symbol -> {note: int} of one code object, every numeric note."""
    txt = subprocess.check_output([os.path.join(codeobj.LLVM, "llvm-readelf"), "--notes", co], text=True)
    out = {}
    for blk in re.split(r"\n\s*- \.agpr_count", txt)[1:]:
        m = re.search(r"\.symbol:\s+(\S+)\.kd", blk)
        if m:
            out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", ".agpr_count" + blk, re.M)}
    return out


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    so = build.build(verbose=False)
    tmp = str(tmp_path_factory.mktemp("snapshot_codeobj"))
    raw, bundles = rollout.bundle_notes(so, tmp)  # (leaves every bundle's code object behind: b<n>/gfx950.co)
    assert bundles == len(build.SOURCES)
    out = {}
    for n in range(bundles):
        for mangled, v in all_notes(os.path.join(tmp, "b%d" % n, "gfx950.co")).items():
            if "k_snapshot" in mangled or "k_memory_rows" in mangled:
                dm = subprocess.check_output(["c++filt", mangled], text=True).strip()
                out[re.sub(r"^void ", "", dm).split("(")[0].split("::")[-1]] = v
    return out


def test_one_instance_per_direction(notes):
    assert sorted(k for k in notes if k.startswith("k_snapshot")) == ["k_snapshot<false>", "k_snapshot<true>"], sorted(notes)


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernels_are_there_without_scratch_lds_or_spills(notes, kernel):
    assert kernel in notes, (kernel, sorted(notes))
    n = notes[kernel]
    print(kernel, {k: n[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                                     "sgpr_spill_count", "vgpr_spill_count")})
    assert n["private_segment_fixed_size"] == 0 and n["group_segment_fixed_size"] == 0, (kernel, n)
    assert n["sgpr_spill_count"] == 0 and n["vgpr_spill_count"] == 0, (kernel, n)
    assert n["vgpr_count"] <= 64, (kernel, n)  # (a copy kernel waits on memory: eight waves per SIMD)
