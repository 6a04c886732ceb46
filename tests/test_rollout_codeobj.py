"""The rollout buffer's kernels in the built code object, through tests/test_episode_log_codeobj.py's reader
(llvm-readelf --notes on a gfx950 code object): they are there, use no scratch and spill nothing.

The library's .hip_fatbin section holds one offload bundle per source file, and that reader unbundles the first one it
finds (sf_api.hip's).  So the section is cut at the bundle magic here, every bundle is wrapped as the .hip_fatbin section of
an object file of its own, and the reader is run on each."""
import os
import subprocess

import pytest

import test_episode_log_codeobj as codeobj
from strikeforce_amd import build

KERNELS = ("k_rollout_record", "k_rollout_returns", "k_rollout_release", "k_rollout_ready", "k_update_actions")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def bundle_notes(so, tmp):
    """kernel_notes of every bundle in the library, merged: mangled name -> notes."""
    fat = os.path.join(tmp, "all.fatbin")
    subprocess.check_call([os.path.join(codeobj.LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fat])
    data = open(fat, "rb").read()
    starts = []
    i = data.find(MAGIC)
    while i >= 0:
        starts.append(i)
        i = data.find(MAGIC, i + 1)
    out = {}
    for n, (a, b) in enumerate(zip(starts, starts[1:] + [len(data)])):
        piece, obj, sub = os.path.join(tmp, "bundle%d.bin" % n), os.path.join(tmp, "bundle%d.o" % n), os.path.join(tmp, "b%d" % n)
        open(piece, "wb").write(data[a:b])
        subprocess.check_call([os.path.join(codeobj.LLVM, "llvm-objcopy"), "-I", "binary", "-O", "elf64-x86-64",
                               "--rename-section", ".data=.hip_fatbin", piece, obj])
        os.mkdir(sub)
        out.update(codeobj.kernel_notes(obj, sub))
    return out, len(starts)


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    so = build.build(verbose=False)
    raw, bundles = bundle_notes(so, str(tmp_path_factory.mktemp("rollout_codeobj")))
    assert bundles == len(build.SOURCES)
    out = {}
    for mangled, v in raw.items():
        if "k_rollout" in mangled or "k_update_actions" in mangled:
            dm = subprocess.check_output(["c++filt", mangled], text=True).strip()
            out[dm.split("(")[0].split("::")[-1]] = v
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_rollout_kernels_are_there_without_scratch_or_spills(notes, kernel):
    assert kernel in notes, (kernel, sorted(notes))
    n = notes[kernel]
    print(kernel, n)
    assert n["private_segment_fixed_size"] == 0 and n["sgpr_spill_count"] == 0, (kernel, n)
    assert n["vgpr_count"] <= 128, (kernel, n)  # (four waves per SIMD at the least: these kernels wait on memory)
