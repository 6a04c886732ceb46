"""The episode log in the built code object (llvm-readelf --notes on the gfx950 code object inside the .so): its kernels
are there, its entry points are exported, and the step kernels keep the register budget the parent commit's numbers
below set.  Every k_step / k_step_half / k_reset variant launched with the log off is built without log code and may not
use one VGPR or one SGPR spill more, nor any scratch.  The k_step instances launched while the log is on (k_step<.., LOG>,
sf_core.hpp latch_results<true>) may not use a VGPR more than their variant did, nor scratch, and on the variants the
BASELINE configurations C1-C5 run at most 4 more SGPR spills (to VGPR lanes)."""
import os
import re
import subprocess

import pytest

from strikeforce_amd import build, env

LLVM = "/opt/rocm/lib/llvm/bin"

# (vgpr_count, sgpr_spill_count) before the episode log; key: kernel<NB, HBM_PLANE, BITMAPS, ZL>
BEFORE = {
    "k_reset<1,0,1,0>": (42, 4),
    "k_reset<1,1,0,0>": (42, 0),
    "k_reset<1,1,1,0>": (42, 0),
    "k_reset<2,0,1,0>": (42, 4),
    "k_reset<2,1,0,0>": (42, 0),
    "k_reset<2,1,1,0>": (42, 0),
    "k_reset<3,0,1,0>": (42, 4),
    "k_reset<3,1,0,0>": (42, 0),
    "k_reset<3,1,1,0>": (42, 0),
    "k_reset<4,0,1,0>": (42, 4),
    "k_reset<4,0,1,1>": (40, 17),
    "k_reset<4,1,0,0>": (42, 0),
    "k_reset<4,1,0,1>": (38, 16),
    "k_reset<4,1,1,0>": (42, 0),
    "k_reset<4,1,1,1>": (39, 17),
    "k_step<1,0,1,0>": (123, 179),
    "k_step<1,1,0,0>": (120, 157),
    "k_step<1,1,1,0>": (119, 178),
    "k_step<2,0,1,0>": (135, 186),
    "k_step<2,1,0,0>": (131, 170),
    "k_step<2,1,1,0>": (132, 195),
    "k_step<3,0,1,0>": (148, 211),
    "k_step<3,1,0,0>": (143, 176),
    "k_step<3,1,1,0>": (144, 203),
    "k_step<4,0,1,0>": (160, 218),
    "k_step<4,0,1,1>": (172, 213),
    "k_step<4,1,0,0>": (155, 182),
    "k_step<4,1,0,1>": (161, 219),
    "k_step<4,1,1,0>": (156, 195),
    "k_step<4,1,1,1>": (168, 225),
    "k_step_half<1,0,1,0>": (131, 166),
    "k_step_half<1,1,0,0>": (127, 138),
    "k_step_half<1,1,1,0>": (127, 146),
    "k_step_half<2,0,1,0>": (147, 174),
    "k_step_half<2,1,0,0>": (143, 157),
    "k_step_half<2,1,1,0>": (143, 174),
    "k_step_half<3,0,1,0>": (163, 174),
    "k_step_half<3,1,0,0>": (159, 167),
    "k_step_half<3,1,1,0>": (159, 188),
    "k_step_half<4,0,1,0>": (179, 208),
    "k_step_half<4,0,1,1>": (179, 234),
    "k_step_half<4,1,0,0>": (176, 204),
    "k_step_half<4,1,0,1>": (181, 217),
    "k_step_half<4,1,1,0>": (175, 195),
    "k_step_half<4,1,1,1>": (175, 207),
}
# the variants C1-C5 run: C1 / C2 / C3 (LDS plane, one bullet word), C4 (128 x 128: HBM plane with bitmaps), C5
# (256 x 256, 128 bullets: HBM plane, no bitmaps, two bullet words)
BASELINE_VARIANTS = {"<1,0,1,0>", "<1,1,1,0>", "<2,1,0,0>"}


def kernel_notes(so, tmp):
    fat, co = os.path.join(tmp, "lib.fatbin"), os.path.join(tmp, "gfx950.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
    txt = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    out, cur = {}, None
    for ln in txt.splitlines():
        s = ln.strip()
        m = re.match(r"^-?\s*\.name:\s+(\S+)", s)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.match(r"^\.(vgpr_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)", s)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


def short_name(mangled):
    dm = subprocess.check_output(["c++filt", mangled], text=True).strip()
    m = re.match(r"void sf::(k_step|k_step_half|k_reset)<(\d+), (\w+), (\w+), (\w+)(?:, (\w+))?>", dm)
    if m:
        flags = ",".join("1" if m.group(i) == "true" else "0" for i in (3, 4, 5))
        return "%s<%s,%s>%s" % (m.group(1), m.group(2), flags, "+log" if m.group(6) == "true" else "")
    m = re.match(r"(?:void )?sf::(k_\w+)\(", dm)
    return m.group(1) if m else dm


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    so = build.build(verbose=False)
    raw = kernel_notes(so, str(tmp_path_factory.mktemp("codeobj")))
    return {short_name(k): v for k, v in raw.items()}


def test_collection_kernels_are_in_the_code_object(notes):
    for k in ("k_ep_plan", "k_ep_copy", "k_ep_late"):
        assert k in notes, k
        assert notes[k]["private_segment_fixed_size"] == 0


def test_step_kernels_keep_their_registers(notes):
    rows = []
    for k, (v0, s0) in sorted(BEFORE.items()):
        n, lg = notes[k], notes.get(k + "+log")
        row = "%-22s vgpr %3d -> %3d   sgpr spills %3d -> %3d" % (k, v0, n["vgpr_count"], s0, n["sgpr_spill_count"])
        if lg:
            row += "   | log on: vgpr %3d, sgpr spills %3d" % (lg["vgpr_count"], lg["sgpr_spill_count"])
        rows.append(row)
    print("\n".join(rows))  # (pytest -s: the before / after table)
    assert set(BEFORE) <= set(notes)
    for k, (v0, s0) in BEFORE.items():
        n = notes[k]  # log off: no log code
        assert n["private_segment_fixed_size"] == 0, (k, n)
        assert n["vgpr_count"] <= v0 and n["sgpr_spill_count"] <= s0, (k, v0, s0, n)
        if not k.startswith("k_step<"):
            assert k + "+log" not in notes  # k_step_half and k_reset have no log instance (k_ep_late)
            continue
        lg = notes[k + "+log"]  # log on
        assert lg["private_segment_fixed_size"] == 0, (k, lg)
        assert lg["vgpr_count"] <= v0, (k, v0, lg)
        if k[k.index("<"):] in BASELINE_VARIANTS:
            assert lg["sgpr_spill_count"] <= s0 + 4, (k, s0, lg)


def test_episode_log_entry_points_are_exported():
    L = env.load_library()
    for name in ("sf_episode_log", "sf_episodes", "sf_episodes_device", "sf_episode_ring", "sf_episodes_allgather"):
        assert hasattr(L, name), name
        assert name in env.EXPORTS
