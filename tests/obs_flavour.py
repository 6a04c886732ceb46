"""A build of sf_api.hip alone with SMALL observation limits (tests/libsf_obs_small.so, git-ignored), so that ordinary worlds
take the fallbacks that no game reaches at the product's limits: the dense kernel's pow queue overflow (values mapped in
place), the list kernel's (the same, past the host-built table), its cell limit and last compaction pass at 65..128 cells,
mode 3's unstaged branch, and spills / crowded markers in most steps.  Test helper only.

The limits are compile-time constants of sf_obs_kernels.hpp (which sf_api.hip includes) with #ifndef defaults; nothing
else differs from the product build, and the product build defines none of them.  Loaded through SF_LIBRARY_PATH in a child process (the path is read once per
process): tests/obs_edges_child.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "strikeforce_amd", "csrc")
LIB = os.path.join(ROOT, "tests", "libsf_obs_small.so")

# the product's limits (the #ifndef defaults in sf_obs_kernels.hpp) and the small flavour's.  rec = own records of the
# dense kernel (OBS_REC_MAX less its 8 shared class records), list = its pow queue, staged = mode 3's staging area;
# ol_* = k_observe_list's own records, pow queue and non-empty cells.
PRODUCT = {"rec": 64, "list": 256, "staged": 1922, "ol_rec": 48, "ol_powq": 384, "ol_cells": 640}
SMALL = {"rec": 16, "list": 16, "staged": 256, "ol_rec": 30, "ol_powq": 16, "ol_cells": 128}
# (OL_REC cannot go below 30: the occupant words of a window share the record area, OL_REC * 33 >= 964)


def flags(limits=SMALL):
    return ["-DSF_OBS_REC_MAX=%d" % (8 + limits["rec"]), "-DSF_OBS_LIST_MAX=%d" % limits["list"],
            "-DSF_OBS_STAGED=%d" % limits["staged"], "-DSF_OL_REC=%d" % limits["ol_rec"],
            "-DSF_OL_POWQ=%d" % limits["ol_powq"], "-DSF_OL_CELLS=%d" % limits["ol_cells"]]


def stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if not f.startswith("sf_policy")]
    deps += [os.path.join(ROOT, "include", "strikeforce.h"), os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def lib():
    """Path of the small-limits library, built first if it is missing or older than its sources."""
    if stale():
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared"] + flags() + ["-o", LIB, "sf_api.hip"]
        subprocess.check_call(cmd, cwd=CSRC)
    return LIB


if __name__ == "__main__":
    print(lib())
