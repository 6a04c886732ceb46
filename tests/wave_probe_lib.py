"""Loader and runner of the wave-backend probes (tests/wave_probe/): libsf_wave_probe_emu.so runs them on the CPU wave
emulator, tests/libsf_wave_probe.so (git-ignored) on the device backend, built with the product's flags.  Test helper only.

run(backend, probe, cases, ...) fills a PArgs (tests/wave_probe/probe_body.hpp) from numpy arrays, checks every index
the case list hands the probe against the size of the region it indexes, runs the probe and returns all arrays, the
result rows and scalars prefilled with FILL so that a word nobody wrote is seen as such."""
import ctypes as C
import os
import subprocess
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "strikeforce_amd", "csrc")
DIR = os.path.join(ROOT, "tests", "wave_probe")
LIB = os.path.join(ROOT, "tests", "libsf_wave_probe.so")
FILL = 0xA5A5A5A5
LOGT_OFF = 1024
LOGT_ENTRIES = LOGT_OFF + 65537
RNG_WORDS, SC_WORDS = 18, 24
SC_JOMLE, SC_WARM = 5, 16

PROBES = """lane_all shl1 sum18_row1 readlane setlane uni ballot frombits rank_below bits64 popc0
select sar31 le0 gts ltu minu shrv shlv mul24 mul24_su mad24
lds_store_u8 lds_store_u32 ulds_store ulds_load lds_u8 lds_u32 lds_or_u32 lds_or_rtn_u32
lds_zero copy_g2l g2l_split1 g2l_split2 g2l_split4 copy_l2g
gload gload_u8 gload_u16 gstore gstore_u8 gload_u16_at u_i32 u_i16
pow_bytes pow_pair log_pow rng_round rng_split rng_reduce
gen_srand gen_prewarm gen_draw gen_draw_core""".split()
# probes of operations the emulator does not have (the core calls them only from code the emulator never instantiates)
DEVICE_ONLY = ("uni", "rank_below", "gstore_u8")

_PTRS = ["in0", "in1", "in2", "in3", "s0", "s1", "s2", "s3", "out0", "out1", "out2", "so", "g", "limg"]


class PArgs(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in _PTRS]
                + [(n, C.c_uint32) for n in ("so_n", "g_stride", "l_stride", "cases")]
                + [(n, C.c_void_p) for n in ("logt", "exptab", "rng", "rng2", "scal")]
                + [("A", C.c_int32), ("per", C.c_int32)])


class PSizes(C.Structure):
    _fields_ = [("v", C.c_uint64 * 17)]


_SIZE_ORDER = _PTRS + ["rng", "rng2", "scal"]


def stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in ("wave_gfx950.hpp", "sf_core.hpp", "sf_host.hpp", "sf_types.hpp", "sf_obs.hpp")]
    deps += [os.path.join(DIR, "probe_gfx950.hip"), os.path.join(DIR, "probe_body.hpp"),
             os.path.join(ROOT, "include", "strikeforce.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def lib():
    """Path of the device probe library, built first if it is missing or older than its sources."""
    if stale():
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-o", LIB, "probe_gfx950.hip"]
        subprocess.check_call(cmd, cwd=DIR)
    return LIB


_LIBS = {}


def emu_lib():
    if "emu" not in _LIBS:
        subprocess.check_call(["make", "-s", "-C", DIR, "libsf_wave_probe_emu.so"])
        L = C.CDLL(os.path.join(DIR, "libsf_wave_probe_emu.so"))
        L.sfpe_sum_bias_lane.restype = C.c_uint32
        _LIBS["emu"] = L
    return _LIBS["emu"]


def gpu_lib():
    if "gpu" not in _LIBS:
        _LIBS["gpu"] = C.CDLL(lib())
    return _LIBS["gpu"]


def tables(backend="emu"):
    """(logt, exptab) as the product's host code builds them (sf_host.hpp build_rng_tables), from the library itself."""
    key = "tables_" + backend
    if key not in _LIBS:
        logt = np.full(LOGT_ENTRIES, 0xFFFF, dtype=np.uint16)
        exptab = np.full(512, FILL, dtype=np.uint32)
        fn = emu_lib().sfpe_tables if backend == "emu" else gpu_lib().sfp_tables
        fn(C.c_void_p(logt.ctypes.data), C.c_void_p(exptab.ctypes.data))
        _LIBS[key] = (logt, exptab)
    return _LIBS[key]


# what a probe indexes with which input: (field, bytes per element, region, "idx" | "cnt")
_INDEXED = {
    "lds_store_u8": [("in0", 1, "l", "idx")], "lds_store_u32": [("in0", 4, "l", "idx")],
    "ulds_store": [("s0", 1, "l", "idx"), ("s2", 4, "l", "idx")], "ulds_load": [("s0", 1, "l", "idx"), ("s2", 4, "l", "idx")],
    "lds_u8": [("in0", 1, "l", "idx")], "lds_u32": [("in0", 4, "l", "idx")],
    "lds_or_u32": [("in0", 4, "l", "idx")], "lds_or_rtn_u32": [("in0", 4, "l", "idx")],
    "lds_zero": [("s0", 4, "l", "cnt")],
    "copy_g2l": [("s0", 1, "l", "cnt"), ("s0", 1, "g", "cnt")], "copy_l2g": [("s0", 1, "l", "cnt"), ("s0", 1, "g", "cnt")],
    "g2l_split1": [("s0", 1, "l", "cnt"), ("s0", 1, "g", "cnt")], "g2l_split2": [("s0", 1, "l", "cnt"), ("s0", 1, "g", "cnt")],
    "g2l_split4": [("s0", 1, "l", "cnt"), ("s0", 1, "g", "cnt")],
    "gload": [("in0", 4, "g", "idx")], "gload_u8": [("in0", 1, "g", "idx")], "gload_u16": [("in0", 2, "g", "idx")],
    "gstore": [("in0", 4, "g", "idx")], "gstore_u8": [("in0", 1, "g", "idx")],
    "u_i32": [("s0", 4, "g", "idx"), ("s1", 4, "g", "idx")], "u_i16": [("s0", 2, "g", "idx"), ("s1", 2, "g", "idx")],
}
_ROWS = {"readlane": ["s0"], "setlane": ["s0"], "uni": ["s0"]}  # lane numbers
_NEED = {  # the arrays a probe reads or writes: all of them must be there
    "lane_all": [], "shl1": ["in0"], "sum18_row1": ["in0"], "readlane": ["in0", "s0", "so"], "setlane": ["in0", "s0", "s1"],
    "uni": ["in0", "in1", "s0"], "ballot": ["in2", "so"], "frombits": ["s0", "s1"], "rank_below": ["s0", "s1"],
    "bits64": ["s0", "s1", "so"], "popc0": ["s0", "s1", "so"], "select": ["in0", "in1", "in2"], "sar31": ["in0"], "le0": ["in0"],
    "gts": ["in0", "in1"], "ltu": ["in0", "in1", "s0"], "minu": ["in0", "in1"], "shrv": ["in0", "in1"], "shlv": ["in0", "in1"],
    "mul24": ["in0", "in1"], "mul24_su": ["s0", "in1"], "mad24": ["in0", "s0", "in1"],
    "lds_store_u8": ["in0", "in1", "in2", "limg"], "lds_store_u32": ["in0", "in1", "in2", "limg"],
    "ulds_store": ["s0", "s1", "s2", "s3", "limg"], "ulds_load": ["s0", "s2", "so", "limg"],
    "lds_u8": ["in0", "in2", "limg"], "lds_u32": ["in0", "in2", "limg"], "lds_or_u32": ["in0", "in1", "in2", "limg"],
    "lds_or_rtn_u32": ["in0", "in1", "in2", "limg"], "lds_zero": ["s0", "limg"],
    "copy_g2l": ["s0", "g", "limg"], "g2l_split1": ["s0", "g", "limg"], "g2l_split2": ["s0", "g", "limg"],
    "g2l_split4": ["s0", "g", "limg"], "copy_l2g": ["s0", "g", "limg"],
    "gload": ["in0", "in2", "g"], "gload_u8": ["in0", "in2", "g"], "gload_u16": ["in0", "in2", "g"],
    "gstore": ["in0", "in1", "in2", "g"], "gstore_u8": ["in0", "in1", "in2", "g"], "gload_u16_at": ["in0"],
    "u_i32": ["s0", "s1", "s2", "so", "g"], "u_i16": ["s0", "s1", "s2", "so", "g"],
    "pow_bytes": ["in0"], "pow_pair": ["in0"], "log_pow": ["in0"],
    "rng_round": ["in0", "in1", "in2", "in3", "s0", "so"], "rng_split": ["in0", "in1", "in2", "in3", "s0", "so"],
    "rng_reduce": ["in0", "in1", "in2"],
    "gen_srand": ["s0", "s1", "s2", "s3", "so", "rng", "rng2", "scal"], "gen_prewarm": ["s0", "s1", "so", "rng", "rng2", "scal"],
    "gen_draw": ["so", "rng", "rng2", "scal"], "gen_draw_core": ["so", "rng", "rng2", "scal"],
}
_SO_MIN = {"readlane": 1, "ballot": 2, "bits64": 3, "popc0": 1, "ulds_load": 2, "u_i32": 2, "u_i16": 2, "rng_round": 1,
           "rng_split": 1, "gen_prewarm": 1}


def _check(probe, cases, a, so_n, g_stride, l_stride, A, per):
    """Nothing a probe does may leave the arrays it was given: the case lists are checked here, before any launch."""
    for n in _NEED[probe]:
        assert n == "so" or a.get(n) is not None, (probe, n)
    assert so_n >= _SO_MIN.get(probe, 0), probe
    stride = {"l": l_stride, "g": g_stride}
    for field, unit, region, kind in _INDEXED.get(probe, []):
        top = int(a[field].max())
        assert (top + (1 if kind == "idx" else 0)) * unit <= stride[region], (probe, field, top, stride[region])
    for field in _ROWS.get(probe, []):
        assert int(a[field].max()) < 64, (probe, field)
    if probe in ("copy_g2l", "copy_l2g", "g2l_split1", "g2l_split2", "g2l_split4"):
        assert g_stride % 16 == 0 and l_stride % 16 == 0 and not (a["s0"] % 16).any(), probe
        if probe.startswith("g2l_split"):
            assert int(a["s0"].max()) <= 1024 * int(probe[-1]), probe
    if probe == "lds_zero":
        assert not (a["s0"] % 4).any()
    if probe in ("shrv", "shlv"):
        assert int(a["in1"].max()) < 32
    if probe == "gload_u16_at":
        assert int(a["in0"].max()) <= 2 * (LOGT_ENTRIES - 1) and not (a["in0"] % 2).any()
    if probe == "log_pow":
        assert 1 <= int(a["in0"].min()) and int(a["in0"].max()) <= 65536
    if probe.startswith("gen_"):
        assert per >= 1 and A == cases * per, probe
        assert a["rng"].size == A * RNG_WORDS and a["rng2"].size == A * RNG_WORDS and a["scal"].size == A * SC_WORDS
        for w in (a["rng"], a["rng2"]):  # values index the log table, digits bound the tap sum (sf_core.hpp SUM_BIAS_LANE)
            assert int((w & 0xFFFFF).max()) <= 0x1FFFF and int(((w >> 20) & 15).max()) <= 10 and int((w >> 24).max()) <= 10
        assert int((a["rng"] & 0xFFFFF).max()) <= 65536
        if probe == "gen_srand":
            assert so_n % 512 == 0 and per == so_n // 512
        if probe == "gen_prewarm":
            assert int(a["s1"].max()) <= 1024


def run(backend, probe, cases, so_n=0, per=1, **arrays):
    """Run `probe` on "emu" or "gpu" for `cases` cases.  arrays: in0..in3 [cases][64], s0..s3 [cases], g / limg
    [cases][stride] bytes, rng / rng2 [A][18], scal [A][24].  Returns every array as it is afterwards."""
    assert probe in PROBES and backend in ("emu", "gpu") and cases >= 1
    a = {}
    for n in ("in0", "in1", "in2", "in3"):
        if arrays.get(n) is not None:
            a[n] = np.ascontiguousarray(arrays[n], dtype=np.uint32).reshape(cases, 64).copy()
    for n in ("s0", "s1", "s2", "s3"):
        if arrays.get(n) is not None:
            a[n] = np.ascontiguousarray(arrays[n], dtype=np.uint32).reshape(cases).copy()
    for n in ("g", "limg"):
        if arrays.get(n) is not None:
            a[n] = np.ascontiguousarray(arrays[n], dtype=np.uint8).reshape(cases, -1).copy()
    for n in ("rng", "rng2"):
        if arrays.get(n) is not None:
            a[n] = np.ascontiguousarray(arrays[n], dtype=np.uint32).reshape(-1, RNG_WORDS).copy()
    if arrays.get("scal") is not None:
        a["scal"] = np.ascontiguousarray(arrays["scal"], dtype=np.uint32).reshape(-1, SC_WORDS).copy()
    assert set(arrays) <= set(a), "unknown or empty array among %s" % sorted(arrays)
    for n in ("out0", "out1", "out2"):
        a[n] = np.full((cases, 64), FILL, dtype=np.uint32)
    a["so"] = np.full((cases, max(so_n, 1)), FILL, dtype=np.uint32)
    g_stride = a["g"].shape[1] if "g" in a else 0
    l_stride = a["limg"].shape[1] if "limg" in a else 0
    A = a["rng"].shape[0] if "rng" in a else 0
    _check(probe, cases, a, so_n, g_stride, l_stride, A, per)
    assert l_stride % 4 == 0 and l_stride <= 40 * 1024 and cases <= 8192

    pa, sz = PArgs(), PSizes()
    for i, n in enumerate(_SIZE_ORDER):
        if n in a:
            setattr(pa, n, a[n].ctypes.data)
            sz.v[i] = a[n].nbytes
    pa.so_n, pa.g_stride, pa.l_stride, pa.cases, pa.A, pa.per = max(so_n, 1), g_stride, l_stride, cases, A, per
    if backend == "emu":
        logt, exptab = tables("emu")
        pa.logt, pa.exptab = logt.ctypes.data, exptab.ctypes.data
        rc = getattr(emu_lib(), "sfpe_" + probe)(C.byref(pa))
    else:
        rc = getattr(gpu_lib(), "sfp_" + probe)(C.byref(pa), C.byref(sz))
    assert rc == 0, "%s on %s: launcher returned %d" % (probe, backend, rc)
    return types.SimpleNamespace(**a)


if __name__ == "__main__":
    print(lib())
