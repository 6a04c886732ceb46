"""sf_record_* at the C-ABI boundary: the header declares the entries, the built library exports them, the Python surface
binds them, the SF_RECORD_* values are abi's, and SF_ABI_VERSION stays 2."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from strikeforce_amd import abi, build, env, replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strikeforce.h")

DECLARATIONS = {
    "sf_record_create": r"sf_env\s*\*\s*env\s*,\s*int64_t\s+bytes_per_arena\s*,\s*int32_t\s+games_per_arena\s*,\s*sf_recorder\s*\*\*\s*out",
    "sf_record_destroy": r"sf_recorder\s*\*\s*r",
    "sf_record_step": r"sf_env\s*\*\s*env\s*,\s*sf_recorder\s*\*\s*r\s*,\s*const\s+uint8_t\s*\*\s*d_cmd",
    "sf_record_flush": r"sf_env\s*\*\s*env\s*,\s*sf_recorder\s*\*\s*r",
    "sf_record_collect_device": r"sf_recorder\s*\*\s*r\s*,\s*uint8_t\s*\*\s*d_bytes\s*,\s*int64_t\s+max_bytes\s*,\s*int32_t\s*\*\s*d_games\s*,"
                                r"\s*int32_t\s+max_games\s*,\s*int64_t\s*\*\s*d_counts",
    "sf_record_collect": r"sf_recorder\s*\*\s*r\s*,\s*uint8_t\s*\*\s*bytes_host\s*,\s*int64_t\s+max_bytes\s*,\s*int32_t\s*\*\s*games_host\s*,"
                         r"\s*int32_t\s+max_games\s*,\s*int64_t\s*\*\s*counts_host",
}


def test_header_declares_the_entries_and_keeps_the_version():
    text = open(HEADER).read()
    for name, args in DECLARATIONS.items():
        assert re.search(r"int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), text), name
    assert "#define SF_ABI_VERSION 2" in text  # additive: the version stays
    assert ["sf_" + n for n in abi.RECORD_EXPORTS] == list(DECLARATIONS)
    assert set(DECLARATIONS) <= set(env.EXPORTS)
    assert re.search(r"typedef\s+struct\s+sf_recorder\s+sf_recorder\s*;", text)


def test_the_headers_values_are_abis():
    text = open(HEADER).read()
    enum = re.search(r"enum\s*\{\s*(SF_RECORD_GAME_ENDED[^}]*)\}", text).group(1)
    got = {k: int(v) for k, v in re.findall(r"(SF_RECORD_\w+)\s*=\s*(\d+)", enum)}
    assert got == {"SF_RECORD_GAME_ENDED": abi.RECORD_GAME_ENDED, "SF_RECORD_CUT": abi.RECORD_CUT,
                   "SF_RECORD_OVERFLOW": abi.RECORD_OVERFLOW, "SF_RECORD_BROKEN": abi.RECORD_BROKEN}
    assert len(set(got.values())) == 4 and 0 not in got.values()
    assert int(re.search(r"#define\s+SF_RECORD_GAME_WORDS\s+(\d+)", text).group(1)) == abi.RECORD_GAME_WORDS == 12
    assert int(re.search(r"#define\s+SF_RECORD_COUNT_WORDS\s+(\d+)", text).group(1)) == abi.RECORD_COUNT_WORDS == len(abi.RECORD_COUNT_FIELDS)


def test_a_c_compiler_takes_the_declarations(tmp_path):
    src = tmp_path / "decl.c"
    src.write_text('#include "strikeforce.h"\n'
                   "int main(void) {\n"
                   "  int (*a)(sf_env *, int64_t, int32_t, sf_recorder **) = sf_record_create;\n"
                   "  int (*b)(sf_recorder *) = sf_record_destroy;\n"
                   "  int (*c)(sf_env *, sf_recorder *, const uint8_t *) = sf_record_step;\n"
                   "  int (*d)(sf_env *, sf_recorder *) = sf_record_flush;\n"
                   "  int (*e)(sf_recorder *, uint8_t *, int64_t, int32_t *, int32_t, int64_t *) = sf_record_collect_device;\n"
                   "  int (*f)(sf_recorder *, uint8_t *, int64_t, int32_t *, int32_t, int64_t *) = sf_record_collect;\n"
                   "  return !(a && b && c && d && e && f) + SF_RECORD_BROKEN - 4; }\n")
    stubs, exe = tmp_path / "stubs.c", tmp_path / "decl"
    stubs.write_text("".join("int %s() { return 0; }\n" % n for n in DECLARATIONS))
    cc = os.environ.get("CC", "cc")
    subprocess.check_call([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src), str(stubs)])
    assert subprocess.call([str(exe)]) == 0


def test_library_exports_the_symbols_and_python_binds_them():
    so = build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    L = env.load_library()
    for name in DECLARATIONS:
        assert re.search(r"\bT %s\b" % name, out), name
        assert getattr(L, name).restype is C.c_int
    assert callable(env.ArenaBatch.recorder)
    for m in ("step", "flush", "collect", "collect_device", "close"):
        assert callable(getattr(env.Recorder, m)), m
    assert callable(replay.samples_from_recording)


def test_decode_games_names_the_words():
    g = np.arange(24, dtype=np.int32).reshape(2, 12)
    g[1, 2:6] = [-1, 1, -2, 0]
    g[1, 10:12] = [5, 1]
    d = env.decode_games(g)
    assert d["arena"].tolist() == [0, 12] and d["episode"].tolist() == [1, 13] and d["lines"].tolist() == [6, 18]
    assert d["iterations"].tolist() == [7, 19] and d["end"].tolist() == [8, 20] and d["outcome"].tolist() == [9, 21]
    assert int(d["tb"][1]) == (1 << 32) | 0xFFFFFFFF and int(d["serial"][1]) == 0xFFFFFFFE and int(d["offset"][1]) == (1 << 32) + 5
    assert env.decode_games(np.zeros((0, 12), np.int32))["arena"].shape == (0,)
