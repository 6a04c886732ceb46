"""sf_state_put_device / sf_state_put_status / sf_load_arena at the C-ABI boundary: the header declares the entries and the
struct, a C compiler gives the struct the size and field offsets the ctypes mirror assumes, the built library exports the
symbols, the Python surface has them, SF_ABI_VERSION stays 2, env.encode_state inverts env.decode_state, and a runtime
without the launches (the wave emulator's) answers SF_ERR_STATE."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from strikeforce_amd import abi, build, env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strikeforce.h")

DECLARATIONS = {
    "sf_state_put_device": r"sf_env\s*\*\s*env\s*,\s*const\s+sf_state_put_io\s*\*\s*io",
    "sf_state_put_status": r"sf_env\s*\*\s*env\s*,\s*int64_t\s+out_host\s*\[\s*4\s*\]",
    "sf_load_arena": r"sf_env\s*\*\s*env\s*,\s*int32_t\s+arena\s*,\s*const\s+sf_arena_hdr\s*\*\s*hdr\s*,\s*const\s+sf_human_rec\s*\*\s*humans\s*,"
                     r"\s*const\s+sf_zombie_rec\s*\*\s*zombies\s*,\s*const\s+sf_bullet_rec\s*\*\s*bullets\s*,\s*const\s+sf_portal_rec\s*\*\s*portals\s*,"
                     r"\s*const\s+uint8_t\s*\*\s*cell_flags\s*,\s*const\s+int32_t\s*\*\s*cell_dmg\s*,\s*const\s+int32_t\s*\*\s*cell_portal",
}
FIELDS = ["d_row_of_arena", "rows", "humans", "zombies", "bullets", "portals"] + list(abi.STATE_PUT_PARTS) + ["d_status", "d_selected"]


def test_header_declares_the_entries_and_keeps_the_version():
    text = open(HEADER).read()
    for name, args in DECLARATIONS.items():
        assert re.search(r"int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), text), name
    assert "#define SF_ABI_VERSION 2" in text  # additive: the version stays
    assert ["sf_" + n for n in abi.STATE_PUT_EXPORTS] == list(DECLARATIONS)
    assert set(DECLARATIONS) <= set(env.EXPORTS)
    body = re.search(r"typedef\s+struct\s+sf_state_put_io\s*\{(.*?)\}\s*sf_state_put_io\s*;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"[*\s,](\w+)\s*(?=,|$)", decl.strip())]
    assert names == FIELDS and [n for n, _ in abi.StatePutIO._fields_] == FIELDS, names
    bits = dict(re.findall(r"(SF_PUT_BAD_\w+)\s*=\s*(\d+)", text))
    assert {k: int(v) for k, v in bits.items()} == {"SF_PUT_BAD_HDR": abi.PUT_BAD_HDR, "SF_PUT_BAD_HUMAN": abi.PUT_BAD_HUMAN,
                                                    "SF_PUT_BAD_ZOMBIE": abi.PUT_BAD_ZOMBIE, "SF_PUT_BAD_BULLET": abi.PUT_BAD_BULLET,
                                                    "SF_PUT_BAD_PORTAL": abi.PUT_BAD_PORTAL, "SF_PUT_BAD_CELL": abi.PUT_BAD_CELL,
                                                    "SF_PUT_BAD_ROW": abi.PUT_BAD_ROW}
    # the contract is said where the caller reads it (comment lines joined)
    text = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("The core property", "What the destination keeps", "before any word of any arena is written", "never becomes an address",
                   "a dead `ind` keeps its cell and its command", "hdr.tb + reseed_stride", "jomle - 1042", "memory safety and determinism",
                   "may be captured in a graph", "neither needed a change", "on a runtime without the launches"):
        assert phrase in text, phrase


def test_ctypes_mirror_matches_the_c_compilers_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "strikeforce.h"\n'
                   "int main(void) {\n"
                   "  int (*d)(sf_env *, const sf_state_put_io *) = sf_state_put_device;\n"
                   "  int (*s)(sf_env *, int64_t *) = sf_state_put_status;\n"
                   "  (void)d, (void)s;\n"
                   '  printf("%zu", sizeof(sf_state_put_io));\n'
                   + "".join('  printf(" %%zu", offsetof(sf_state_put_io, %s));\n' % f for f in FIELDS) +
                   "  return 0; }\n")
    obj, stubs, exe = tmp_path / "layout.o", tmp_path / "stubs.c", tmp_path / "layout"
    cc = os.environ.get("CC", "cc")
    subprocess.check_call([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(obj), str(src)])
    stubs.write_text("".join("int %s() { return 0; }\n" % n for n in DECLARATIONS))
    subprocess.check_call([cc, "-o", str(exe), str(obj), str(stubs)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    IO = abi.StatePutIO
    assert got == [C.sizeof(IO)] + [getattr(IO, f).offset for f in FIELDS]


def test_library_exports_the_symbols_and_python_binds_them():
    so = build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    L = env.load_library()
    for name in DECLARATIONS:
        assert re.search(r"\bT %s\b" % name, out), name
        assert getattr(L, name).restype is C.c_int
    for m in ("put_state", "state_put_io", "state_put_device", "put_status", "load_arena"):
        assert callable(getattr(env.ArenaBatch, m)), m


def test_encode_state_inverts_decode_state():
    rng = np.random.RandomState(5)
    h = rng.randint(-2**31, 2**31, size=(2, 3, 28), dtype=np.int64).astype(np.int32)
    z = rng.randint(-2**31, 2**31, size=(2, 5, 7), dtype=np.int64).astype(np.int32)
    b = rng.randint(-2**31, 2**31, size=(2, 1, 11), dtype=np.int64).astype(np.int32)
    p = rng.randint(-2**31, 2**31, size=(2, 4, 4), dtype=np.int64).astype(np.int32)
    hdr = rng.randint(-2**31, 2**31, size=(2, 40), dtype=np.int64).astype(np.int32)
    x = env.decode_state(hdr, h, z, b, p)
    y = env.encode_state(**x)
    for name, want in (("hdr", hdr), ("humans", h), ("zombies", z), ("bullets", b), ("portals", p)):
        assert y[name].dtype == np.int32 and np.array_equal(y[name], want), name
    # and the other way round, from plain lists
    one = env.encode_state(zombies={"alive": [[1]], "f": [[0]], "r": [[3]], "c": [[4]], "hp": [[-5]], "mindamage": [[7]], "super_": [[1]]})
    assert one["zombies"].tolist() == [[[1, 0, 3, 4, -5, 7, 1]]]
    assert env.decode_state(zombies=one["zombies"])["zombies"]["hp"].tolist() == [[-5]]


def test_a_runtime_without_the_launches_answers_err_state(tmp_path):
    """tests/state_put/emu_state.cpp: the wave emulator's runtime as it is, has_state_put false, SF_ERR_STATE from both."""
    exe = str(tmp_path / "emu_state")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O0", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", exe,
                           os.path.join(ROOT, "tests", "state_put", "emu_state.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("emu_state ok"), (r.stdout[-1000:], r.stderr[-1000:])
