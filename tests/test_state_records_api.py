"""sf_state_device / sf_state_bytes at the C-ABI boundary: the header declares the entries and the struct, a C compiler gives
the struct the size and field offsets the ctypes mirror assumes, the built library exports the symbols, the Python surface
has them, and SF_ABI_VERSION stays 2."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from strikeforce_amd import abi, build, env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strikeforce.h")

DECLARATIONS = {
    "sf_state_device": r"sf_env\s*\*\s*env\s*,\s*const\s+sf_state_io\s*\*\s*io",
    "sf_state_bytes": r"sf_env\s*\*\s*env\s*,\s*const\s+sf_state_io\s*\*\s*io\s*,\s*int64_t\s+bytes_out\s*\[\s*10\s*\]",
}
FIELDS = ["d_arena_ids", "rows", "humans", "zombies", "bullets", "portals"] + list(abi.STATE_OUTPUTS)


def test_header_declares_the_entries_and_keeps_the_version():
    text = open(HEADER).read()
    for name, args in DECLARATIONS.items():
        assert re.search(r"int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), text), name
    assert "#define SF_ABI_VERSION 2" in text  # additive: the version stays
    assert ["sf_" + n for n in abi.STATE_EXPORTS] == list(DECLARATIONS)
    assert set(DECLARATIONS) <= set(env.EXPORTS)
    body = re.search(r"typedef\s+struct\s+sf_state_io\s*\{(.*?)\}\s*sf_state_io\s*;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"[*\s,](\w+)\s*(?=,|$)", decl.strip())]
    assert names == FIELDS and [n for n, _ in abi.StateIO._fields_] == FIELDS, names
    # the contract is said where the caller reads it (comment lines joined)
    text = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("never becomes an address", "whatever the cuts", "bit for bit", "between sf_step_begin and sf_step_end",
                   "gameplay.hpp:461", "Character.hpp:65", "nothing is launched then"):
        assert phrase in text, phrase


def test_ctypes_mirror_matches_the_c_compilers_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "strikeforce.h"\n'
                   "int main(void) {\n"
                   "  int (*d)(sf_env *, const sf_state_io *) = sf_state_device;\n"
                   "  int (*b)(sf_env *, const sf_state_io *, int64_t *) = sf_state_bytes;\n"
                   "  (void)d, (void)b;\n"
                   '  printf("%zu %d", sizeof(sf_state_io), SF_STATE_COUNT_WORDS);\n'
                   + "".join('  printf(" %%zu", offsetof(sf_state_io, %s));\n' % f for f in FIELDS) +
                   '  printf(" %zu %zu %zu %zu %zu", sizeof(sf_arena_hdr), sizeof(sf_human_rec), sizeof(sf_zombie_rec), sizeof(sf_bullet_rec),\n'
                   "         sizeof(sf_portal_rec));\n"
                   "  return 0; }\n")
    obj, stubs, exe = tmp_path / "layout.o", tmp_path / "stubs.c", tmp_path / "layout"
    cc = os.environ.get("CC", "cc")
    subprocess.check_call([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(obj), str(src)])
    stubs.write_text("".join("int %s() { return 0; }\n" % n for n in DECLARATIONS))
    subprocess.check_call([cc, "-o", str(exe), str(obj), str(stubs)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    IO = abi.StateIO
    assert got == [C.sizeof(IO), abi.STATE_COUNT_WORDS] + [getattr(IO, f).offset for f in FIELDS] + [
        C.sizeof(s) for s in (abi.ArenaHdr, abi.HumanRec, abi.ZombieRec, abi.BulletRec, abi.PortalRec)]
    assert len(abi.STATE_COUNT_FIELDS) == abi.STATE_COUNT_WORDS and len(abi.STATE_OUTPUTS) == 10


def test_library_exports_the_symbols_and_python_binds_them():
    so = build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    L = env.load_library()
    for name in DECLARATIONS:
        assert re.search(r"\bT %s\b" % name, out), name
        assert getattr(L, name).restype is C.c_int
    for m in ("state_records", "state_io", "digest_device", "state_device", "state_bytes"):
        assert callable(getattr(env.ArenaBatch, m)), m


def test_decode_state_names_the_words_of_every_record():
    h = np.arange(2 * 3 * 28, dtype=np.int32).reshape(2, 3, 28)
    z = np.arange(2 * 5 * 7, dtype=np.int32).reshape(2, 5, 7)
    b = np.arange(2 * 11, dtype=np.int32).reshape(2, 1, 11)
    p = np.arange(2 * 4 * 4, dtype=np.int32).reshape(2, 4, 4)
    hdr = np.arange(2 * 40, dtype=np.int32).reshape(2, 40)
    cnt = np.arange(16, dtype=np.int32).reshape(2, 8)
    x = env.decode_state(hdr, h, z, b, p, cnt)
    assert x["humans"]["alive"][1, 2] == h[1, 2, 0] and x["humans"]["hp"][0, 1] == h[0, 1, 9] and x["humans"]["portal_ind"][1, 0] == h[1, 0, 27]
    assert x["humans"]["cons"].shape == (2, 3, 4) and x["humans"]["throw_cnt"][1, 1].tolist() == h[1, 1, 21:25].tolist()
    assert x["zombies"]["super_"][1, 4] == z[1, 4, 6] and x["bullets"]["ref"][1, 0] == b[1, 0, 10] and x["portals"]["c"][0, 3] == p[0, 3, 3]
    assert x["hdr"]["steps"][1] == hdr[1, 16:18].view(np.int64)[0] and x["hdr"]["rng"].shape == (2, 18) and x["hdr"]["outcome"][1] == hdr[1, 39]
    assert x["hdr"]["tb"].dtype == np.int64 and x["counts"]["zombies_extent"].tolist() == [5, 13]
    x["humans"]["hp"][0, 0] = -5  # views, not copies
    assert h[0, 0, 9] == -5
    # the named words are the C structs' fields, in order
    for struct in (abi.HumanRec, abi.ZombieRec, abi.BulletRec, abi.PortalRec):
        words = [w for _, w, _ in abi.record_fields(struct)]
        assert words == sorted(words) and words[0] == 0 and sum(k for _, _, k in abi.record_fields(struct)) * 4 == C.sizeof(struct)
