"""sf_snapshot_* and sf_policy_memory_rows at the C-ABI boundary: the headers declare the entries with the argument lists the
ctypes mirrors bind, a C compiler accepts the declarations and gives the argument types the sizes the mirrors assume, the
built library exports the symbols, the Python surface has them, and SF_ABI_VERSION stays 2."""
import ctypes as C
import os
import re
import subprocess

from strikeforce_amd import abi, build, env, policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strikeforce.h")
POLICY_HEADER = os.path.join(ROOT, "include", "strikeforce_policy.h")

DECLARATIONS = {
    "sf_snapshot_create": r"sf_env\s*\*\s*env\s*,\s*int32_t\s+slots\s*,\s*sf_snapshot\s*\*\*\s*out",
    "sf_snapshot_destroy": r"sf_snapshot\s*\*\s*s",
    "sf_snapshot_slot_bytes": r"sf_env\s*\*\s*env\s*,\s*int64_t\s*\*\s*device_bytes\s*,\s*int64_t\s*\*\s*blob_bytes",
    "sf_snapshot_save": r"sf_env\s*\*\s*env\s*,\s*sf_snapshot\s*\*\s*s\s*,\s*const\s+int32_t\s*\*\s*d_slot_of_arena",
    "sf_snapshot_load": r"sf_env\s*\*\s*env\s*,\s*sf_snapshot\s*\*\s*s\s*,\s*const\s+int32_t\s*\*\s*d_slot_of_arena",
    "sf_snapshot_status": r"sf_snapshot\s*\*\s*s\s*,\s*int32_t\s+out_host\s*\[\s*4\s*\]",
    "sf_snapshot_export": r"sf_snapshot\s*\*\s*s\s*,\s*int32_t\s+slot\s*,\s*void\s*\*\s*blob_host\s*,\s*int64_t\s+bytes",
    "sf_snapshot_import": r"sf_snapshot\s*\*\s*s\s*,\s*int32_t\s+slot\s*,\s*const\s+void\s*\*\s*blob_host\s*,\s*int64_t\s+bytes",
}


def test_header_declares_the_entries_and_keeps_the_version():
    text = open(HEADER).read()
    assert re.search(r"typedef\s+struct\s+sf_snapshot\s+sf_snapshot\s*;", text)
    for name, args in DECLARATIONS.items():
        assert re.search(r"int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), text), name
    assert "#define SF_ABI_VERSION 2" in text  # additive: the version stays
    assert ["sf_" + n for n in abi.SNAPSHOT_EXPORTS] == list(DECLARATIONS)
    # what a slot does not carry is said where the caller reads it
    for phrase in ("episodes", "result latch", "episode-log ring", "SOURCE's seed sequence", "unique"):
        assert phrase in text, phrase


def test_policy_header_declares_memory_rows():
    text = open(POLICY_HEADER).read()
    assert re.search(r"int\s+sf_policy_memory_rows\s*\(\s*sf_policy\s*\*\s*p\s*,\s*int32_t\s+to_rows\s*,\s*float\s*\*\s*d_h\s*(/\*.*?\*/)?\s*,"
                     r"\s*float\s*\*\s*d_action\s*(/\*.*?\*/)?\s*,\s*const\s+int32_t\s*\*\s*d_row_of_agent\s*,\s*int32_t\s+rows\s*,"
                     r"\s*int32_t\s+agents\s*\)\s*;", text, re.S)


def test_ctypes_mirrors_match_the_c_compilers_sizes(tmp_path):
    """The mirrors pass handles and pointers as c_void_p, counts as c_int32, byte counts as c_int64 and the status words as
    int32[4]: a C program that calls every entry through the header's prototypes compiles, and the sizes agree."""
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "strikeforce.h"\n#include "strikeforce_policy.h"\n'
                   "int main(void) {\n"
                   "  int (*c)(sf_env *, int32_t, sf_snapshot **) = sf_snapshot_create;\n"
                   "  int (*d)(sf_snapshot *) = sf_snapshot_destroy;\n"
                   "  int (*b)(sf_env *, int64_t *, int64_t *) = sf_snapshot_slot_bytes;\n"
                   "  int (*s)(sf_env *, sf_snapshot *, const int32_t *) = sf_snapshot_save;\n"
                   "  int (*l)(sf_env *, sf_snapshot *, const int32_t *) = sf_snapshot_load;\n"
                   "  int (*t)(sf_snapshot *, int32_t *) = sf_snapshot_status;\n"
                   "  int (*e)(sf_snapshot *, int32_t, void *, int64_t) = sf_snapshot_export;\n"
                   "  int (*i)(sf_snapshot *, int32_t, const void *, int64_t) = sf_snapshot_import;\n"
                   "  int (*m)(sf_policy *, int32_t, float *, float *, const int32_t *, int32_t, int32_t) = sf_policy_memory_rows;\n"
                   "  (void)c, (void)d, (void)b, (void)s, (void)l, (void)t, (void)e, (void)i, (void)m;\n"
                   '  printf("%zu %zu %zu %zu %zu", sizeof(sf_snapshot *), sizeof(int32_t), sizeof(int64_t), sizeof(int32_t[4]), sizeof(int));\n'
                   "  return 0; }\n")
    obj = tmp_path / "size.o"
    cc = os.environ.get("CC", "cc")
    subprocess.check_call([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(obj), str(src)])
    # (only sizes are printed: link against stubs of the nine entries)
    stubs = tmp_path / "stubs.c"
    stubs.write_text("".join("int %s() { return 0; }\n" % n for n in list(DECLARATIONS) + ["sf_policy_memory_rows"]))
    exe = tmp_path / "size"
    subprocess.check_call([cc, "-o", str(exe), str(obj), str(stubs)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(C.c_void_p), C.sizeof(C.c_int32), C.sizeof(C.c_int64), C.sizeof(C.c_int32 * abi.SNAPSHOT_STATUS_WORDS),
                   C.sizeof(C.c_int)]


def test_library_exports_the_symbols_and_python_binds_them():
    so = build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    L = env.load_library()
    for name in DECLARATIONS:
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in env.EXPORTS
        assert getattr(L, name).restype is C.c_int
    assert L.sf_snapshot_save.argtypes == [C.c_void_p] * 3 and L.sf_snapshot_export.argtypes[3] is C.c_int64
    for m in ("save", "load", "status", "export", "import_", "close"):
        assert callable(getattr(env.Snapshot, m)), m
    assert callable(env.ArenaBatch.snapshot)
    assert re.search(r"\bT sf_policy_memory_rows\b", out)
    assert "sf_policy_memory_rows" in policy.EXPORTS
    assert callable(policy.PolicyBatch.memory_rows) and callable(policy.RewardBatch.memory_rows)
