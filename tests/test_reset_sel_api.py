"""sf_reset_arenas at the C-ABI boundary: the header declares the entry and its struct, the ctypes mirror has the struct's
fields in the header's order and the size the C compiler gives it, the built library exports the symbol and the Python
surface binds it."""
import ctypes as C
import os
import re
import subprocess

from strikeforce_amd import abi, build, env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strikeforce.h")

FIELDS = ["d_mask", "mask_stride", "done_too", "max_steps", "d_tb", "d_serial", "d_selected"]


def test_header_declares_the_entry_and_the_struct():
    text = open(HEADER).read()
    assert re.search(r"int\s+sf_reset_arenas\s*\(\s*sf_env\s*\*\s*env\s*,\s*const\s+sf_reset_sel\s*\*\s*sel\s*\)\s*;", text)
    m = re.search(r"typedef\s+struct\s+sf_reset_sel\s*\{(.*?)\}\s*sf_reset_sel\s*;", text, re.S)
    assert m, "struct sf_reset_sel is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == FIELDS
    assert "#define SF_ABI_VERSION 2" in text  # additive: the version stays


def test_ctypes_struct_matches_the_header(tmp_path):
    assert [n for n, _ in abi.ResetSel._fields_] == FIELDS
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "strikeforce.h"\n'
                   "int main(void) { printf(\"%zu\", sizeof(sf_reset_sel));\n"
                   + "".join('  printf(" %%zu", offsetof(sf_reset_sel, %s));\n' % f for f in FIELDS)
                   + "  return 0; }\n")
    exe = tmp_path / "size"
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == C.sizeof(abi.ResetSel)
    assert got[1:] == [getattr(abi.ResetSel, f).offset for f in FIELDS]


def test_library_exports_the_symbol_and_python_binds_it():
    so = build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    assert re.search(r"\bT sf_reset_arenas\b", out)
    assert "sf_reset_arenas" in env.EXPORTS
    L = env.load_library()
    assert L.sf_reset_arenas.argtypes[1]._type_ is abi.ResetSel
    assert callable(getattr(env.ArenaBatch, "reset_arenas"))
