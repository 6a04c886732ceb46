"""sf_action_mask_* and sf_policy_act_masked at the C-ABI boundary: the headers declare the entries, the struct and the command
table; a C compiler gives the struct the size and field offsets the ctypes mirror assumes; the built library exports the
symbols; the Python surface has them; SF_ABI_VERSION stays 2; and every refusal that needs no device state (null handles) is
answered with SF_ERR_ARG before any device call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from strikeforce_amd import abi, build, env, policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strikeforce.h")
POLICY_HEADER = os.path.join(ROOT, "include", "strikeforce_policy.h")
SF_ERR_ARG = -1

DECLARATIONS = {
    "sf_action_mask_device": r"sf_env\s*\*\s*env\s*,\s*const\s+sf_action_mask_io\s*\*\s*io",
    "sf_action_mask": r"sf_env\s*\*\s*env\s*,\s*uint32_t\s*\*\s*out_host",
}


def test_header_declares_the_entries_and_keeps_the_version():
    text = open(HEADER).read()
    for name, args in DECLARATIONS.items():
        assert re.search(r"int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), text), name
    assert "#define SF_ABI_VERSION 2" in text  # additive: the version stays
    assert ["sf_" + n for n in abi.ACTION_MASK_EXPORTS] == list(DECLARATIONS)
    assert re.search(r'#define\s+SF_COMMANDS\s+"%s"' % re.escape(abi.ALL_COMMANDS), text)
    assert re.search(r"#define\s+SF_N_COMMANDS\s+30\b", text) and abi.N_COMMANDS == 30 == len(env.COMMANDS)
    assert env.COMMANDS == abi.VALID_COMMANDS + "_"  # gameplay.hpp:45 with '_' appended
    # the caveat of a mask taken at observation time, and what a clear bit of every corner means, are said where the caller reads them
    flat = lambda t: " ".join(t.replace("\n * ", " ").split())  # (comment lines joined)
    for phrase in ("What a set bit is not: a promise", "gameplay.hpp:1455-1464", "never 0", "gets the word 0",
                   "between sf_step_begin and sf_step_end"):
        assert phrase in flat(text), phrase
    ptext = flat(open(POLICY_HEADER).read())
    assert re.search(r"int sf_policy_act_masked\(sf_policy \*p, const float \*d_probs, int32_t agents, const char \*action_string, "
                     r"uint64_t seed, int32_t greedy, const uint32_t \*d_action_mask", ptext)
    for phrase in ("-inf", "bit for bit", "never drawn"):
        assert phrase in ptext, phrase


def test_ctypes_mirror_matches_the_c_compilers_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <string.h>\n#include "strikeforce_policy.h"\n'
                   "int main(void) {\n"
                   "  int (*d)(sf_env *, const sf_action_mask_io *) = sf_action_mask_device;\n"
                   "  int (*h)(sf_env *, uint32_t *) = sf_action_mask;\n"
                   "  int (*m)(sf_policy *, const float *, int32_t, const char *, uint64_t, int32_t, const uint32_t *, uint8_t *,\n"
                   "           int32_t *, float *) = sf_policy_act_masked;\n"
                   "  (void)d, (void)h, (void)m;\n"
                   '  printf("%zu %zu %zu %zu %d %zu", sizeof(sf_action_mask_io), offsetof(sf_action_mask_io, d_commands),\n'
                   "         offsetof(sf_action_mask_io, action_string), offsetof(sf_action_mask_io, d_actions), SF_N_COMMANDS,\n"
                   "         strlen(SF_COMMANDS));\n"
                   "  return 0; }\n")
    obj, stubs, exe = tmp_path / "layout.o", tmp_path / "stubs.c", tmp_path / "layout"
    cc = os.environ.get("CC", "cc")
    subprocess.check_call([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(obj), str(src)])
    stubs.write_text("".join("int %s() { return 0; }\n" % n for n in list(DECLARATIONS) + ["sf_policy_act_masked"]))
    subprocess.check_call([cc, "-o", str(exe), str(obj), str(stubs)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    IO = abi.ActionMaskIO
    assert got == [C.sizeof(IO), IO.d_commands.offset, IO.action_string.offset, IO.d_actions.offset, abi.N_COMMANDS, 30]


def test_library_exports_the_symbols_and_python_binds_them():
    so = build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    L = env.load_library()
    for name in DECLARATIONS:
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in env.EXPORTS
        assert getattr(L, name).restype is C.c_int
    assert re.search(r"\bT sf_policy_act_masked\b", out) and "sf_policy_act_masked" in policy.EXPORTS
    for m in ("action_mask", "action_mask_device", "action_mask_host"):
        assert callable(getattr(env.ArenaBatch, m)), m
    assert callable(policy.PolicyBatch.act_masked)


def test_null_handles_are_refused_before_any_device_call():
    L = env.load_library()
    io = abi.ActionMaskIO(None, b"+xzqeawsd", None)
    assert L.sf_action_mask_device(None, C.byref(io)) == SF_ERR_ARG
    assert b"null" in L.sf_last_error()
    assert L.sf_action_mask(None, None) == SF_ERR_ARG
    L.sf_policy_act_masked.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_char_p, C.c_uint64, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]
    L.sf_policy_act_masked.restype = C.c_int
    assert L.sf_policy_act_masked(None, None, 1, b"+xzqeawsd", 0, 0, None, None, None, None) != 0


def test_decode_action_mask():
    words = np.array([[0, 1], [(1 << 30) - 1, (1 << 9) | (1 << 29)]], dtype=np.uint32)
    m = env.decode_action_mask(words)
    assert m.shape == (2, 2, 30) and m.dtype == bool
    assert not m[0, 0].any() and m[0, 1].tolist() == [True] + [False] * 29 and m[1, 0].all()
    assert [env.COMMANDS[k] for k in np.nonzero(m[1, 1])[0]] == ["s", "_"]
    assert env.decode_action_mask(np.int32(-1 & 0x3FFFFFFF)).shape == (30,)
