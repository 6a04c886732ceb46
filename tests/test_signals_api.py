"""sf_signals_* at the C-ABI boundary: the header declares the entries and the two structs, a C compiler gives the structs the
sizes and field offsets and the constants the values the ctypes mirrors assume, the built library exports the symbols, the
Python surface has them, and SF_ABI_VERSION stays 2."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from strikeforce_amd import abi, build, env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strikeforce.h")

DECLARATIONS = {
    "sf_signals_create": r"sf_env\s*\*\s*env\s*,\s*sf_signals\s*\*\*\s*out",
    "sf_signals_destroy": r"sf_signals\s*\*\s*s",
    "sf_signals_step": r"sf_env\s*\*\s*env\s*,\s*sf_signals\s*\*\s*s\s*,\s*const\s+sf_signals_io\s*\*\s*io",
    "sf_signals_status": r"sf_signals\s*\*\s*s\s*,\s*int64_t\s+out_host\s*\[\s*4\s*\]",
}


def test_header_declares_the_entries_and_keeps_the_version():
    text = open(HEADER).read()
    assert re.search(r"typedef\s+struct\s+sf_signals\s+sf_signals\s*;", text)
    for name, args in DECLARATIONS.items():
        assert re.search(r"int\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), text), name
    assert "#define SF_ABI_VERSION 2" in text  # additive: the version stays
    assert ["sf_" + n for n in abi.SIGNALS_EXPORTS] == list(DECLARATIONS)
    # what the detection cannot see, and whose words the last step of a game holds, are said where the caller reads them
    for phrase in ("cannot see", "whatever stands in its slot", "d_rebase is authoritative", "gameplay.hpp:461", "Character.hpp:294"):
        assert phrase in text, phrase


def test_ctypes_mirrors_match_the_c_compilers_layout(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "strikeforce.h"\n'
                   "int main(void) {\n"
                   "  int (*c)(sf_env *, sf_signals **) = sf_signals_create;\n"
                   "  int (*d)(sf_signals *) = sf_signals_destroy;\n"
                   "  int (*s)(sf_env *, sf_signals *, const sf_signals_io *) = sf_signals_step;\n"
                   "  int (*t)(sf_signals *, int64_t *) = sf_signals_status;\n"
                   "  (void)c, (void)d, (void)s, (void)t;\n"
                   '  printf("%zu %zu %zu %zu %zu %zu ", sizeof(sf_reward_weights), offsetof(sf_reward_weights, w), offsetof(sf_reward_weights, died),\n'
                   "         offsetof(sf_reward_weights, outcome), sizeof(sf_signals_io), offsetof(sf_signals_io, weights));\n"
                   '  printf("%zu %zu %zu %zu ", offsetof(sf_signals_io, d_vitals), offsetof(sf_signals_io, d_delta), offsetof(sf_signals_io, d_reward),\n'
                   "         offsetof(sf_signals_io, d_rebase));\n"
                   '  printf("%d %d %d %d %d %d %d %d", SF_VITALS_WORDS, SF_DELTA_WORDS, SF_SIG_PRESENT, SF_SIG_DIED, SF_SIG_ENDED, SF_SIG_REBASED,\n'
                   "         SF_SIG_UNRESOLVED, SF_SIG_IDLE);\n"
                   "  return 0; }\n")
    obj, stubs, exe = tmp_path / "layout.o", tmp_path / "stubs.c", tmp_path / "layout"
    cc = os.environ.get("CC", "cc")
    subprocess.check_call([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(obj), str(src)])
    stubs.write_text("".join("int %s() { return 0; }\n" % n for n in DECLARATIONS))
    subprocess.check_call([cc, "-o", str(exe), str(obj), str(stubs)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    W, IO = abi.RewardWeights, abi.SignalsIO
    assert got == [C.sizeof(W), W.w.offset, W.died.offset, W.outcome.offset, C.sizeof(IO), IO.weights.offset,
                   IO.d_vitals.offset, IO.d_delta.offset, IO.d_reward.offset, IO.d_rebase.offset,
                   abi.VITALS_WORDS, abi.DELTA_WORDS, abi.SIG_PRESENT, abi.SIG_DIED, abi.SIG_ENDED, abi.SIG_REBASED,
                   abi.SIG_UNRESOLVED, abi.SIG_IDLE]
    assert len(abi.VITALS_FIELDS) == abi.VITALS_WORDS and len(abi.DELTA_FIELDS) == abi.DELTA_WORDS


def test_library_exports_the_symbols_and_python_binds_them():
    so = build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    L = env.load_library()
    for name in DECLARATIONS:
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in env.EXPORTS
        assert getattr(L, name).restype is C.c_int
    for m in ("step", "status", "close"):
        assert callable(getattr(env.Signals, m)), m
    assert callable(env.ArenaBatch.signals)
    assert (env.SIG_PRESENT, env.SIG_DIED, env.SIG_ENDED, env.SIG_REBASED, env.SIG_UNRESOLVED, env.SIG_IDLE) == (1, 2, 4, 8, 16, 32)


def test_decode_signals_and_reward_weights():
    v = np.arange(2 * 3 * 16, dtype=np.int32).reshape(2, 3, 16)
    d = np.zeros((2, 3, 8), dtype=np.int32)
    d[0, 1] = [env.SIG_DIED | env.SIG_UNRESOLVED, 0, 1, 100, 0, 0, -1000, 0]
    d[1, 2] = [env.SIG_ENDED | env.SIG_PRESENT, 2, 0, 0, 300, -5, 0, 2]
    x = env.decode_signals(v, d)
    assert x["hp"][1, 0] == v[1, 0, 1] and x["steps"][0, 2] == v[0, 2, 15] and x["team"].shape == (2, 3)
    assert x["d_hp"][0, 1] == -1000 and x["d_loot"][0, 1] == 100 and x["outcome"][1, 2] == 2 and x["d_damage"][1, 2] == 300
    only = env.decode_signals(delta=d)
    assert only["died"].tolist() == [[False, True, False], [False] * 3] and only["unresolved"][0, 1] and only["ended"][1, 2]
    assert only["present"][1, 2] and not only["rebased"].any() and not only["idle"].any() and "hp" not in only
    w = env.reward_weights(per_step=-0.5, kills=1, teams_kills=2, loot=3, damage=4, effect=5, hp=6, died=-7, outcome={2: 9.0, 7: 1.0})
    assert (w.per_step, list(w.w), w.died, list(w.outcome)) == (-0.5, [1, 2, 3, 4, 5, 6], -7, [0, 0, 9, 0, 0, 0, 0, 1])
    assert list(env.reward_weights(outcome=[0, 1, 2]).outcome) == [0, 1, 2, 0, 0, 0, 0, 0]
