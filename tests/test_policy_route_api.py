"""sf_route_* as declared and exported, and the ctypes structs of strikeforce_amd.policy against the header's (field order and
sizes), without a GPU.  The argument checks of sf_route_create stand in front of its first device call, so they run here too."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from strikeforce_amd import build, env, policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "strikeforce_policy.h")).read()

DECLARATIONS = [
    r"int sf_route_create\(const int32_t \*assign, int32_t agents, int32_t nets, int32_t device, sf_route \*\*out\);",
    r"void sf_route_destroy\(sf_route \*r\);",
    r"int sf_route_set_stream\(sf_route \*r, void \*hip_stream\);",
    r"int sf_route_synchronize\(sf_route \*r\);",
    r"int sf_route_count\(sf_route \*r, int32_t net, int32_t \*n\);",
    r"int sf_route_agents_device\(sf_route \*r, int32_t net, const int32_t \*\*d_agent_of_slot\);",
    r"int sf_route_gather\(sf_route \*r, const sf_route_src \*src, const sf_route_dst \*dst\);",
    r"int sf_route_scatter\(sf_route \*r, const sf_route_rows \*rows, const sf_route_rows \*env\);",
]

C_TYPES = {"int32_t": C.c_int32, "uint64_t": C.c_uint64}


def header_fields(struct):
    """[(name, ctypes type)] of `typedef struct NAME { ... } NAME;` in the header: pointers as c_void_p."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        head, names = re.match(r"((?:const )?\w+)\s+(.*)", decl, re.S).groups()
        for n in names.split(","):
            n = n.strip()
            out.append((n.lstrip("*"), C.c_void_p if n.startswith("*") else C_TYPES[head.replace("const ", "")]))
    return out


@pytest.mark.parametrize("decl", DECLARATIONS)
def test_header_declares_the_entry(decl):
    assert re.search(decl, HEADER), decl


def test_abi_version_stays_and_the_limit_is_eight():
    assert "#define SF_POLICY_ABI_VERSION 1\n" in HEADER
    assert "#define SF_ROUTE_MAX_NETS 8\n" in HEADER and policy.ROUTE_MAX_NETS == 8
    # the entries cite the reference lines they stand for
    section = HEADER[HEADER.index("several networks in one match"):]
    for cite in ("Custom.hpp:161-165", "Agent.hpp:84-101", "gameplay.hpp:57-207", "selected_agent.hpp:25"):
        assert cite in section, cite
    assert "(seed, s, i)" in section  # the draw of a routed network is keyed by the slot


@pytest.mark.parametrize("struct,cls", [("sf_route_src", "RouteSrc"), ("sf_route_dst", "RouteDst"), ("sf_route_rows", "RouteRows")])
def test_ctypes_structs_have_the_headers_field_order_and_sizes(struct, cls):
    cls = getattr(policy, cls)
    want = header_fields(struct)
    assert [(n, t) for n, t in cls._fields_] == want, (cls._fields_, want)
    ref = type("Ref", (C.Structure,), {"_fields_": want})
    assert C.sizeof(cls) == C.sizeof(ref)
    for n, _ in want:
        assert getattr(cls, n).offset == getattr(ref, n).offset, n
    # the leading fields are sf_policy_predict_io's: a caller fills both from the same variables
    if struct == "sf_route_src":
        assert [n for n, _ in want] == [n for n, _ in policy.PredictIO._fields_[:len(want)]]


def test_library_exports_every_entry_and_binds_them():
    build.build(verbose=False)
    L = env.load_library()
    policy._bind_route(L)
    for name in policy.ROUTE_EXPORTS:
        assert hasattr(L, name), name
        assert getattr(L, name).restype is (None if name == "sf_route_destroy" else C.c_int)
    assert sorted(policy.ROUTE_EXPORTS) == sorted(set(re.findall(r"\b(sf_route_[a-z_]+)\(", HEADER)))
    for method in ("gather", "inputs", "outputs", "scatter", "count", "agents_of", "set_stream", "close"):
        assert callable(getattr(policy.Router, method)), method


def test_a_library_without_the_entries_is_a_clear_error():
    class Old:
        pass
    with pytest.raises(env.StrikeForceError, match="no sf_route_\\* entry points"):
        policy._bind_route(Old())


def test_create_refuses_bad_arguments_before_any_device_call():
    build.build(verbose=False)
    L = env.load_library()
    policy._bind_route(L)
    out = C.c_void_p()
    i32p = C.POINTER(C.c_int32)

    def create(assign, nets, agents=None):
        a = np.asarray(assign, dtype=np.int32)
        return L.sf_route_create(a.ctypes.data_as(i32p), len(a) if agents is None else agents, nets, 0, C.byref(out))

    for assign, nets, agents, text in [([0, 1], 0, None, b"nets must be"), ([0, 1], 9, None, b"nets must be"),
                                       ([0, 2], 2, None, b"assign[1]"), ([0, -2], 2, None, b"assign[1]"),
                                       ([0], 1, 0, b"agents must be")]:
        assert create(assign, nets, agents) == -1 and text in L.sf_last_error(), (assign, nets, L.sf_last_error())
    assert L.sf_route_create(None, 1, 1, 0, C.byref(out)) == -1
    assert L.sf_route_count(None, 0, C.byref(C.c_int32())) == -1 and b"null route" in L.sf_last_error()
    assert L.sf_route_gather(None, None, None) == -1 and L.sf_route_scatter(None, None, None) == -1
