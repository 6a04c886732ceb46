"""The lane functions of csrc/sf_state_records.hpp — the text k_state_records compiles — on the CPU, in the stand-alone program
tests/state_records/state_main.cpp, built once plain and once with -fsanitize=address,undefined.  Nothing sanitized is loaded
into Python.

The states are the cases' oracle dumps packed by state_records_ref.encode() (the inverse of the library's decode()), with
garbage wherever the decoder must not look, plus a synthetic state of edge values: coordinates 1023 and floor 3, negative hp
and effect, traveled and range 65535, backpack.ind 14, portal_ind 254, item counts 65535, every HF_* bit.  The program writes
the full request's outputs, which must be the records the state was packed from, their counts and the restated digest (which
tests/test_state_records_cases.py holds to the oracle's); the program itself compares every subset of outputs, cut and id list
with slices of that (see its header)."""
import os
import subprocess

import numpy as np
import pytest

import state_records_cases as sc
import state_records_ref as ref
from strikeforce_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "state_records", "state_main.cpp")
BASE = ["-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
HF_CTRL, HF_OCC, HF_AGP = 1 << 15, 1 << 22, 15 << 23  # the bits of HW_FLAGS no record shows (csrc/sf_types.hpp)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("state_main")
    out = {}
    for name, flags in BUILDS.items():
        out[name] = str(d / ("state_main_" + name))
        subprocess.check_call([os.environ.get("CXX", "g++")] + BASE + flags + ["-o", out[name], SRC])
    return out


def write_state(path, arrs, map_pidx, cells_pad, extra=0):
    """The packed state of the arenas `arrs` ([arena] -> arena_arrays()) in state_main's layout."""
    enc = [ref.encode(a, map_pidx, extra) for a in arrs]
    A = len(arrs)
    H, Z, B, P = (len(arrs[0][t]) for t in ref.TABLES)
    cells = len(arrs[0]["cell_flags"])
    soa = lambda key: np.stack([e[key] for e in enc], axis=1)  # [field][arena][slot]
    flags = np.full((A, cells_pad), 0xEE, dtype=np.uint8)  # (the pad behind an arena's cells is never read)
    for a, e in enumerate(enc):
        flags[a, :cells] = e["flags"]
    parts = [np.array([A, H, Z, B, P, cells, cells_pad], dtype=np.int32), soa("hum"), soa("zom"), soa("bul"),
             np.stack([e["por"] for e in enc]), np.stack([e["rng"] for e in enc]), np.stack([e["scal"] for e in enc]), flags,
             np.stack([e["aux_dmg"] for e in enc]), np.stack([e["aux_pidx"] for e in enc]), np.asarray(map_pidx, dtype=np.int16)]
    with open(path, "wb") as f:
        for p in parts:
            f.write(np.ascontiguousarray(p).tobytes())


def read_outputs(path, arrs):
    A = len(arrs)
    raw = np.fromfile(path, dtype=np.uint8)
    out, at = {}, 0
    for n in ref.OUTPUTS:
        if n == "digest":
            shape, dt = (A,), np.uint64
        else:
            shape, dt = (A,) + arrs[0][n].shape, arrs[0][n].dtype
        nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[n] = raw[at:at + nbytes].view(dt).reshape(shape)
        at += nbytes
    assert at == len(raw)
    return out


def check(programs, tmp_path, arrs, map_pidx, cells_pad, extra=0, requests=None):
    state = str(tmp_path / "state.bin")
    write_state(state, arrs, map_pidx, cells_pad, extra)
    want = ref.expected(arrs, range(len(arrs)), tuple(len(arrs[0][t]) for t in ref.TABLES),
                        np.array([ref.digest_of(a) for a in arrs], dtype=np.uint64))
    for build, exe in programs.items():
        got_file = str(tmp_path / ("out_" + build + ".bin"))
        r = subprocess.run([exe, state, got_file], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (build, r.stdout[-2000:], r.stderr[-4000:])
        last = r.stdout.strip().split("\n")[-1].split()
        assert last[:2] == ["state_main", "ok"], (build, r.stdout[-2000:])
        if requests is not None:
            assert int(last[2]) == requests, (build, last)
        got = read_outputs(got_file, arrs)
        for n in ref.OUTPUTS:
            assert np.array_equal(got[n], want[n]), (build, n, np.argwhere(got[n] != want[n])[:4].tolist())


def cells_pad_of(cells):
    return (cells + 63) // 64 * 64


@pytest.mark.parametrize("name", ["tiny", "battle", "large", "swarm"])
def test_cases_states_through_the_lane_functions(programs, tmp_path, name):
    dumps, digests = sc.oracle_dumps(name)
    arrs = [ref.arena_arrays(d) for d in dumps]
    w = sc.case(name).w
    map_pidx = [int(w.cfg.map_portal[i]) for i in range(w.cells)]
    # every subset x 4 cuts x 3 id lists, the full request four times — or, above 512 cells, 12 requests per cut and list
    small = w.cells <= 512
    check(programs, tmp_path, arrs, map_pidx, cells_pad_of(w.cells) + 64, HF_CTRL | HF_OCC, requests=4 + 12 * (1024 if small else 12))
    assert [ref.digest_of(a) for a in arrs] == [int(x) for x in digests]


def synthetic_arena(rng, H, Z, B, P, cells, map_pidx, first):
    i32 = lambda: int(rng.randint(-2**31, 2**31, dtype=np.int64))
    hum = np.zeros((H, 28), dtype=np.int32)
    for i in range(H):
        if i % 5 == 4:
            continue  # a slot never used
        f, r, c = (3, 1023, 5) if i == 0 else (0, 7, 1023) if i == 1 else (rng.randint(4), rng.randint(1024), rng.randint(1023))
        hum[i] = [rng.randint(2), rng.randint(2), rng.randint(2), rng.randint(2), f, r, c, 1 + rng.randint(4), rng.randint(256),
                  i32(), i32(), i32(), i32(), i32(), i32(), rng.randint(-1, 3), rng.randint(-1, 15)] + \
                 [rng.randint(65536) for _ in range(8)] + [rng.randint(256), rng.randint(256), rng.randint(-1, 255)]
    if first:  # the edges, by name: hp and effect negative, backpack.ind 14, counts 65535, blocks / portals 255, portal_ind 254
        hum[0, 0:4] = 1
        hum[0, 8:17] = [255, -1, -2**31, 2**31 - 1, 2**31 - 1, -5, -2**31, 2, 14]
        hum[0, 17:25] = 65535
        hum[0, 25:28] = [255, 255, 254]
        hum[1, 0] = 0  # dead, with everything else still there
        hum[1, 15:17] = [-1, -1]
        hum[1, 27] = -1
    zom = np.zeros((Z, 7), dtype=np.int32)
    for i in range(Z):
        if rng.randint(3):
            zom[i] = [1, rng.randint(4), rng.randint(1024), rng.randint(1024), i32(), i32(), rng.randint(2)]
    if first:
        zom[Z - 1] = [1, 3, 1023, 1023, -1, -2**31, 1]  # (a zombie's position has no "none" value: all ones are coordinates)
    bul = np.zeros((B, 11), dtype=np.int32)
    for i in range(B):
        if rng.randint(2):
            bul[i] = [1, rng.randint(4), rng.randint(1024), rng.randint(1024), 1 + rng.randint(4), rng.randint(65536), i32(),
                      rng.randint(-32768, 32768), rng.randint(65536), rng.randint(65536), rng.randint(2)]
    if first:
        bul[0] = [1, 3, 1023, 1023, 4, 65535, -2**31, -32768, 65535, 65535, 0]
        bul[B - 1] = [1, 0, 0, 0, 1, 0, 2**31 - 1, 32767, 0, 0, 1]
    por = np.zeros((P, 4), dtype=np.int32)
    for i in range(P):
        if i % 3 != 1:
            por[i] = [1, rng.randint(4), rng.randint(1024), rng.randint(1024)]
    flags = rng.randint(0, 256, size=cells).astype(np.uint8)
    flags[:8] = [0, 0xFF, abi.CELL_TEMP, abi.CELL_PIN_UP, abi.CELL_PIN_DN | abi.CELL_TEMP, abi.CELL_PIN_UP | abi.CELL_PIN_DN, 1, 0xC0 | abi.CELL_CHEST]
    temp, pin = (flags & abi.CELL_TEMP) != 0, (flags & (abi.CELL_PIN_UP | abi.CELL_PIN_DN)) != 0
    dmg = np.where(temp, rng.randint(-2**31, 2**31, size=cells, dtype=np.int64), 0).astype(np.int32)
    pidx = np.where(pin, np.where(temp, rng.randint(-32768, 32768, size=cells), map_pidx), -1).astype(np.int32)
    hdr = np.zeros(40, dtype=np.int32)
    h64 = hdr[:20].view(np.int64)
    h64[:] = [i32(), i32(), i32(), -1, -2**31, rng.randint(0, 2**32, dtype=np.int64), i32() << 32 | 0xFFFFFFFF, -1 if first else i32() << 31,
              2**31 - 1, i32()]
    hdr[20:38] = rng.randint(0, 1 << 20, size=18)
    hdr[20], hdr[37] = 0xFFFFF, 0
    hdr[38], hdr[39] = 1, abi.SAMPLE_END
    arr = {"hdr": hdr, "humans": hum, "zombies": zom, "bullets": bul, "portals": por, "cell_flags": flags, "cell_dmg": dmg,
           "cell_portal": pidx}
    arr["counts"] = ref.counts_of(arr)
    return arr


@pytest.mark.parametrize("H,Z,B,P,cells", [(3, 5, 70, 9, 37), (22, 130, 64, 65, 257)])
def test_synthetic_edge_values(programs, tmp_path, H, Z, B, P, cells):
    rng = np.random.RandomState(1000 * H + cells)
    map_pidx = rng.randint(0, P, size=cells).astype(np.int16)
    arrs = [synthetic_arena(rng, H, Z, B, P, cells, map_pidx, a == 0) for a in range(3)]
    arrs[2]["zombies"][:] = 0  # an arena without a zombie: count and extent 0
    arrs[2]["counts"] = ref.counts_of(arrs[2])
    assert arrs[2]["counts"][1] == 0 and arrs[2]["counts"][5] == 0
    check(programs, tmp_path, arrs, map_pidx, cells + 11, HF_CTRL | HF_OCC | HF_AGP, requests=4 + 12 * 1024)
