"""The lane functions of csrc/sf_state_put.hpp — the text k_put_check / k_put_write compile — on the CPU, in the
stand-alone program tests/state_put/put_main.cpp, built once plain and once with -fsanitize=address,undefined.  Nothing
sanitized is loaded into Python.

Inputs: the six cases' oracle dumps, and synthetic rows of edge values (coordinates at the map's last cell, the top floor,
negative hp and effect, counts of 65535, backpack.ind 14, portal_ind cap - 1, a dead `ind`, a slot never used).  The program
itself runs the matrix (every subset of the parts x four cuts x 1 / 3 / 64 wavefronts per row, exact-size heap buffers, LDS
refilled with garbage between units), decodes every result with the decoders of csrc/sf_state_records.hpp and compares it with
its input, and holds every check predicate at its last good and first bad value.  Here: the packed words of the full put
equal state_records_ref.encode() on every bit the decoder reads and the stated rule on every bit it does not."""
import os
import subprocess

import numpy as np
import pytest

import state_records_cases as sc
import state_records_ref as ref
from strikeforce_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "state_put", "put_main.cpp")
BASE = ["-std=c++17", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}
HF_ALIVE, HF_CTRL, HF_OCC, HF_AGP_SH = 1 << 11, 1 << 15, 1 << 22, 23
PATTERN = 0x5B5B5B5B


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("put_main")
    out = {}
    for name, flags in BUILDS.items():
        out[name] = str(d / ("put_main_" + name))
        subprocess.check_call([os.environ.get("CXX", "g++")] + BASE + flags + ["-o", out[name], SRC])
    return out


def write_rows(path, arrs, shape, map_pidx, cells_pad):
    """shape: dict F N M mode n_agents ind npc_block auto_reset reseed"""
    A = len(arrs)
    H, Z, B, P = (len(arrs[0][t]) for t in ref.TABLES)
    cells = len(arrs[0]["cell_flags"])
    head = np.array([A, H, Z, B, P, cells, cells_pad, shape["F"], shape["N"], shape["M"], shape["mode"], shape["n_agents"], shape["ind"],
                     shape["npc_block"], shape["auto_reset"], shape["reseed"]], dtype=np.int32)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        for n in ("hdr",) + ref.TABLES + ("cell_flags", "cell_dmg", "cell_portal"):
            f.write(np.ascontiguousarray(np.stack([a[n] for a in arrs])).tobytes())
        f.write(np.asarray(map_pidx, dtype=np.int16).tobytes())


def read_state(path, A, H, Z, B, P, cells, cells_pad):
    raw = np.fromfile(path, dtype=np.uint8)
    out, at = {}, 0
    for n, shape, dt in (("hum", (13, A, H), np.uint32), ("zom", (3, A, Z), np.uint32), ("bul", (4, A, B), np.uint32),
                         ("por", (A, P), np.uint32), ("rng", (A, 18), np.uint32), ("rng2", (A, 18), np.uint32), ("scal", (A, 24), np.int32),
                         ("flags", (A, cells_pad), np.uint8), ("aux_dmg", (A, cells), np.int32), ("aux_pidx", (A, cells), np.int16)):
        nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[n] = raw[at:at + nbytes].view(dt).reshape(shape)
        at += nbytes
    assert at == len(raw)
    return out


def hidden_bits(shape, slot, h):
    """The rule for the bits of HW_FLAGS no record shows (DESIGN.md §4 "State put")."""
    alive, rnpc, profile, way = int(h[0]), int(h[2]), int(h[3]), int(h[7])
    if way == 0:
        return 0
    keep = alive or slot == shape["ind"]
    if shape["mode"] == abi.MODE_BATTLE:
        seat = slot < shape["n_agents"]
    elif shape["mode"] == abi.MODE_SQUAD:
        seat = slot == 0 or (slot < shape["n_agents"] and slot < 10)
    else:
        seat = slot == 0
    fl = (HF_OCC if keep else 0) | (HF_CTRL if keep and seat and not rnpc else 0)
    if not profile and shape["mode"] == abi.MODE_BATTLE and shape["npc_block"] > 1 and slot < shape["n_agents"]:
        fl |= slot << HF_AGP_SH
    return fl


def digits(x, n=18):
    return [(x // 10 ** i) % 10 + 1 for i in range(n)]


def check(programs, tmp_path, arrs, shape, map_pidx, cells_pad):
    A = len(arrs)
    H, Z, B, P = (len(arrs[0][t]) for t in ref.TABLES)
    cells = len(arrs[0]["cell_flags"])
    rows = str(tmp_path / "rows.bin")
    write_rows(rows, arrs, shape, map_pidx, cells_pad)
    for build, exe in programs.items():
        out = str(tmp_path / ("state_" + build + ".bin"))
        r = subprocess.run([exe, rows, out], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (build, r.stdout[-2000:], r.stderr[-4000:])
        assert r.stdout.strip().split("\n")[-1].split()[:2] == ["put_main", "ok"], (build, r.stdout[-2000:])
        got = read_state(out, A, H, Z, B, P, cells, cells_pad)
        for a, arr in enumerate(arrs):
            e = ref.encode(arr, map_pidx)
            for i in range(H):  # humans: every word, the hidden flag bits by the rule
                want = e["hum"][:, i].copy()
                want[1] |= hidden_bits(shape, i, arr["humans"][i])
                assert np.array_equal(got["hum"][:, a, i], want), (build, a, i, got["hum"][:, a, i].tolist(), want.tolist())
            zl, bl, pl = arr["zombies"][:, 0] != 0, arr["bullets"][:, 0] != 0, arr["portals"][:, 0] != 0
            assert np.array_equal(got["zom"][:, a][:, zl], e["zom"][:, zl]) and not got["zom"][:, a][:, ~zl].any()  # empty: all-zero words
            assert np.array_equal(got["bul"][:, a][:, bl], e["bul"][:, bl]) and not got["bul"][:, a][:, ~bl].any()
            assert np.array_equal(got["por"][a][pl], e["por"][pl]) and not got["por"][a][~pl].any()
            hdr = arr["hdr"]
            tb, sr = int(hdr[12:14].view(np.uint64)[0]), int(hdr[14:16].view(np.uint64)[0])
            rng = hdr[20:38].astype(np.uint32) | (np.array(digits(sr), dtype=np.uint32) << 20) | (np.array(digits(tb), dtype=np.uint32) << 24)
            assert np.array_equal(got["rng"][a], rng), (build, a)
            rng2 = np.full(18, 0x10000, dtype=np.uint32)
            if shape["auto_reset"]:
                rng2 |= np.array(digits((tb + shape["reseed"]) % 2**64), dtype=np.uint32) << 24
            assert np.array_equal(got["rng2"][a], rng2), (build, a)
            s = got["scal"][a]
            for k in (0, 1, 2, 3, 4, 5, 6, 8, 9, 11, 12, 13, 14):
                assert s[k] == e["scal"][k], (build, a, k)
            assert s[7] == np.uint32(PATTERN).view(np.int32) and s[10] == 0 and s[16] == 0 and list(s[20:23]) == [0, 0, 0]
            assert np.uint32(s[15]) == np.uint32((int(np.uint32(hdr[10])) - 1042) % 2**32)
            cnt = ref.counts_of(arr)
            assert s[17] == cnt[0] + cnt[1] and s[18] == (cnt[5] + 63) // 64 and s[19] == (cnt[7] + 63) // 64
            fl = arr["cell_flags"]
            temp, pin = (fl & abi.CELL_TEMP) != 0, (fl & (abi.CELL_PIN_UP | abi.CELL_PIN_DN)) != 0
            assert np.array_equal(got["flags"][a, :cells], fl) and (got["flags"][a, cells:] == 0x5B).all()
            assert np.array_equal(got["aux_dmg"][a][temp], arr["cell_dmg"][temp]) and (got["aux_dmg"][a][~temp] == np.uint32(PATTERN).view(np.int32)).all()
            both = temp & pin
            assert np.array_equal(got["aux_pidx"][a][both], arr["cell_portal"][both].astype(np.int16)) and (got["aux_pidx"][a][~both] == 0x5B5B).all()


def shape_of(w):
    cfg = w.cfg
    return {"F": cfg.floors, "N": cfg.rows, "M": cfg.cols, "mode": cfg.mode, "n_agents": cfg.n_agents, "ind": cfg.ind,
            "npc_block": 16 if cfg.n_agent_profiles else 1, "auto_reset": cfg.auto_reset,
            "reseed": cfg.reseed_stride if cfg.reseed_stride > 0 else cfg.arenas}


@pytest.mark.parametrize("name", sc.NAMES)
def test_cases_dumps_through_the_lane_functions(programs, tmp_path, name):
    dumps, _ = sc.oracle_dumps(name)
    arrs = [ref.arena_arrays(d) for d in dumps][:3]
    w = sc.case(name).w
    map_pidx = [int(w.cfg.map_portal[i]) if w.cfg.map[i] in b"^v" else -1 for i in range(w.cells)]
    check(programs, tmp_path, arrs, shape_of(w), map_pidx, (w.cells + 15) // 16 * 16 + 16)


def synthetic_arena(rng, shape, H, Z, B, P, cells, map_pidx, first):
    F, N, M = shape["F"], shape["N"], shape["M"]
    i32 = lambda: int(rng.randint(-2**31, 2**31, dtype=np.int64))
    pos = lambda: [rng.randint(F), rng.randint(N), rng.randint(M)]
    hum = np.zeros((H, 28), dtype=np.int32)
    for i in range(H):
        if i % 5 == 4:
            continue  # a slot never used
        vec = rng.randint(-1, 3)
        ind = rng.randint(-1, 15) if vec == -1 else rng.randint(8 if vec == 2 else 4)
        hum[i] = [rng.randint(2), rng.randint(2), rng.randint(2), rng.randint(2)] + pos() + [1 + rng.randint(4), rng.randint(256),
                  i32(), i32(), i32(), i32(), i32(), i32(), vec, ind] + [rng.randint(65536) for _ in range(8)] + \
                 [rng.randint(256), rng.randint(256), rng.randint(-1, min(P, 255))]
    if first:
        hum[0, 0] = 0  # a dead `ind` (slot 0): it keeps its cell and its command
        hum[0, 2] = 0
        hum[1, 0:4] = 1
        hum[1, 4:7] = [F - 1, N - 1, M - 1]
        hum[1, 8:17] = [255, -1, -2**31, 2**31 - 1, 2**31 - 1, -5, -2**31, 2, 7]
        hum[1, 17:25] = 65535
        hum[1, 25:28] = [255, 255, min(P, 255) - 1]
        hum[2, 15:17] = [-1, 14]
    zom = np.zeros((Z, 7), dtype=np.int32)
    for i in range(Z):
        if rng.randint(3):
            zom[i] = [1] + pos() + [i32(), i32(), rng.randint(2)]
    bul = np.zeros((B, 11), dtype=np.int32)
    for i in range(B):
        if rng.randint(2):
            bul[i] = [1] + pos() + [1 + rng.randint(4), rng.randint(65536), i32(), rng.randint(-32768, 32768), rng.randint(65536),
                                    rng.randint(H + 1), rng.randint(2)]
    por = np.zeros((P, 4), dtype=np.int32)
    for i in range(P):
        if i % 3 != 1:
            por[i] = [1] + pos()
    if first:
        zom[Z - 1] = [1, F - 1, N - 1, M - 1, -1, -2**31, 1]
        bul[0] = [1, F - 1, N - 1, M - 1, 4, 65535, -2**31, -32768, 65535, H, 0]
        bul[B - 1] = [1, 0, 0, 0, 1, 0, 2**31 - 1, 32767, 0, 0, 1]
        por[P - 1] = [1, F - 1, N - 1, M - 1]
    flags = rng.randint(0, 64, size=cells).astype(np.uint8)
    chest = (flags & abi.CELL_CHEST) != 0
    flags[chest] |= (rng.randint(0, 4, size=int(chest.sum())) << 6).astype(np.uint8)
    temp, pin = (flags & abi.CELL_TEMP) != 0, (flags & (abi.CELL_PIN_UP | abi.CELL_PIN_DN)) != 0
    dmg = np.where(temp, rng.randint(-2**31, 2**31, size=cells, dtype=np.int64), 0).astype(np.int32)
    pidx = np.where(pin, np.where(temp, rng.randint(0, P, size=cells), map_pidx), -1).astype(np.int32)
    hdr = np.zeros(40, dtype=np.int32)
    h64 = hdr[:20].view(np.int64)
    h64[:] = [2**31 - 1 if first else rng.randint(2**31), i32(), i32(), -1, -2**31, 2**32 - 1 if first else 1042 + rng.randint(10**6),
              rng.randint(0, 2**63, dtype=np.int64), -1 if first else 999999999999999999, 2**31 - 1, i32()]
    hdr[20:38] = rng.randint(0, 65537, size=18)
    hdr[20], hdr[37] = 65536, 0
    hdr[38], hdr[39] = 1, abi.SAMPLE_END
    arr = {"hdr": hdr, "humans": hum, "zombies": zom, "bullets": bul, "portals": por, "cell_flags": flags, "cell_dmg": dmg,
           "cell_portal": pidx}
    arr["counts"] = ref.counts_of(arr)
    return arr


@pytest.mark.parametrize("H,Z,B,P,cells,mode,n_agents,npc_block", [(3, 5, 70, 9, (1, 5, 7), abi.MODE_TIMER, 1, 1),
                                                                   (22, 130, 64, 300, (4, 8, 9), abi.MODE_BATTLE, 8, 16),
                                                                   (12, 65, 129, 64, (2, 11, 13), abi.MODE_SQUAD, 3, 1)])
def test_synthetic_edge_values(programs, tmp_path, H, Z, B, P, cells, mode, n_agents, npc_block):
    F, N, M = cells
    ncell = F * N * M
    rng = np.random.RandomState(1000 * H + ncell)
    shape = {"F": F, "N": N, "M": M, "mode": mode, "n_agents": n_agents, "ind": 0, "npc_block": npc_block, "auto_reset": int(mode != abi.MODE_SQUAD),
             "reseed": 4096}
    map_pidx = rng.randint(0, P, size=ncell).astype(np.int16)
    arrs = [synthetic_arena(rng, shape, H, Z, B, P, ncell, map_pidx, a == 0) for a in range(3)]
    arrs[2]["zombies"][:] = 0  # an arena without a zombie: extent 0, no word of the large pool in use
    arrs[2]["counts"] = ref.counts_of(arrs[2])
    check(programs, tmp_path, arrs, shape, map_pidx, ncell + 11)
