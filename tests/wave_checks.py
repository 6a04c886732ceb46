"""The comparisons of the wave-backend probes with tests/wave_ref.py, one function per probe, for either backend:
tests/test_wave_probe.py runs them on the CPU wave emulator, tests/test_gpu_wave_probe.py on the device.  Everything is
integer and compared bit for bit; every function also checks the sentinels of the regions its probe was given."""
import json
import os

import numpy as np

import wave_cases as K
import wave_ref as R
from wave_probe_lib import (DEVICE_ONLY, FILL, LOGT_ENTRIES, LOGT_OFF, RNG_WORDS, SC_JOMLE, SC_WARM, SC_WORDS, run,
                            tables)

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "kat.json")))
SEED_PAIRS = [(c["tb"], c["serial"]) for c in GOLD["rand"]] + K.SEED_PAIRS
PRED_NAMES = ["none", "all", "one", "odd"]
REPORT = {}  # what the hardware was seen to do where the contract leaves it open (printed by the GPU tests)


def same(got, want, what):
    got, want = [int(x) for x in got], [int(x) for x in want]
    assert len(got) == len(want), what
    for i, (x, y) in enumerate(zip(got, want)):
        assert x == y, "%s: first difference at %d: got %#x, want %#x" % (what, i, x, y)


def untouched(r, *names):
    """Result rows a probe has no business writing still hold the fill."""
    for n in names:
        assert (getattr(r, n) == FILL).all(), n


# ---- lane crossing -----------------------------------------------------------------------------------------------
def lane_all(b):
    r = run(b, "lane_all", 2)
    for c in range(2):
        same(r.out0[c], R.lane(), "lane"), same(r.out1[c], [1] * 64, "all")
    untouched(r, "out2")


def shl1(b):
    r = run(b, "shl1", len(K.SHL1), in0=K.SHL1)
    for c, v in enumerate(K.SHL1):
        same(r.out0[c], R.shl1(v), "shl1 case %d" % c)
        assert int(r.out0[c][63]) == 0
    untouched(r, "out1", "out2")


def sum18_row1(b):
    r = run(b, "sum18_row1", len(K.SUM18) + 1, in0=K.SUM18 + [K.SUM18_JUNK])
    for c, v in enumerate(K.SUM18):
        assert all(x == 0 for x in v[18:])
        same(r.out0[c][16:32], [R.sum18(v)] * 16, "sum18_row1 case %d, lanes 16..31" % c)
    junk = [int(x) for x in r.out0[len(K.SUM18)][16:32]]
    assert len(set(junk)) == 1 and junk[0] != FILL, "junk on lanes >= 18: row 1 holds one defined sum"
    REPORT["sum18_row1 outside lanes 16..31 (case 1: lanes 0..17 = 1..18)"] = \
        "lane 0: %d, lane 32: %d, lane 48: %d (the sum: %d)" % (r.out0[1][0], r.out0[1][32], r.out0[1][48], R.sum18(K.SUM18[1]))


def readlane(b):
    r = run(b, "readlane", len(K.LANE_IDX), so_n=1, in0=[K.NOISE_A] * len(K.LANE_IDX), s0=K.LANE_IDX)
    same(r.so[:, 0], [R.readlane(K.NOISE_A, i) for i in K.LANE_IDX], "readlane")


def setlane(b):
    n = len(K.LANE_IDX)
    r = run(b, "setlane", n, in0=[K.NOISE_B] * n, s0=K.LANE_IDX, s1=[0xC0FFEE00 + i for i in K.LANE_IDX])
    for c, i in enumerate(K.LANE_IDX):
        same(r.out0[c], R.setlane(K.NOISE_B, i, 0xC0FFEE00 + i), "setlane %d" % i)


def uni(b):
    n = len(K.LANE_IDX)
    r = run(b, "uni", n, in0=[K.NOISE_C] * n, in1=[K.RAMP] * n, s0=K.LANE_IDX)
    for c, i in enumerate(K.LANE_IDX):  # lanes below i sit out and keep their ramp word; the first active lane is i
        same(r.out0[c], K.RAMP[:i] + [K.NOISE_C[i]] * (64 - i), "uni from lane %d" % i)


def ballot(b):
    ps = [R.frombits(m) for m in K.MASKS0]
    r = run(b, "ballot", len(ps), so_n=2, in2=ps)
    same([int(x[0]) | (int(x[1]) << 32) for x in r.so], K.MASKS0, "ballot")


def _masks(ms):
    return dict(s0=[m & K.M32 for m in ms], s1=[m >> 32 for m in ms])


def frombits(b):
    r = run(b, "frombits", len(K.MASKS0), **_masks(K.MASKS0))
    for c, m in enumerate(K.MASKS0):
        same(r.out0[c], R.frombits(m), "frombits %#x" % m)


def rank_below(b):
    r = run(b, "rank_below", len(K.MASKS0), **_masks(K.MASKS0))
    for c, m in enumerate(K.MASKS0):
        same(r.out0[c], R.rank_below(m), "rank_below %#x" % m)


def bits64(b):
    r = run(b, "bits64", len(K.MASKS), so_n=3, **_masks(K.MASKS))
    for c, m in enumerate(K.MASKS):
        same(r.so[c], [R.popc64(m), R.ctz64(m), R.clz64(m)], "popc64 / ctz64 / clz64 of %#x" % m)
    r = run(b, "popc0", 1, so_n=1, **_masks([0]))
    assert int(r.so[0][0]) == 0


# ---- per-lane arithmetic -----------------------------------------------------------------------------------------
def _two(b, probe, fn):
    n = len(K.ARITH)
    r = run(b, probe, n, in0=[a for a, _ in K.ARITH], in1=[x for _, x in K.ARITH])
    for c, (a, x) in enumerate(K.ARITH):
        same(r.out0[c], fn(a, x), "%s case %d" % (probe, c))
    return r


def select(b):
    cs = [(a, x, K.PRED_ROWS[p]) for a, x in K.ARITH[:2] for p in PRED_NAMES]
    r = run(b, "select", len(cs), in0=[c[0] for c in cs], in1=[c[1] for c in cs], in2=[c[2] for c in cs])
    for c, (a, x, p) in enumerate(cs):
        same(r.out0[c], R.select(p, a, x), "select case %d" % c)


def sar31(b):
    vs = [K.PAIR_A, K.NOISE_A]
    r = run(b, "sar31", 2, in0=vs)
    for c, v in enumerate(vs):
        same(r.out0[c], R.sar31(v), "sar31")


def le0(b):
    vs = [K.PAIR_A, K.NOISE_A]
    r = run(b, "le0", 2, in0=vs)
    for c, v in enumerate(vs):
        same(r.out0[c], R.le0(v), "le0")


def gts(b):
    _two(b, "gts", R.gts)


def ltu(b):
    n = len(K.ARITH)
    bounds = [18, 0, 0xFFFFFFFF, 0x80000000]
    r = run(b, "ltu", n, in0=[a for a, _ in K.ARITH], in1=[x for _, x in K.ARITH], s0=bounds)
    for c, (a, x) in enumerate(K.ARITH):
        same(r.out0[c], R.ltu(a, x), "ltu case %d" % c)
        same(r.out1[c], R.ltu(a, [bounds[c]] * 64), "ltu against the scalar %#x" % bounds[c])
    r = run(b, "ltu", 1, in0=[K.RAMP], in1=[K.RAMP], s0=[18])  # the form every tap predicate takes: lane < 18
    same(r.out1[0], [1] * 18 + [0] * 46, "lane < 18")


def minu(b):
    _two(b, "minu", R.minu)


def shifts(b):
    cs = [(v, s) for v in K.SHIFT_VALUES for s in K.SHIFTS]
    for probe, fn in (("shrv", R.shrv), ("shlv", R.shlv)):
        r = run(b, probe, len(cs), in0=[c[0] for c in cs], in1=[c[1] for c in cs])
        for c, (v, s) in enumerate(cs):
            same(r.out0[c], fn(v, s), "%s case %d" % (probe, c))


def mul24(b):
    """Operands from 2^24 on as well: the asm form multiplies the low 24 bits, and the generator relies on it (rl is
    left unreduced on the hot path)."""
    r = run(b, "mul24", 2, in0=[K.MUL_A, K.NOISE_A], in1=[K.MUL_B, K.NOISE_B])
    same(r.out0[0], R.mul24(K.MUL_A, K.MUL_B), "mul24, all pairs")
    same(r.out0[1], R.mul24(K.NOISE_A, K.NOISE_B), "mul24, noise")
    n = len(K.MUL_OPS)
    r = run(b, "mul24_su", n, s0=K.MUL_OPS, in1=[K.MUL_A] * n)
    for c, s in enumerate(K.MUL_OPS):
        same(r.out0[c], R.mul24([s] * 64, K.MUL_A), "mul24_su %#x" % s)


def mad24(b):
    """Inside the contract only — both factors below 2^24.  The emulator masks wider factors to 24 bits; on the device
    __umul24 leaves the choice between the 24-bit and the 32-bit multiply to the compiler, so for wider factors the result
    may be either.  The core never passes one and nothing is promised: what one wide pair gives is reported, not asserted."""
    ss = [x for x in K.MAD_OPS]
    r = run(b, "mad24", len(ss), in0=[K.MAD_A] * len(ss), s0=ss, in1=[K.MAD_C] * len(ss))
    for c, s in enumerate(ss):
        same(r.out0[c], R.mad24(K.MAD_A, s, K.MAD_C), "mad24 by %#x" % s)
    # outside the contract, reported only: a factor of 2^24 + 5 times 2^24 + 3
    wide = int(run(b, "mad24", 1, in0=[[(1 << 24) + 3] * 64], s0=[(1 << 24) + 5], in1=[[0] * 64]).out0[0][0])
    REPORT["mad24 with factors 2^24 + 3 and 2^24 + 5"] = "%#x (all 32 bits multiplied: %#x, low 24 bits each: %#x)" % (
        wide, ((1 << 24) + 3) * ((1 << 24) + 5) & K.M32, 15)


# ---- LDS ---------------------------------------------------------------------------------------------------------
def _img(n, nbytes, seed=0):
    return [np.frombuffer(K.region(nbytes, seed + c), dtype=np.uint8) for c in range(n)]


def _words(img):
    return [int(x) for x in np.frombuffer(bytes(img), dtype="<u4")]


def _bytes_of(words):
    return np.array(words, dtype="<u4").tobytes()


def _word_cells(idx):
    """The byte cells of a case list as word cells of the same 1 KiB region (256 words)."""
    return [x - 64 if x >= 256 else x for x in idx]


def lds_stores(b):
    cs = [(i, v, K.PRED_ROWS[p]) for i in K.IDX_DISTINCT for v in K.VALUES for p in PRED_NAMES]
    img = _img(len(cs), K.SMALL)
    r = run(b, "lds_store_u8", len(cs), in0=[c[0] for c in cs], in1=[c[1] for c in cs], in2=[c[2] for c in cs], limg=img)
    for c, (i, v, p) in enumerate(cs):
        assert bytes(r.limg[c]) == bytes(R.store_bytes(bytes(img[c]), i, v, p)), "lds_store_u8 case %d" % c
    cs = [([x - 128 if x >= 256 else x for x in i], v, p) for i, v, p in cs]  # word cells 128..191 and 64..127 of 256
    r = run(b, "lds_store_u32", len(cs), in0=[c[0] for c in cs], in1=[c[1] for c in cs], in2=[c[2] for c in cs], limg=img)
    for c, (i, v, p) in enumerate(cs):
        same(_words(r.limg[c]), R.store_words(_words(img[c]), i, v, p), "lds_store_u32 case %d" % c)


def ulds(b):
    cs = [(0, 0x1FF, 0, 0xDEADBEEF), (511, 0x80, 127, 1), (1023, 7, 255, 0xFFFFFFFF)]  # byte cell, byte, word cell, word
    img = _img(len(cs), K.SMALL)
    r = run(b, "ulds_store", len(cs), s0=[c[0] for c in cs], s1=[c[1] for c in cs], s2=[c[2] for c in cs],
            s3=[c[3] for c in cs], limg=img)
    for c, (bi, bv, wi, wv) in enumerate(cs):
        want = bytearray(img[c])
        want[bi] = bv & 255
        want[4 * wi:4 * wi + 4] = wv.to_bytes(4, "little")
        assert bytes(r.limg[c]) == bytes(want), "ulds_store_u8 / ulds_store_u32 case %d" % c
    r = run(b, "ulds_load", len(cs), so_n=2, s0=[c[0] for c in cs], s2=[c[2] for c in cs], limg=img)
    for c, (bi, _, wi, _) in enumerate(cs):
        same(r.so[c], [img[c][bi], _words(img[c])[wi]], "ulds_u8 / ulds_u32 case %d" % c)
        assert bytes(r.limg[c]) == bytes(img[c])


def lds_loads(b):
    cs = [(i, K.PRED_ROWS[p]) for i in K.IDX_ANY for p in PRED_NAMES]
    img = _img(len(cs), K.SMALL)
    r = run(b, "lds_u8", len(cs), in0=[c[0] for c in cs], in2=[c[1] for c in cs], limg=img)
    for c, (i, p) in enumerate(cs):
        same(r.out0[c], R.load(img[c], i, p), "lds_u8 case %d" % c)
        same(r.out1[c], R.load(img[c], i, [1] * 64), "lds_u8_any case %d" % c)
        assert bytes(r.limg[c]) == bytes(img[c])
    cs = [(_word_cells(i), p) for i, p in cs]
    r = run(b, "lds_u32", len(cs), in0=[c[0] for c in cs], in2=[c[1] for c in cs], limg=img)
    for c, (i, p) in enumerate(cs):
        same(r.out0[c], R.load(_words(img[c]), i, p), "lds_u32 case %d" % c)
        assert bytes(r.limg[c]) == bytes(img[c])


def lds_or(b):
    """OR into LDS words.  Distinct words: the old value comes back.  Lanes sharing a word: the final word is old | all
    bits, and what each lane saw fits SOME order of service (wave_ref.lds_or_rtn_ok) — the emulator's lane order is one."""
    cs = K.OR_DISTINCT + K.OR_SHARED + K.OR_SAME_BIT
    img = _img(len(cs), K.SMALL)
    for c in range(len(K.OR_DISTINCT), len(cs)):  # shared words start clear of the bits the lanes bring
        img[c] = img[c].copy()
        img[c][4 * 80:4 * 100] = 0
    args = dict(in0=[c[0] for c in cs], in1=[c[1] for c in cs], in2=[c[2] for c in cs], limg=img)
    r0, r1 = run(b, "lds_or_u32", len(cs), **args), run(b, "lds_or_rtn_u32", len(cs), **args)
    for c, (w, bits, p) in enumerate(cs):
        before = _words(img[c])
        after = R.lds_or(before, w, bits, p)
        same(_words(r0.limg[c]), after, "lds_or_u32 case %d" % c)
        same(_words(r1.limg[c]), after, "lds_or_rtn_u32 case %d: the words" % c)
        got = [int(x) for x in r1.out0[c]]
        assert R.lds_or_rtn_ok(before, w, bits, p, got), "lds_or_rtn_u32 case %d: no order of service explains %s" % (c, got)
        if c < len(K.OR_DISTINCT):
            same(got, R.load(before, w, p), "lds_or_rtn_u32 case %d: the old values" % c)
    REPORT.pop("lds_or_rtn_u32, lanes colliding on one bit: the lane served first", None)
    for k, (w, bits, p) in enumerate(K.OR_SAME_BIT):  # bm_claim's contract: one winner per word
        got = [int(x) for x in r1.out0[len(K.OR_DISTINCT) + len(K.OR_SHARED) + k]]
        for word in sorted(set(w)):
            clear = [i for i in range(64) if p[i] and w[i] == word and not got[i] & bits[i]]
            assert len(clear) == 1, "same bit, word %d: lanes %s saw it clear" % (word, clear)
            REPORT.setdefault("lds_or_rtn_u32, lanes colliding on one bit: the lane served first", []).append(
                "case %d word %d: lane %d of %s" % (k, word, clear[0], [i for i in range(64) if p[i] and w[i] == word][:3] + ["..."]))


def lds_zero(b):
    img = _img(len(K.LDS_ZERO_WORDS), K.LDS_ZERO_BYTES)
    r = run(b, "lds_zero", len(img), s0=K.LDS_ZERO_WORDS, limg=img)
    for c, n in enumerate(K.LDS_ZERO_WORDS):
        assert bytes(r.limg[c]) == bytes(4 * n) + bytes(img[c][4 * n:]), "lds_zero of %d words" % n


# ---- copies ------------------------------------------------------------------------------------------------------
def copies(b):
    def go(probe, sizes):
        n = len(sizes)
        g, l = _img(n, K.COPY_REGION, 1), _img(n, K.COPY_REGION, 101)
        r = run(b, probe, n, s0=sizes, g=g, limg=l)
        for c, nb in enumerate(sizes):
            if probe == "copy_l2g":
                assert bytes(r.g[c]) == bytes(R.copy(bytes(g[c]), bytes(l[c]), nb)), "%s of %d bytes: HBM" % (probe, nb)
                assert bytes(r.limg[c]) == bytes(l[c]), "%s of %d bytes: LDS" % (probe, nb)
            else:
                assert bytes(r.limg[c]) == bytes(R.copy(bytes(l[c]), bytes(g[c]), nb)), "%s of %d bytes: LDS" % (probe, nb)
                assert bytes(r.g[c]) == bytes(g[c]), "%s of %d bytes: HBM" % (probe, nb)
    go("copy_g2l", K.COPY_BYTES)
    go("copy_l2g", K.COPY_BYTES)
    for u, sizes in K.SPLIT_BYTES.items():
        assert max(sizes) == 1024 * u and any(s < 1024 * u and s > 1024 * (u - 1) for s in sizes)
        go("g2l_split%d" % u, sizes)


# ---- HBM ---------------------------------------------------------------------------------------------------------
def hbm(b):
    cs = [(i, K.PRED_ROWS[p]) for i in K.IDX_ANY for p in PRED_NAMES]
    g = _img(len(cs), K.SMALL, 7)
    for probe, view in (("gload", lambda x: _words(x)), ("gload_u8", lambda x: [int(v) for v in x]),
                        ("gload_u16", lambda x: [int(v) for v in np.frombuffer(bytes(x), dtype="<u2")])):
        r = run(b, probe, len(cs), in0=[_word_cells(c[0]) if probe == "gload" else c[0] for c in cs], in2=[c[1] for c in cs], g=g)
        for c, (i, p) in enumerate(cs):
            i = _word_cells(i) if probe == "gload" else i
            same(r.out0[c], R.load(view(g[c]), i, p), "%s case %d" % (probe, c))
            assert bytes(r.g[c]) == bytes(g[c])
    cs = [(i, v, K.PRED_ROWS[p]) for i in K.IDX_DISTINCT for v in K.VALUES[:1] for p in PRED_NAMES]
    g = _img(len(cs), 2 * K.SMALL, 9)
    args = dict(in0=[c[0] for c in cs], in1=[c[1] for c in cs], in2=[c[2] for c in cs], g=g)
    r = run(b, "gstore", len(cs), **args)
    for c, (i, v, p) in enumerate(cs):
        same(_words(r.g[c]), R.store_words(_words(g[c]), i, v, p), "gstore case %d" % c)
    if b == "gpu":
        r = run(b, "gstore_u8", len(cs), **args)
        for c, (i, v, p) in enumerate(cs):
            assert bytes(r.g[c]) == bytes(R.store_bytes(bytes(g[c]), i, v, p)), "gstore_u8 case %d" % c


def gload_u16_at(b):
    logt, _ = tables(b)
    last = 2 * 65536 + 2 * LOGT_OFF
    offs = [[0] * 64, [last] * 64, K.row(lambda i: 2 * i), K.row(lambda i: last - 2 * i), K.row(lambda i: (K.NOISE_A[i] % (LOGT_ENTRIES)) * 2)]
    r = run(b, "gload_u16_at", len(offs), in0=offs)
    for c, o in enumerate(offs):
        same(r.out0[c], [R.logt_entry(x // 2 - LOGT_OFF) for x in o], "gload_u16_at case %d" % c)
        same(r.out0[c], [logt[x // 2] for x in o], "gload_u16_at case %d against the table" % c)


def uniform_hbm(b):
    """uload / ustore: a word the host wrote, then a store and the load right behind it from the same wave."""
    vals = K.U_VALUES
    n = len(vals)
    g = _img(n, 64, 3)
    for c in range(n):
        g[c] = g[c].copy()
        g[c][8:12] = np.frombuffer(vals[(c + 1) % n].to_bytes(4, "little"), np.uint8)
    r = run(b, "u_i32", n, so_n=2, s0=[2] * n, s1=[5] * n, s2=vals, g=g)
    for c, v in enumerate(vals):
        same(r.so[c], [vals[(c + 1) % n], v], "uload_i32 / ustore_i32 case %d" % c)
        want = bytearray(g[c])
        want[20:24] = v.to_bytes(4, "little")
        assert bytes(r.g[c]) == bytes(want)
    v16 = [0xFFFF, 0x8000, 0x7FFF, 0, 1]  # -1, -32768, 32767
    sx = lambda x: (x | 0xFFFF0000) if x & 0x8000 else x
    n = len(v16)
    g = _img(n, 64, 4)
    for c in range(n):
        g[c] = g[c].copy()
        g[c][6:8] = np.frombuffer(v16[(c + 1) % n].to_bytes(2, "little"), np.uint8)
    r = run(b, "u_i16", n, so_n=2, s0=[3] * n, s1=[9] * n, s2=v16, g=g)
    for c, v in enumerate(v16):
        same(r.so[c], [sx(v16[(c + 1) % n]), sx(v)], "uload_i16 / ustore_i16 case %d" % c)
        want = bytearray(g[c])
        want[18:20] = v.to_bytes(2, "little")
        assert bytes(r.g[c]) == bytes(want)


# ---- tables ------------------------------------------------------------------------------------------------------
def host_tables(b):
    """logt and exptab as the product's host code builds them: every entry."""
    logt, exptab = tables(b)
    assert len(logt) == LOGT_ENTRIES == LOGT_OFF + 65537
    want = np.array([R.logt_entry(t) for t in range(-LOGT_OFF, 65537)], dtype=np.uint16)
    bad = np.nonzero(logt != want)[0]
    assert bad.size == 0, "logt differs first at t = %d" % (int(bad[0]) - LOGT_OFF)
    assert int(logt[LOGT_OFF]) == 0 and int(logt[LOGT_OFF - 1]) == R.log3(65536) == 32768  # residue 0, and its neighbour below
    same(exptab, [pow(3, i, R.MOD) for i in range(256)] + [pow(3, 256 * i, R.MOD) for i in range(256)], "exptab")


def pow_tables(b):
    ms = np.arange(65536, dtype=np.uint32)
    junk = ms | ((ms * np.uint32(40503) + np.uint32(0x9E37)) << np.uint32(16))  # the same exponents, junk in bits 16..31
    want = np.array([R.table_product(m) for m in range(65536)], dtype=np.uint32)
    assert all(int(w) % R.MOD == pow(3, m, R.MOD) for m, w in enumerate(want))
    r = run(b, "pow_bytes", 2048, in0=np.concatenate([ms, junk]))
    assert (r.out0.reshape(-1)[:65536] == want).all(), "pow_bytes"
    assert (r.out0.reshape(-1)[65536:] == want).all(), "pow_bytes with junk in bits 16..31"
    r = run(b, "pow_pair", 1024, in0=ms * np.uint32(4))
    assert (r.out0.reshape(-1) == want).all(), "pow_pair"
    assert (r.out0.reshape(-1).astype(np.uint64) % R.MOD == [pow(3, m, R.MOD) for m in range(65536)]).all()


def log_pow(b):
    v = np.arange(1, 65537, dtype=np.uint32)
    r = run(b, "log_pow", 1024, in0=v)
    assert (r.out0.reshape(-1) == [R.log3(int(x)) for x in v]).all(), "the log of every value"
    assert (r.out1.reshape(-1) == v).all(), "pow3_v(logt[v + LOGT_OFF]) == v, 65536 included"


# ---- the generator -----------------------------------------------------------------------------------------------
def _scal(g, warm=1024):
    s = [0] * SC_WORDS
    s[SC_JOMLE], s[SC_WARM] = g.jomle & K.M32, warm
    return s


def _blank(n):
    return dict(rng=np.zeros((n, RNG_WORDS), np.uint32), rng2=np.zeros((n, RNG_WORDS), np.uint32), scal=np.zeros((n, SC_WORDS), np.uint32))


_STREAMS = {}


def ref_stream(tb, serial):
    """The reference's draws and checkpoints for one seed pair, computed once."""
    if (tb, serial) not in _STREAMS:
        g = R.Gen.srand(tb, serial)
        out, states = [], []
        for i in range(K.DRAWS):
            out.append(g.rand())
            if (i + 1) % K.EVERY == 0:
                states.append((g.rng_words(), g.jomle))
        _STREAMS[(tb, serial)] = (out, states)
    return _STREAMS[(tb, serial)]


def gen_srand(b):
    """(a) srand_ + 4096 draw() calls per seed pair; outputs, and the stored state every 512 draws."""
    n, per = len(SEED_PAIRS), K.DRAWS // K.EVERY
    r = run(b, "gen_srand", n, so_n=K.DRAWS, per=per, s0=[t & K.M32 for t, _ in SEED_PAIRS], s1=[t >> 32 for t, _ in SEED_PAIRS],
            s2=[s & K.M32 for _, s in SEED_PAIRS], s3=[s >> 32 for _, s in SEED_PAIRS], **_blank(n * per))
    for c, (tb, serial) in enumerate(SEED_PAIRS):
        out, states = ref_stream(tb, serial)
        same(r.so[c], out, "draws of (%d, %d)" % (tb, serial))
        for k, (words, jomle) in enumerate(states):
            same(r.rng[c * per + k], words, "state of (%d, %d) after %d draws" % (tb, serial, (k + 1) * K.EVERY))
            assert int(r.scal[c * per + k][SC_JOMLE]) == jomle


def warm_state(tb, serial, warm):
    us, seed = [], []
    for _ in range(18):
        us.append(serial % 10 + 1), seed.append(tb % 10 + 1)
        serial //= 10
        tb //= 10
    g = R.Gen([0] * 18, us, seed, 18)
    for _ in range(warm):
        g.rand()
    return g


def gen_prewarm(b):
    """(b) prewarm_one from `warm` to 1024 gives the state srand_ gives.  The stored form carries rng (for us), rng2 (the
    log state and seeds) and SC_WARM; la2_ok = 1 means the lookup was issued before the first call.  At warm = 17 a lookup
    issued early belongs to a state the 18th draw is about to replace; see test_wave_probe.py for what holds there."""
    tb, serial = SEED_PAIRS[0]
    full = warm_state(tb, serial, 1024)
    cs = K.PREWARM
    a = _blank(len(cs))
    for c, (warm, _) in enumerate(cs):
        g = warm_state(tb, serial, warm)
        a["rng"][c] = full.rng_words()  # the running episode's own generator: only its us digits matter here
        a["rng2"][c] = g.rng2_words()
        a["scal"][c] = _scal(full, warm)
    r = run(b, "gen_prewarm", len(cs), so_n=1, s0=[ok for _, ok in cs], s1=[1024 - w for w, _ in cs], **a)
    res = {}
    for c, (warm, ok) in enumerate(cs):
        assert int(r.scal[c][SC_WARM]) == 1024
        res[(warm, ok)] = [int(x) for x in r.rng2[c]] == full.rng2_words()
    return res


_ROUND = []


def round_cases():
    """Registers of the round: 4096 states the reference generates (64 seed-pair streams of 64 draws), then the edge
    states, then the draws whose jomle crosses 2^16 and 2^24.  Computed once."""
    if _ROUND:
        return _ROUND
    out = _ROUND
    pairs = SEED_PAIRS + [(1000003 * k + 7, 999983 * k + 1) for k in range(64 - len(SEED_PAIRS))]
    for tb, serial in pairs[:K.ROUND_STATES // 64]:
        g = R.Gen.srand(tb, serial)
        for _ in range(64):
            out.append(g.copy())
            g.rand()
    for name in sorted(K.EDGE_STATES):
        out.append(K.EDGE_STATES[name]())
    for j in K.JOMLE_WINDOWS:
        g = K.base_state(j + 39)  # the draw whose jomle crosses
        out.append(g)
    return out


def rng_round(b, bias=K.SUM_BIAS_LANE):
    """(c) rng_round against the split form on the same registers, and both against wave_ref, all 64 lanes of the byte
    offset: every lane loads from its own."""
    gs = round_cases()
    regs = [R.hot_regs(g) for g in gs]
    args = dict(in0=[x[0] for x in regs], in1=[x[2] for x in regs], in2=[x[3] for x in regs], in3=[x[4] for x in regs],
                s0=[x[1] for x in regs])
    split = run(b, "rng_split", len(gs), so_n=1, **args)
    fused = run(b, "rng_round", len(gs), so_n=1, **args)
    for c, (g, (rl, e, la, seed, us)) in enumerate(zip(gs, regs)):
        rl2, off, d, out = R.rng_round(rl, e, la, seed, us, [bias] * 64)
        same(split.out0[c], rl2, "rng_commit, state %d" % c)
        same(split.out1[c], off, "rng_reduce, state %d" % c)
        same(split.out2[c], d, "signed powers, state %d" % c)
        assert R.draw_value(int(split.so[c][0])) == out
        if b == "gpu":
            same(fused.out0[c], rl2, "rng_round: rl, state %d" % c)
            same(fused.out1[c], off, "rng_round: offsets, state %d" % c)
            assert int(fused.so[c][0]) == out, "rng_round: the draw's value, state %d" % c
    if b == "emu":  # no emulator form: the stub's result, so that a real one has to come with its test
        assert (fused.out1 == 0).all() and (fused.so == 0xDEADBEEF).all()
        assert (fused.out0 == np.array(args["in0"], dtype=np.uint32)).all()


def rng_reduce(b, bias=K.SUM_BIAS_LANE):
    cs = K.REDUCE_ENDS + [(K.NOISE_A, K.NOISE_B)]
    bs = [[bias] * 64] * len(K.REDUCE_ENDS) + [K.NOISE_C]
    r = run(b, "rng_reduce", len(cs), in0=[c[0] for c in cs], in1=[c[1] for c in cs], in2=bs)
    for c, ((d, us), bb) in enumerate(zip(cs, bs)):
        same(r.out0[c], R.rng_reduce(d, us, bb), "rng_reduce case %d" % c)


def _stored(gs):
    a = _blank(len(gs))
    for c, g in enumerate(gs):
        a["rng"][c], a["scal"][c] = g.rng_words(), _scal(g)
    return a


def gen_windows(b):
    """(d) jomle crossing 2^16, 2^24, 2^24 + 2^16 and 2^32 - 2^16: 80 draws through draw() and through draw_core;
    (e) the constructed states through both."""
    gs = [K.base_state(j) for j in K.JOMLE_WINDOWS] + [K.EDGE_STATES[n]() for n in sorted(K.EDGE_STATES)]
    want, after = [], []
    for g in gs:
        h = g.copy()
        want.append([h.rand() for _ in range(K.WINDOW_DRAWS)])
        after.append(h)
    for probe in ("gen_draw", "gen_draw_core"):
        r = run(b, probe, len(gs), so_n=K.WINDOW_DRAWS, **_stored(gs))
        for c, h in enumerate(after):
            same(r.so[c], want[c], "%s, state %d: the draws" % (probe, c))
            same(r.rng[c], h.rng_words(), "%s, state %d: the state afterwards" % (probe, c))
            assert int(r.scal[c][SC_JOMLE]) == h.jomle & K.M32
            if probe == "gen_draw_core":
                same(r.out0[c][16:32], [want[c][-1]] * 16, "draw_core's value on lanes 16..31")


PROBED_BY = {  # probe -> the function here that runs it
    "lane_all": lane_all, "shl1": shl1, "sum18_row1": sum18_row1, "readlane": readlane, "setlane": setlane, "uni": uni,
    "ballot": ballot, "frombits": frombits, "rank_below": rank_below, "bits64": bits64, "popc0": bits64,
    "select": select, "sar31": sar31, "le0": le0, "gts": gts, "ltu": ltu, "minu": minu, "shrv": shifts, "shlv": shifts,
    "mul24": mul24, "mul24_su": mul24, "mad24": mad24, "lds_store_u8": lds_stores, "lds_store_u32": lds_stores,
    "ulds_store": ulds, "ulds_load": ulds, "lds_u8": lds_loads, "lds_u32": lds_loads, "lds_or_u32": lds_or,
    "lds_or_rtn_u32": lds_or, "lds_zero": lds_zero, "copy_g2l": copies, "g2l_split1": copies, "g2l_split2": copies,
    "g2l_split4": copies, "copy_l2g": copies, "gload": hbm, "gload_u8": hbm, "gload_u16": hbm, "gstore": hbm,
    "gstore_u8": hbm, "gload_u16_at": gload_u16_at, "u_i32": uniform_hbm, "u_i16": uniform_hbm, "pow_bytes": pow_tables,
    "pow_pair": pow_tables, "log_pow": log_pow, "rng_round": rng_round, "rng_split": rng_round, "rng_reduce": rng_reduce,
    "gen_srand": gen_srand, "gen_prewarm": gen_prewarm, "gen_draw": gen_windows, "gen_draw_core": gen_windows,
}
assert set(DEVICE_ONLY) <= set(PROBED_BY)
