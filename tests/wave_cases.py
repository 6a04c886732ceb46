"""The case lists of the wave-backend probes (tests/wave_checks.py): the smallest inputs that reach each edge an
operation has.  A row is 64 words, one per lane.  Generator states that have to reach an edge of the arithmetic are
built at the end, and tests/test_wave_probe.py asserts on the reference that each of them does."""
import wave_ref as R

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
EDGE32 = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]
LANE_IDX = [0, 15, 16, 31, 32, 63]


def row(f):
    return [f(i) & M32 for i in range(64)]


def noise(seed):
    """64 fixed words that look like nothing in particular (a 32-bit LCG)."""
    out, x = [], seed
    for _ in range(64):
        x = (x * 1664525 + 1013904223) & M32
        out.append(x)
    return out


RAMP = row(lambda i: i)
NOISE_A, NOISE_B, NOISE_C = noise(1), noise(2), noise(3)

# ---- lane crossing -----------------------------------------------------------------------------------------------
SHL1 = [
    row(lambda i: i + 1),
    row(lambda i: 0x100 * (i // 16 + 1) + i),          # differs at every lane, rows told apart
    row(lambda i: 0xAAAA0000 if i >= 16 else 0x5555),  # a step between lanes 15 and 16
    row(lambda i: 0xAAAA0000 if i >= 32 else 0x5555),  # ... 31 and 32
    row(lambda i: 0xAAAA0000 if i >= 48 else 0x5555),  # ... 47 and 48
    row(lambda i: M32 if i == 63 else 0),              # lane 63 alone: it reaches lane 62, and lane 63 reads 0
    row(lambda i: M32 if i == 0 else 0),               # lane 0 alone: nobody reads it
    NOISE_A,
]
# non-zero on lanes < 18 only
SUM18 = [
    row(lambda i: 1 if i < 18 else 0),
    row(lambda i: i + 1 if i < 18 else 0),
    row(lambda i: (1 << 24) // 18 if i < 18 else 0),   # all eighteen at 2^24 / 18: the largest tap sum
    row(lambda i: 5 if i == 0 else 0),
    row(lambda i: 5 if i == 15 else 0),
    row(lambda i: 5 if i == 16 else 0),
    row(lambda i: 5 if i == 17 else 0),
    row(lambda i: 0xF0000000 + i if i < 18 else 0),    # the sum wraps 2^32
    [x if i < 18 else 0 for i, x in enumerate(NOISE_A)],
]
SUM18_JUNK = NOISE_B  # junk on lanes >= 18: only "row 1 holds one sum" is asserted
MASKS = [1, 1 << 31, 1 << 32, 1 << 63, M64, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555, 0x8000000100000001, 0x00FF00F00F0000F0]
MASKS0 = MASKS + [0]  # where 0 is defined (not ctz64 / clz64)

# ---- per-lane arithmetic: every pair of the edge values sits in lanes 0..24 --------------------------------------
PAIR_A = row(lambda i: EDGE32[i % 5])
PAIR_B = row(lambda i: EDGE32[(i // 5) % 5])
ARITH = [(PAIR_A, PAIR_B), (PAIR_B, PAIR_A), (NOISE_A, NOISE_B), (NOISE_A, NOISE_A)]
PRED_ROWS = {
    "none": [0] * 64,
    "all": [1] * 64,
    "one": row(lambda i: int(i == 21)),
    "odd": row(lambda i: i & 1),
}
SHIFTS = [[0] * 64, [31] * 64, row(lambda i: i % 32), row(lambda i: 31 - i % 32)]
SHIFT_VALUES = [PAIR_A, NOISE_C, [M32] * 64, [1] * 64]
# operands of the 24-bit multiplies: inside the contract, and from 2^24 on, where the asm form masks (the generator
# feeds it an unreduced rl).  All 64 pairs fit one row
MUL_OPS = [0, 1, 1 << 16, (1 << 24) - 1, 1 << 24, (1 << 24) + 5, 0xFFFFFFFF, 0x12345678]
MUL_A = row(lambda i: MUL_OPS[i % 8])
MUL_B = row(lambda i: MUL_OPS[i // 8])
# mad24 inside its contract only: both factors below 2^24
MAD_OPS = [0, 1, 1 << 16, (1 << 24) - 1, 10, 65535, 63489 + 11 * 65537, 0x00ABCDEF]
MAD_A = row(lambda i: MAD_OPS[i % 8])
MAD_C = row(lambda i: EDGE32[(i // 8) % 5])

# ---- LDS and HBM regions -----------------------------------------------------------------------------------------
def region(nbytes, seed=0):
    """A region's first image: bytes that depend on their address, so that a word in the wrong place shows."""
    return bytes(((i * 7 + 3 + seed) ^ (i >> 8)) & 255 for i in range(nbytes))


SMALL = 1024  # bytes of the region of the store / load / OR probes: cells 256..511 are used, the rest are sentinels
PERM = row(lambda i: (i * 37 + 11) % 64)  # a permutation of the lanes: distinct cells, out of order
IDX_DISTINCT = [row(lambda i: 256 + PERM[i]), row(lambda i: 64 + i)]  # cells (bytes or words of the region)
IDX_ANY = [row(lambda i: 256 + (i * 5) % 17), row(lambda i: 0 if i < 32 else 255), row(lambda i: 64 + i)]  # lanes may share
VALUES = [NOISE_A, row(lambda i: 0x01010101 * (i + 1))]
# OR-ing bits into words: (word per lane, bits per lane, predicate)
OR_DISTINCT = [(row(lambda i: 70 + PERM[i]), NOISE_B, PRED_ROWS["all"]), (row(lambda i: 70 + i), NOISE_C, PRED_ROWS["odd"]),
               (row(lambda i: 70 + i), NOISE_C, PRED_ROWS["none"])]
# 2, 32 and 64 lanes on one word.  A word has 32 bits: with 64 lanes, lane i and lane i + 32 bring the same bit
OR_SHARED = [
    (row(lambda i: 80), row(lambda i: 1 << (i % 32)), row(lambda i: int(i in (5, 40)))),
    (row(lambda i: 80), row(lambda i: 1 << (i % 32)), row(lambda i: int(i < 32))),
    (row(lambda i: 80), row(lambda i: 1 << (i % 32)), row(lambda i: int(16 <= i < 48))),
    (row(lambda i: 80), row(lambda i: 1 << (i % 32)), PRED_ROWS["all"]),
    (row(lambda i: 80 + i % 2), row(lambda i: 1 << (i // 2)), PRED_ROWS["all"]),  # two words, 32 lanes each
]
# lanes colliding on the SAME bit of one word (bm_claim): exactly one of them may see it clear
OR_SAME_BIT = [
    (row(lambda i: 90), row(lambda i: 1 << 7), row(lambda i: int(i in (3, 50)))),
    (row(lambda i: 90), row(lambda i: 1 << 31), PRED_ROWS["all"]),
    (row(lambda i: 90), row(lambda i: 1), row(lambda i: int(i >= 32))),
    (row(lambda i: 90 + i // 16), row(lambda i: 1 << 13), PRED_ROWS["all"]),  # four words, 16 lanes each: one winner per word
]
LDS_ZERO_WORDS = [4, 252, 256, 260, 1024]
LDS_ZERO_BYTES = 4 * 1024 + 64
COPY_BYTES = [16, 1008, 1024, 1040, 4096, 4112, 8192 + 16]
COPY_REGION = 8192 + 16 + 64
SPLIT_BYTES = {1: [16, 1008, 1024], 2: [16, 1008, 1024, 1040, 2032, 2048], 4: [16, 1008, 1024, 1040, 4080, 4096]}
U_VALUES = [0xFFFFFFFF, 0xFFFF8000, 32767, 0x7FFFFFFF, 0x80000000, 0]  # -1, -32768, 32767, the ends of int32

# ---- the generator -----------------------------------------------------------------------------------------------
# (tb, serial): the pairs of tests/golden/kat.json come first in the tests; these are added
SEED_PAIRS = [
    (0, 1), (1, 0), (0, 999999999999999999), (999999999999999999, 0),
    (999999999999999999, 999999999999999999), (900000000000000000, 900000000000000009),
    (909090909090909090, 90909090909090909), (100000000000000000, 1), (9, 9), (10, 10),
    (1700000000, 0), (0, 123456789), (111111111111111111, 222222222222222222), (123456789, 1700000000),
    (990099009900990099, 9009009009009009), (1771155561, 42), (4294967296, 4294967295), (9223372036854775807, 9223372036854775807),
]
DRAWS, EVERY = 4096, 512
PREWARM = [(0, 0), (17, 0), (17, 1), (18, 0), (18, 1), (1023, 0), (1023, 1)]  # (warm, la2_ok)
JOMLE_WINDOWS = [(1 << 16) - 40, (1 << 24) - 40, (1 << 24) + (1 << 16) - 40, (1 << 32) - (1 << 16) - 40]
WINDOW_DRAWS = 80
SUM_BIAS_LANE = 63489 + 11 * 65537  # sf_core.hpp: every lane's share of the tap sum's bias, and the offset's
ROUND_STATES = 4096  # reference-generated states for the round, register for register


def base_state(jomle=None):
    """A warmed-up state whose tap 3 has seed 1 (tb's digit 3 is 0), so that solve_tap can place the tap sum."""
    g = R.Gen.srand(1700000123, 987654321)
    assert g.seed[3] == 1, g.seed
    if jomle is not None:
        g.jomle = jomle
    return g


def sum_state(target, jomle=None):
    return R.solve_tap(base_state(jomle), 3, target)


def lane18_is_65536():
    """A state whose next draw's new value is 65536 = 3^32768: the tap sum t has log3(t) * (jomle + 1) = 32768 mod 65536."""
    g = base_state()
    e = g.jomle + 1
    assert e & 1  # odd: invertible mod 65536
    lg = 32768 * pow(e, -1, 65536) % 65536
    return R.solve_tap(g, 3, pow(3, lg, R.MOD))


def lane18_negative():
    """A state after whose next round lane 18's signed power (lo16 - hi16 of the table product) is negative."""
    g = base_state()
    for _ in range(64):
        rl, e, la, seed, us = R.hot_regs(g)
        if R.s32(R.rng_round(rl, e, la, seed, us, [0] * 64)[2][18]) < 0:
            return g
        g.rand()
    raise AssertionError("no such state within 64 draws")


EDGE_STATES = {
    "sum_0": lambda: sum_state(0),
    "sum_65536": lambda: sum_state(65536),
    "lane18_negative": lane18_negative,
    "lane18_65536": lane18_is_65536,
}
EDGE_DRAWS = 40
# every tap's power at its largest and smallest (+-65535) with us = 10: the ends of the biased sum rng_reduce forms
REDUCE_ENDS = [(row(lambda i: 65535 if i < 18 else 0), row(lambda i: 10 if i < 18 else 0)),
               (row(lambda i: -65535 if i < 18 else 0), row(lambda i: 10 if i < 18 else 0)),
               (row(lambda i: 65535 if i < 18 else -65535), row(lambda i: 10 if i < 18 else 0)),
               (row(lambda i: (65535, -65535)[i & 1]), row(lambda i: 1 + i % 10 if i < 18 else 0))]
