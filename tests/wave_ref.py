"""What every operation of the wave backend means (strikeforce_amd/csrc/wave_gfx950.hpp, tests/emu/wave_emu.hpp), in
plain Python integers: the reference that tests/test_wave_probe.py and tests/test_gpu_wave_probe.py compare the
emulator and the device with, bit for bit.  Written from each operation's stated meaning — a wavefront is a list of 64
words, a predicate a list of 64 truth values, memory a list of words or a bytearray — and from the arithmetic of the
reference's generator (random.hpp:27-77, restated from oracle/sf_oracle.c o_rand / o_srand), never from the emulator.

Three operations promise less than the emulator happens to give; the functions here state the promise:
  * sum18_row1: the sum of lanes 0..17 of a value that is zero elsewhere, on lanes 16..31 (row1());
  * mad24: a * b + c for factors below 2^24 (nothing said about wider ones);
  * lds_or_rtn_u32: lanes that share a word are served one after the other in SOME order (lds_or_rtn_ok())."""

M32 = 0xFFFFFFFF
MOD = 65537
ROW1 = range(16, 32)


def s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def s24(x):
    x &= 0xFFFFFF
    return x - (1 << 24) if x >> 23 else x


# ---- lane crossing -----------------------------------------------------------------------------------------------
def lane():
    return list(range(64))


def shl1(v):
    """Lane i reads lane i + 1; lane 63 reads 0."""
    return list(v[1:]) + [0]


def sum18(v):
    """The sum of lanes 0..17 (mod 2^32): what sum18_row1 leaves on lanes 16..31 when v is zero on lanes >= 18."""
    return sum(v[:18]) & M32


def readlane(v, idx):
    return v[idx]


def setlane(v, idx, val):
    r = list(v)
    r[idx] = val
    return r


def ballot(p):
    return sum(1 << i for i in range(64) if p[i])


def frombits(m):
    return [(m >> i) & 1 for i in range(64)]


def rank_below(m):
    return [bin(m & ((1 << i) - 1)).count("1") for i in range(64)]


def popc64(m):
    return bin(m).count("1")


def ctz64(m):
    assert m
    return (m & -m).bit_length() - 1


def clz64(m):
    assert m
    return 64 - m.bit_length()


# ---- per-lane arithmetic -----------------------------------------------------------------------------------------
def select(p, a, b):
    return [x if c else y for c, x, y in zip(p, a, b)]


def sar31(v):
    return [M32 if x >> 31 else 0 for x in v]


def le0(v):
    return [int(s32(x) <= 0) for x in v]


def gts(a, b):
    return [int(s32(x) > s32(y)) for x, y in zip(a, b)]


def ltu(a, b):
    return [int(x < y) for x, y in zip(a, b)]


def minu(a, b):
    return [min(x, y) for x, y in zip(a, b)]


def shrv(a, sh):
    return [x >> s for x, s in zip(a, sh)]


def shlv(a, sh):
    return [(x << s) & M32 for x, s in zip(a, sh)]


def mul24_1(a, b):
    """v_mul_u32_u24: the low 32 bits of the product of the operands' low 24 bits."""
    return ((a & 0xFFFFFF) * (b & 0xFFFFFF)) & M32


def mul24(a, b):
    return [mul24_1(x, y) for x, y in zip(a, b)]


def mad24(a, b, c):
    """a * b + c; the contract covers factors below 2^24 only."""
    assert max(a) < 1 << 24 and b < 1 << 24
    return [(x * b + z) & M32 for x, z in zip(a, c)]


# ---- memory: words = list of ints, bytes = bytearray -------------------------------------------------------------
def store_words(mem, idx, val, p):
    """Predicated per-lane store to distinct cells; returns the new memory."""
    r = list(mem)
    for i, v, c in zip(idx, val, p):
        if c:
            r[i] = v
    return r


def store_bytes(mem, idx, val, p):
    r = bytearray(mem)
    for i, v, c in zip(idx, val, p):
        if c:
            r[i] = v & 255
    return r


def load(mem, idx, p):
    return [mem[i] if c else 0 for i, c in zip(idx, p)]


def lds_or(mem, idx, bits, p):
    r = list(mem)
    for i, b, c in zip(idx, bits, p):
        if c:
            r[i] |= b
    return r


def lds_or_rtn_ok(mem, idx, bits, p, got):
    """Is `got` what lds_or_rtn_u32 may return?  Lanes that share a word are served in some order: a lane without
    the predicate reads 0; every other lane reads the word's old value OR-ed with the bits of the lanes served before
    it.  Checked by walking the lanes of each word in the order of what they saw (a chain of growing sets)."""
    for i in range(64):
        if not p[i] and got[i] != 0:
            return False
    for w in set(i for i, c in zip(idx, p) if c):
        ls = [k for k in range(64) if p[k] and idx[k] == w]
        seen = mem[w]
        todo = set(ls)
        while todo:
            nxt = [k for k in todo if got[k] == seen]
            if not nxt:
                return False
            k = min(nxt, key=lambda k: (bits[k] & ~seen != 0, k))  # lanes that add nothing new first: any order among them
            todo.remove(k)
            seen |= bits[k]
    return True


def lds_zero(mem, nwords):
    return [0] * nwords + list(mem[nwords:])


def copy(dst, src, n):
    r = bytearray(dst)
    r[:n] = src[:n]
    return r


# ---- the generator's tables --------------------------------------------------------------------------------------
_LOG3 = None


def log3(v):
    """The discrete logarithm to base 3 in Z/65537*, by enumeration."""
    global _LOG3
    if _LOG3 is None:
        _LOG3 = {}
        x = 1
        for m in range(65536):
            assert x not in _LOG3  # 3 generates the whole group
            _LOG3[x] = m
            x = x * 3 % MOD
    return _LOG3[v]


def logt_entry(t):
    """Entry t + LOGT_OFF of the log table: log3 of the residue of t, and 0 for the residue 0."""
    r = t % MOD
    return log3(r) if r else 0


def table_product(m):
    """3^byte0(m) * 3^(256 byte1(m)) from the two halves of the power table, not reduced; bits of m above 16 ignored."""
    return mul24_1(pow(3, m & 255, MOD), pow(3, 256 * ((m >> 8) & 255), MOD))


def pow_bytes(m):
    return [table_product(x) for x in m]


def pow_pair(m4):
    return [table_product(x >> 2) for x in m4]


def mod65537(x):
    return x % MOD


# ---- the generator, random.hpp:27-77 -----------------------------------------------------------------------------
class Gen:
    """random[18], us[18], seed[18], jomle: any state, not only one _srand reaches."""

    def __init__(self, random, us, seed, jomle):
        self.random, self.us, self.seed, self.jomle = list(random), list(us), list(seed), jomle

    @classmethod
    def srand(cls, tb, u_s):
        us, seed = [], []
        for _ in range(18):
            us.append(u_s % 10 + 1)
            seed.append(tb % 10 + 1)
            u_s //= 10
            tb //= 10
        g = cls([0] * 18, us, seed, 18)
        for _ in range(1024):
            g.rand()
        return g

    def copy(self):
        return Gen(self.random, self.us, self.seed, self.jomle)

    def tap_sum(self):
        s = 1
        for r, u, e in zip(self.random, self.us, self.seed):
            s = (s + u * pow(r, e, MOD)) % MOD
        return s

    def rand(self):
        s = self.tap_sum()
        self.jomle += 1
        new = pow(s + (s == 0), self.jomle % (MOD - 1), MOD)
        self.random = self.random[1:] + [new]
        return new & 1023

    def state19(self):
        return self.random + [self.jomle]

    # the product's stored form (sf_core.hpp load() / store()): one word per tap, the scalars apart
    def rng_words(self):
        return [r | (u << 20) | (e << 24) for r, u, e in zip(self.random, self.us, self.seed)]

    def rng2_words(self):
        """The log form of a generator being warmed up: log3(random[i]), bit 16 for random[i] == 0, seed << 24."""
        return [(log3(r) if r else 0x10000) | (e << 24) for r, e in zip(self.random, self.seed)]


def solve_tap(g, k, target):
    """A copy of g with random[k] set so that the tap sum is `target` (mod 65537).  seed[k] must be 1: the tap's term is
    then us[k] * random[k] itself and the equation is linear."""
    assert g.seed[k] == 1
    h = g.copy()
    h.random[k] = 0
    rest = h.tap_sum()
    h.random[k] = (target - rest) * pow(h.us[k], MOD - 2, MOD) % MOD
    assert h.tap_sum() == target % MOD
    return h


# ---- the hot round, register for register (wave_gfx950.hpp rng_commit / rng_reduce / rng_round) --------------------
def rng_commit(rl, e, la):
    """rl shifted down by one lane, lanes 17 and 18 replaced by the 24-bit product e * la."""
    r = shl1(rl)
    r[17], r[18] = mul24_1(e, la[17]), mul24_1(e, la[18])
    return r


def signed_power(rl, seed):
    """d = lo16 - hi16 of the table product for the exponent rl * seed: congruent to 3^(rl seed), in (-65536, 65536)."""
    pr = pow_bytes(mul24(rl, seed))
    return [((x & 0xFFFF) - (x >> 16)) & M32 for x in pr]


def rng_reduce(d, us, bias):
    """x = d * us + bias per lane (signed 24-bit factors), summed over each row of 16 lanes, row 1 plus row 0's sum;
    t = lo16(x) - hi16(x); the byte offset 2 t + bias.  Every lane gets one: every lane loads from it."""
    x = [(s24(a) * s24(b) + c) & M32 for a, b, c in zip(d, us, bias)]
    rows = [sum(x[16 * r:16 * r + 16]) & M32 for r in range(4)]
    out = []
    for i in range(64):
        r = i >> 4
        X = (rows[r] + (rows[0] if r == 1 else 0)) & M32
        t = ((X & 0xFFFF) - (X >> 16)) & M32
        out.append(((t << 1) + bias[i]) & M32)
    return out


def draw_value(d18):
    """The draw's value from lane 18's signed power: the residue made non-negative, its low ten bits."""
    o = s32(d18)
    return (o + (MOD if o < 0 else 0)) & 1023


def rng_round(rl, e, la, seed, us, bias):
    """(rl after the round, byte offsets, d, the draw's value)."""
    r = rng_commit(rl, e, la)
    d = signed_power(r, seed)
    return r, rng_reduce(d, us, bias), d, draw_value(d[18])


def hot_regs(g):
    """The registers draw() holds for a warmed-up state g (no zero tap): (rl, e, la, seed, us).  Lane i < 18 carries
    log3(random[i]); lane 18 a copy of the newest log and seed 1; la the log of the tap sum, looked up ahead."""
    assert all(g.random)
    rl = [log3(r) for r in g.random] + [log3(g.random[17])] + [0] * 45
    la = [logt_entry(g.tap_sum())] * 64
    return rl, (g.jomle + 1) & M32, la, g.seed + [1] + [0] * 45, g.us + [0] * 46


def offset_t(off, bias):
    """The signed half-reduced tap sum t an offset stands for: off = 2 t + bias."""
    return s32(off - bias) // 2
