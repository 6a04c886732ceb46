"""The wave-backend probes without a GPU: tests/wave_ref.py pinned on the oracle's known answers, every probe of
tests/wave_probe/probe_body.hpp on the CPU wave emulator against wave_ref bit for bit, and the case lists of
tests/wave_cases.py checked on the reference for the edge each of them is there to reach.  tests/test_gpu_wave_probe.py
runs the same comparisons (tests/wave_checks.py) on the device.

Two places where the emulator is not compared in full:
  * rng_round has no emulator form (WaveEmu::FUSED_ROUND is false): its result must be the stub's, so that a real
    implementation has to come with its test;
  * the three contracts the emulator states more strictly than the hardware gives (lds_or_rtn_u32's order of service,
    mad24's wide factors, sum18_row1 outside lanes 16..31) are compared in their weak form only."""
import ctypes as C
import os
import re

import pytest

import oracle_lib
import test_gpu_wave_probe as G
import wave_cases as K
import wave_checks as W
import wave_ref as R
from wave_probe_lib import CSRC, DEVICE_ONLY, LOGT_OFF, PROBES, emu_lib


# ---- the reference itself -----------------------------------------------------------------------------------------
def test_ref_generator_matches_the_oracle():
    """wave_ref's generator equals sfo_kat_rand / sfo_kat_rand_state for every case of tests/golden/kat.json (and the
    fixture's recorded answers) and for the added seed pairs: 4096 draws each, the state every 512."""
    L = oracle_lib.lib()
    assert len(K.SEED_PAIRS) >= 16 and len(W.SEED_PAIRS) == len(W.GOLD["rand"]) + len(K.SEED_PAIRS)
    for case in W.GOLD["rand"]:
        out, _ = W.ref_stream(case["tb"], case["serial"])
        assert out[:len(case["first"])] == case["first"]
        g = R.Gen.srand(case["tb"], case["serial"])
        for _ in range(4096):
            g.rand()
        assert g.state19() == case["state_after_4096"]
    for tb, serial in W.SEED_PAIRS:
        out, states = W.ref_stream(tb, serial)
        want = (C.c_int32 * K.DRAWS)()
        L.sfo_kat_rand(tb, serial, K.DRAWS, want)
        assert out == list(want), (tb, serial)
        g = R.Gen.srand(tb, serial)
        for k in range(K.DRAWS // K.EVERY):
            st = (C.c_int64 * 19)()
            L.sfo_kat_rand_state(tb, serial, (k + 1) * K.EVERY, st)
            for _ in range(K.EVERY):
                g.rand()
            assert g.state19() == list(st), (tb, serial, k)
            assert (g.rng_words(), g.jomle) == states[k]


def test_seed_pairs_reach_their_edges():
    ps = K.SEED_PAIRS
    assert any(tb == 0 for tb, _ in ps) and any(s == 0 for _, s in ps)
    digits = lambda x: "%018d" % x
    assert any(len(str(tb)) == 18 and "0" in digits(tb) and "9" in digits(tb) for tb, _ in ps)
    assert any(len(str(s)) == 18 and "0" in digits(s) and "9" in digits(s) for _, s in ps)
    assert all(0 <= tb < 1 << 63 and 0 <= s < 1 << 63 for tb, s in ps)  # the reference's seeds are signed 64-bit


def test_ref_constants_are_the_product_s():
    L = emu_lib()
    assert L.sfpe_sum_bias_lane() == K.SUM_BIAS_LANE and L.sfpe_logt_off() == LOGT_OFF
    assert L.sfpe_fused_round() == 0


# ---- the edges the case lists are there to reach, asserted on the reference ------------------------------------------
def _next_round(g):
    rl, e, la, seed, us = R.hot_regs(g)
    return R.rng_round(rl, e, la, seed, us, [K.SUM_BIAS_LANE] * 64)


def test_edge_states_reach_their_edges():
    g = K.EDGE_STATES["sum_0"]()
    assert g.tap_sum() == 0 and all(g.random)
    h = g.copy()
    h.rand()
    assert h.random[17] == 1  # binpow(sum + (sum == 0), ...) = 1: the log table's entry for residue 0 stands for it
    assert R.hot_regs(g)[2][17] == 0
    g = K.EDGE_STATES["sum_65536"]()
    assert g.tap_sum() == 65536 and all(g.random) and R.hot_regs(g)[2][17] == 32768
    g = K.EDGE_STATES["lane18_negative"]()
    rl, off, d, out = _next_round(g)
    assert R.s32(d[18]) < 0  # the + 65537 sign fix before & 1023 decides this draw
    h = g.copy()
    assert out == h.rand() and (R.s32(d[18]) & 1023) != out
    g = K.EDGE_STATES["lane18_65536"]()
    rl, off, d, out = _next_round(g)
    h = g.copy()
    h.rand()
    assert h.random[17] == 65536 and R.s32(d[18]) == -1 and out == 65536 & 1023


def test_round_reference_agrees_with_the_arithmetic():
    """The register-level statement of the round (what the device is compared with) against the generator's arithmetic:
    the draw's value, the new logs, and the tap sum the returned offset stands for — which lies inside the log table, and
    below LOGT_OFF where lo16 - hi16 went negative."""
    below = 0
    for g in W.round_cases():
        rl, off, d, out = _next_round(g)
        h = g.copy()
        assert out == h.rand()
        assert [x & 0xFFFF for x in rl[:18]] == [R.log3(r) for r in h.random]
        assert rl[18] == rl[17]
        for lane in R.ROW1:
            t = R.offset_t(off[lane], K.SUM_BIAS_LANE)
            assert -LOGT_OFF <= t <= 65536 and t % R.MOD == h.tap_sum()
            below += t < 0
        assert all(-LOGT_OFF <= R.offset_t(o, K.SUM_BIAS_LANE) <= 65536 for o in off)  # every lane loads
    assert below > 0, "no state looks the log up below LOGT_OFF"
    # the sum_0 edge state as load() meets it: the lookup issued for its next draw is the entry of residue 0
    g = K.EDGE_STATES["sum_0"]()
    rl, e, la, seed, us = R.hot_regs(g)
    d = R.signed_power(rl, seed)
    off = R.rng_reduce(d, us, [K.SUM_BIAS_LANE] * 64)
    assert R.offset_t(off[17], K.SUM_BIAS_LANE) % R.MOD == 0


def test_jomle_windows_cross():
    for j in K.JOMLE_WINDOWS:
        crossed = [b for b in (16, 24) if (j >> b) != ((j + K.WINDOW_DRAWS) >> b)]
        assert crossed, j
    assert any((j >> 24) != ((j + K.WINDOW_DRAWS) >> 24) for j in K.JOMLE_WINDOWS)
    assert K.JOMLE_WINDOWS[-1] + K.WINDOW_DRAWS < 1 << 32
    js = [g.jomle + 1 for g in W.round_cases()[-len(K.JOMLE_WINDOWS):]]
    assert all(e % (1 << 16) == 0 for e in js) and any(e % (1 << 24) == 0 for e in js)


def test_reduce_ends_stay_inside_the_table():
    """Every tap's power at +65535 and at -65535 with us = 10: the largest and smallest biased sum rng_reduce forms."""
    for d, us in K.REDUCE_ENDS:
        off = R.rng_reduce(d, us, [K.SUM_BIAS_LANE] * 64)
        for o in off:
            assert 0 <= o + 2 * (LOGT_OFF - K.SUM_BIAS_LANE // 2) <= 2 * (LOGT_OFF + 65536), "byte offset outside logt"
    top = R.rng_reduce(*K.REDUCE_ENDS[0], [K.SUM_BIAS_LANE] * 64)
    low = R.rng_reduce(*K.REDUCE_ENDS[1], [K.SUM_BIAS_LANE] * 64)
    assert R.offset_t(top[17], K.SUM_BIAS_LANE) % R.MOD == (1 + 18 * 10 * 65535) % R.MOD
    assert R.offset_t(low[17], K.SUM_BIAS_LANE) % R.MOD == (1 - 18 * 10 * 65535) % R.MOD


def test_case_lists_reach_their_edges():
    for a, b in ((15, 16), (31, 32), (47, 48)):
        assert any(v[a] != v[b] for v in K.SHL1)
    assert any(v[63] for v in K.SHL1)
    assert [(1 << 24) // 18] * 18 == K.SUM18[2][:18] and any(x for x in K.SUM18_JUNK[18:])
    assert {1, 1 << 31, 1 << 32, 1 << 63, K.M64, 0xAAAAAAAAAAAAAAAA} <= set(K.MASKS) and 0 in K.MASKS0
    pairs = set(zip(K.PAIR_A, K.PAIR_B))
    assert all((x, y) in pairs for x in K.EDGE32 for y in K.EDGE32)
    assert [0] * 64 in K.SHIFTS and [31] * 64 in K.SHIFTS
    assert {0, 1, 1 << 16, (1 << 24) - 1} <= set(K.MUL_OPS) and any(x >= 1 << 24 for x in K.MUL_OPS)
    assert set(zip(K.MUL_A, K.MUL_B)) == {(x, y) for x in K.MUL_OPS for y in K.MUL_OPS}
    assert all(x < 1 << 24 for x in K.MAD_OPS)
    assert sorted(sum(p) for _, _, p in K.OR_SHARED)[:1] == [2] and {32, 64} <= {sum(p) for _, _, p in K.OR_SHARED}
    assert K.LDS_ZERO_WORDS == [4, 252, 256, 260, 1024]
    assert K.COPY_BYTES == [16, 1008, 1024, 1040, 4096, 4112, 8192 + 16]
    assert (17, 0) in K.PREWARM and (18, 1) in K.PREWARM and (1023, 0) in K.PREWARM and (0, 0) in K.PREWARM


# ---- every probe on the emulator ----------------------------------------------------------------------------------
EMU_CHECKS = [
    W.lane_all, W.shl1, W.sum18_row1, W.readlane, W.setlane, W.ballot, W.frombits, W.bits64,
    W.select, W.sar31, W.le0, W.gts, W.ltu, W.minu, W.shifts, W.mul24, W.mad24,
    W.lds_stores, W.ulds, W.lds_loads, W.lds_or, W.lds_zero, W.copies, W.hbm, W.gload_u16_at, W.uniform_hbm,
    W.host_tables, W.pow_tables, W.log_pow, W.rng_reduce, W.rng_round, W.gen_srand, W.gen_windows,
]


@pytest.mark.parametrize("check", EMU_CHECKS, ids=lambda f: f.__name__)
def test_probe_on_emulator(check):
    check("emu")


def test_prewarm():
    """prewarm_one up to 1024 gives the state srand_ gives, from warm = 0, 17, 18 and 1023, with the first lookup already
    issued (la2_ok = 1) or not.  (17, 1) is run but not compared: prewarm_issue is only ever called from warm = 18 on and
    la2_ok is cleared wherever warm is set to 0, so the product never holds an issued lookup below 18; one issued there
    belongs to a state the 18th (general-form) draw replaces, prewarm_one's general branch does not clear the flag, and
    the draw at warm = 18 consumes the stale log.  The probe shows just that: the case ends in a different state."""
    res = W.gen_prewarm("emu")
    assert all(ok for case, ok in res.items() if case != (17, 1)), res
    assert set(res) == set(K.PREWARM)


def test_every_probe_is_checked_and_every_member_is_probed():
    """Every member of WaveGfx950, parsed from the header's text, is run by a probe or listed with the reason it is not;
    every probe is run by a check of both suites (the device-only ones by the GPU suite alone)."""
    txt = open(os.path.join(CSRC, "wave_gfx950.hpp")).read()
    body = txt[txt.index("struct WaveGfx950 {"):txt.rindex("};")]
    members = set(re.findall(r"^\s*static SF_DEV [^(]*?(\w+)\(", body, re.M))
    members |= set(re.findall(r"^\s*static constexpr \w+ (\w+)", body, re.M))
    members |= set(re.findall(r"^\s*struct (\w+) \{", body, re.M)[1:])
    members |= set(re.findall(r"^\s*using (\w+) =", body, re.M))
    assert len(members) > 50 and {"rng_round", "G2L", "FUSED_ROUND", "g2l_store", "V"} <= members
    assert not set(G.COVERED) & set(G.NOT_PROBED)
    assert members == set(G.COVERED) | set(G.NOT_PROBED), sorted(members ^ (set(G.COVERED) | set(G.NOT_PROBED)))
    assert set(G.COVERED.values()) <= set(PROBES)
    body_txt = open(os.path.join(os.path.dirname(__file__), "wave_probe", "probe_body.hpp")).read()
    listed = re.findall(r"X\((\w+)\)", body_txt[body_txt.index("#define SFP_PROBES"):])
    assert listed == PROBES
    assert set(W.PROBED_BY) == set(PROBES)
    src = open(G.__file__).read()
    for probe, fn in W.PROBED_BY.items():
        assert re.search(r"W\.%s\b" % fn.__name__, src), "%s is not run by the GPU suite" % probe
        if probe not in DEVICE_ONLY:
            assert fn in EMU_CHECKS or fn is W.gen_prewarm, probe
