"""The device wave backend (strikeforce_amd/csrc/wave_gfx950.hpp), operation by operation, and the generator's hot round
at its edges, against tests/wave_ref.py.  Every comparison is device against reference, bit for bit — everything here is
integer, so there is no tolerance anywhere.  Each probe is one kernel of tests/wave_probe/probe_gfx950.hip (one wavefront
per case) built with the product's flags; the comparisons are the functions of tests/wave_checks.py, which also check
the sentinel bytes around every LDS and HBM region a probe may write.  tests/test_wave_probe.py runs the same functions
on the CPU wave emulator.

When an end-to-end digest differs from the oracle's, this suite narrows the difference to a primitive.

Where the hardware does more or less than the emulator, the contract the core relies on is the weaker one, and that is
what is asserted: lds_or_rtn_u32 serves colliding lanes in SOME order (exactly one sees a contested bit clear; which one
is printed, not asserted); mad24 is compared for factors below 2^24 only; sum18_row1 on lanes 16..31 only."""
import pytest

import wave_cases as K
import wave_checks as W
from wave_probe_lib import gpu_lib

pytestmark = pytest.mark.gpu

# member of WaveGfx950 -> the probe (tests/wave_probe/probe_body.hpp) that runs it
COVERED = {
    "lane": "lane_all", "all": "lane_all", "ballot": "ballot", "ctz64": "bits64", "clz64": "bits64", "popc64": "bits64",
    "uni": "uni", "readlane": "readlane", "setlane": "setlane", "select": "select", "sar31": "sar31", "le0": "le0",
    "ltu": "ltu", "gts": "gts", "minu": "minu", "shrv": "shrv", "shlv": "shlv", "frombits": "frombits",
    "rank_below": "rank_below", "sum18_row1": "sum18_row1", "shl1": "shl1", "mad24": "mad24", "mul24": "mul24",
    "mul24_su": "mul24_su", "lds_or_u32": "lds_or_u32", "lds_or_rtn_u32": "lds_or_rtn_u32",
    "lds_store_u32": "lds_store_u32", "lds_store_u8": "lds_store_u8", "lds_zero": "lds_zero", "lds_u8": "lds_u8",
    "lds_u8_any": "lds_u8", "lds_u32": "lds_u32", "ulds_u8": "ulds_load", "ulds_u32": "ulds_load",
    "ulds_store_u32": "ulds_store", "ulds_store_u8": "ulds_store", "rng_commit": "rng_split", "rng_reduce": "rng_reduce",
    "rng_round": "rng_round", "pow_bytes": "pow_bytes", "pow_pair": "pow_pair", "gload_u16_at": "gload_u16_at",
    "uload_i32": "u_i32", "ustore_i32": "u_i32", "uload_i16": "u_i16", "ustore_i16": "u_i16", "gload": "gload",
    "gload_u8": "gload_u8", "gload_u16": "gload_u16", "gstore": "gstore", "gstore_u8": "gstore_u8",
    "copy_g2l": "copy_g2l", "g2l_issue": "g2l_split1", "g2l_store": "g2l_split1", "copy_l2g": "copy_l2g",
}
# members without a probe, and why.  (The SF_STAMP_* / SF_COUNT / SF_PROF macros of the header are diagnostics of other
# builds and expand to nothing in the product; they are not members.)
NOT_PROBED = {
    "rng_prio_end": "no result: lowers the wave's priority under SF_RNG_PRIO == 2, nothing in the product build",
    "FUSED_ROUND": "a constant, not an operation: test_rng_round asserts the device takes the fused branch",
    "G2L": "the register type g2l_issue hands to g2l_store: run by the g2l_split probes",
    "V": "the per-lane value type", "P": "the predicate type",
}


@pytest.mark.parametrize("check", [
    W.lane_all, W.shl1, W.sum18_row1, W.readlane, W.setlane, W.uni, W.ballot, W.frombits, W.rank_below, W.bits64,
    W.select, W.sar31, W.le0, W.gts, W.ltu, W.minu, W.shifts, W.mul24, W.mad24,
    W.lds_stores, W.ulds, W.lds_loads, W.lds_zero, W.copies, W.hbm, W.gload_u16_at, W.uniform_hbm,
    W.host_tables, W.pow_tables, W.log_pow, W.rng_reduce, W.gen_srand, W.gen_windows,
], ids=lambda f: f.__name__)
def test_probe(check):
    check("gpu")


def test_weak_contracts_report(capsys):
    """What the hardware does where sum18_row1 (outside lanes 16..31) and mad24 (factors from 2^24 on) promise nothing is
    printed, not asserted."""
    W.sum18_row1("gpu"), W.mad24("gpu")
    with capsys.disabled():
        print("\n[wave probe] " + "; ".join("%s: %s" % kv for kv in W.REPORT.items() if kv[0].startswith(("sum18", "mad24"))))


def test_lds_or(capsys):
    """Colliding lanes: old | bits accounts for the final word, what every lane saw fits some order of service, and on a
    contested bit exactly one lane sees it clear (what bm_claim needs).  Which lane the hardware served first is printed."""
    W.lds_or("gpu")
    with capsys.disabled():
        for k, v in W.REPORT.items():
            if k.startswith("lds_or"):
                print("\n[wave probe] %s: %s" % (k, "; ".join(v)))


def test_rng_round():
    """rng_round against rng_commit -> mul24 -> pow_bytes -> rng_reduce on identical registers and against wave_ref, on
    4096 reference-generated states, the constructed edge states and the draws whose jomle crosses 2^16 / 2^24."""
    assert gpu_lib().sfp_fused_round() == 1  # Core::draw() on the device is this round
    assert len(W.round_cases()) >= K.ROUND_STATES + len(K.EDGE_STATES) + len(K.JOMLE_WINDOWS)
    W.rng_round("gpu")


def test_prewarm():
    """prewarm_one from warm = 0, 17, 18, 1023 to 1024 gives srand_'s state.  (17, la2_ok = 1) is run for its bounds
    only: see tests/test_wave_probe.py test_prewarm."""
    res = W.gen_prewarm("gpu")
    assert all(ok for case, ok in res.items() if case != (17, 1)), res
