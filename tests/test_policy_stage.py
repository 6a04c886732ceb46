"""The host arithmetic that lays the network's weights out for the policy kernels (csrc/sf_policy_stage.hpp), on the CPU:
tests/policy_stage/stage_main.cpp is built with AddressSanitizer and UBSan, run as a child process on a matrix this file
wrote, and the image it writes back is compared BIT FOR BIT with a numpy restatement of the layout each kernel's comment
gives (integer and exactly representable float operations only: no tolerance).  A wrong index here otherwise shows only
as a wrong network output on the device."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "policy_stage", "stage_main.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

HID, ACT, OBS_C, COMB, COMB_PAD = 160, 9, 32, 329, 352


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("policy_stage")
    out = str(d / "stage_main")
    r = subprocess.run(["g++"] + FLAGS + [SRC, "-o", out], capture_output=True, text=True)
    if r.returncode:
        probe = d / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        if subprocess.run(["g++"] + FLAGS + [str(probe), "-o", str(d / "probe")], capture_output=True).returncode:
            pytest.skip("g++ cannot link the sanitizer runtimes")
        pytest.fail("stage_main.cpp does not build:\n" + r.stderr)
    return out


def stage(exe, tmp_path, op, mats, dims, dtype=np.float32):
    """Runs one operation on the matrices `mats` (written back to back); returns (image, the lines it printed)."""
    src, dst = str(tmp_path / "in.f32"), str(tmp_path / "out.bin")
    np.concatenate([np.ascontiguousarray(m, dtype=np.float32).ravel() for m in mats]).tofile(src)
    r = subprocess.run([exe, op, src, dst] + [str(v) for v in dims], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr  # (a sanitizer report ends the program with a non-zero status)
    return np.fromfile(dst, dtype=dtype), r.stdout.split()


def distinct(*shape):
    """Every element its own row-major index: exact in f32 below 2^24, so a swapped index cannot cancel."""
    n = int(np.prod(shape))
    assert n < 1 << 24
    return np.arange(n, dtype=np.float32).reshape(shape)


def same_bits(got, want):
    want = np.ascontiguousarray(want).ravel()
    assert got.dtype == want.dtype and got.shape == want.shape
    u = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    assert np.array_equal(got.view(u), want.view(u))


def tiles_ref(w):
    """k_tail's weight stream: Wt[tile][k-step][lane][j] = W[16 tile + (lane & 15)][16 k-step + 4 (lane >> 4) + j]."""
    n, k = w.shape
    out = np.empty((n // 16, k // 16, 64, 4), dtype=np.float32)
    lane = np.arange(64)
    for tile in range(n // 16):
        for st in range(k // 16):
            for j in range(4):
                out[tile, st, :, j] = w[16 * tile + (lane & 15), 16 * st + 4 * (lane >> 4) + j]
    return out


def test_stage_tiles_appends_each_matrix_in_the_stream_order_of_k_tail(exe, tmp_path):
    # two tiles x two k-steps, then the padded combined_processor width on one tile: one block, the second behind the first
    a, b = distinct(32, 32), distinct(16, COMB_PAD) + 5000.0
    got, offsets = stage(exe, tmp_path, "tiles", [a, b], [32, 32, 16, COMB_PAD])
    assert [int(o) for o in offsets] == [0, a.size]
    same_bits(got, np.concatenate([tiles_ref(a).ravel(), tiles_ref(b).ravel()]))
    # (the restatement is a permutation: nothing lost, nothing doubled)
    assert np.array_equal(np.sort(got), np.sort(np.concatenate([a.ravel(), b.ravel()])))


def bf16_rne(x):
    """f32 -> (bf16 bits, its f32 value), round to nearest, ties to even, decided on the 16 dropped bits."""
    u = x.view(np.uint32).astype(np.uint64)
    keep, drop = u >> 16, u & 0xFFFF
    up = (drop > 0x8000) | ((drop == 0x8000) & ((keep & 1) == 1))
    bits = (keep + up).astype(np.uint32)
    return bits.astype(np.uint16), (bits << np.uint32(16)).view(np.float32)


def split_values(count):
    two = np.float32(2.0)
    special = [0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8), 1.0 + 2.0 ** -23,
               1e30, -1e30, 3.3e20, -3.3e20, 7.7e-20, -7.7e-20, 123456.789, -0.000123456789, 1.0, -1.0, 255.0, 257.0, 65537.0]
    special += [float(two ** e) for e in range(-60, 61, 5)] + [-float(two ** e) for e in range(-60, 61, 7)]
    rng = np.random.RandomState(20260)
    rest = count - len(special)
    draws = rng.standard_normal(rest) * 2.0 ** rng.randint(-40, 41, size=rest)
    v = np.concatenate([np.array(special, dtype=np.float64), draws]).astype(np.float32)
    assert np.all(np.isfinite(v)) and np.abs(v).max() <= np.float32(1e30)
    return v[rng.permutation(count)]


def test_split_weights_is_three_nearest_even_bf16_parts_in_the_image_of_k_gemm_b3(exe, tmp_path):
    n, k = 320, 32  # two 160-row strips x two 16-wide K tiles
    w = split_values(n * k).reshape(n, k)
    assert 1.0 + 2.0 ** -8 in w and 1.0 + 3 * 2.0 ** -8 in w
    hi, hi_f = bf16_rne(w.ravel())
    r1 = w.ravel() - hi_f  # (exact in f32: the parts of one number do not overlap)
    mid, mid_f = bf16_rne(r1)
    lo, _ = bf16_rne(r1 - mid_f)
    # the ties went to even: 1 + 2^-8 -> 1 (0x3f80), 1 + 3 2^-8 -> 1 + 2^-6 (0x3f82)
    flat = w.ravel()
    assert set(hi[flat == np.float32(1.0 + 2.0 ** -8)]) == {0x3F80} and set(hi[flat == np.float32(1.0 + 3 * 2.0 ** -8)]) == {0x3F82}
    # image [N / 160][K / 16][160][3 parts][16]
    parts = np.stack([hi, mid, lo]).reshape(3, n // 160, 160, k // 16, 16)
    want = parts.transpose(1, 3, 2, 0, 4)
    got, _ = stage(exe, tmp_path, "split", [w], [n, k], dtype=np.uint16)
    same_bits(got, want)


def test_conv0_weights_are_transposed_to_channel_tap_major(exe, tmp_path):
    w = distinct(HID, OBS_C, 3, 3)  # [n][c][ky][kx] -> [c][ky][kx][n]
    got, _ = stage(exe, tmp_path, "conv0", [w], [HID, OBS_C * 9])
    same_bits(got, w.transpose(1, 2, 3, 0))


def test_conv123_weights_are_permuted_to_the_k_order_of_an_nhwc_row(exe, tmp_path):
    w = distinct(HID, HID, 3, 3)  # [n][cin][ky][kx] -> [n][ky][kx][cin]
    got, _ = stage(exe, tmp_path, "perm", [w], [HID, HID])
    same_bits(got, w.transpose(0, 2, 3, 1))


@pytest.mark.parametrize("rows,cols,prows,pcols", [
    (HID, COMB, HID, COMB_PAD),  # combined_processor: 329 inputs padded to the GEMMs' K tiles
    (ACT, HID, 16, HID),         # the policy head's 9 rows, and
    (1, HID, 16, HID),           # the value head's one, padded to one 16-column MFMA tile
    (ACT, 1, 16, 1),             # their biases
    (1, 1, 16, 1),
])
def test_paddings_keep_the_matrix_in_the_corner_of_zeros(exe, tmp_path, rows, cols, prows, pcols):
    w = distinct(rows, cols) + 1.0  # (no zero of its own)
    want = np.zeros((prows, pcols), dtype=np.float32)
    want[:rows, :cols] = w
    got, _ = stage(exe, tmp_path, "pad", [w], [rows, cols, prows, pcols])
    same_bits(got, want)
