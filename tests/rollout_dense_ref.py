"""sf_rollout_dense (include/strikeforce_policy.h) restated in numpy: stored observation lists to dense rows, both layouts,
three element types.  The rules, per row: a good cell (inside the buffer, count <= list_cap) has vals[e] at the position
key e names for e < count, in list order (of two entries on one position the later one stays here; the contract allows
either), +0 everywhere else, valid 1; an entry whose key names no position is skipped; a bad cell is all +0, valid 0.
f32 keeps the bits; the 16-bit roundings are torch's CPU conversions (round to nearest even)."""
import numpy as np
import torch

CHANNELS, GRID = 32, 31
ROW = CHANNELS * GRID * GRID  # 30 752
ROWS_MAX = 16384
MARKER = 0xFFFFFFFF
F32, BF16, F16 = 0, 1, 2
NCHW, NHWC = 0, 1
TORCH_DTYPE = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
SENTINEL32, SENTINEL16 = 0x7FA5A5A5, 0x5AA5  # patterns no test value has; the 16-bit one is a NaN in neither 16-bit type


def key(ch, y, x):
    """The packing of sf_observe_sparse_device: channel * 9 | row << 9 | column << 14."""
    return np.uint32(ch * 9 | y << 9 | x << 14)


def position(keys, layout):
    """(position in the row, the key names one) for an array of keys."""
    k = np.asarray(keys).astype(np.int64)
    ch, y, x = (k & 511) // 9, (k >> 9) & 31, (k >> 14) & 31
    ok = (ch < CHANNELS) & (y < GRID) & (x < GRID)
    pos = (y * GRID + x) * CHANNELS + ch if layout == NHWC else (ch * GRID + y) * GRID + x
    return pos, ok


def convert(vals_f32, dtype):
    """f32 values -> the row's element bits: uint32 (unchanged) or uint16 (torch CPU's rounding)."""
    v = np.ascontiguousarray(vals_f32, dtype=np.float32)
    if dtype == F32:
        return v.view(np.uint32).copy()
    t = torch.from_numpy(v.copy()).to(TORCH_DTYPE[dtype])
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def dense_rows(keys, vals, counts, list_cap, cells, dtype=F32, layout=NCHW, first_stays=False):
    """keys uint32, vals float32 [T][agents][list_cap], counts uint32 [T][agents]; cells: int per row.
    first_stays: of two entries on one position the earlier one stays (the other outcome the contract allows).
    -> (bits [rows][ROW] uint32 or uint16, valid [rows] uint8)"""
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1, list_cap)
    vals = np.ascontiguousarray(vals, dtype=np.float32).reshape(-1, list_cap)
    counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
    cells = np.asarray(cells, dtype=np.int64).reshape(-1)
    out = np.zeros((len(cells), ROW), dtype=np.uint32 if dtype == F32 else np.uint16)
    valid = np.zeros(len(cells), dtype=np.uint8)
    for b, c in enumerate(cells):
        if c < 0 or c >= len(counts) or counts[c] > list_cap:
            continue
        valid[b] = 1
        n = int(counts[c])
        pos, ok = position(keys[c, :n], layout)
        bits = convert(vals[c, :n], dtype)
        pos, bits = pos[ok], bits[ok]
        if first_stays:
            pos, bits = pos[::-1], bits[::-1]
        out[b, pos] = bits  # (numpy: of a repeated index the last value is the one assigned)
    return out, valid


def same_elements(got, want, dtype):
    """Element-wise equality of two bit images: bit for bit in f32; in the 16-bit types a NaN equals any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    eq = got == want
    if dtype == F32:
        return eq
    exp, man = (0x7F80, 0x007F) if dtype == BF16 else (0x7C00, 0x03FF)
    nan = lambda a: ((a & exp) == exp) & ((a & man) != 0)
    return eq | (nan(got) & nan(want))
