"""sf_rollout_dense on the CPU: its restatement (tests/rollout_dense_ref.py) against policy_cases.dense_from_lists and a
hand-written row, the ABI surface, the refusals that need no device, and the oracle's observations for the end-to-end
case of tests/test_gpu_rollout_dense.py (which list_cap leaves lists that fit and lists that do not)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import policy_cases as pc
import rollout_dense_ref as dr
from oracle_lib import Oracle
from strikeforce_amd import build, config, env, rollout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the end-to-end case: BASELINE configs[1], 8 arenas (one agent each), 6 ticks of config.bench_commands
SIM_ARENAS, SIM_T, SIM_SMALL_CAP, SIM_FULL_CAP = 8, 6, 160, 512


def sim_workload():
    return config.baseline_workload("C2", arenas=SIM_ARENAS, auto_reset=0)


def sim_commands():
    return config.bench_commands(SIM_ARENAS, 1, SIM_T)[0]


@functools.lru_cache(maxsize=None)
def sim_oracle_observations():
    """[SIM_T][SIM_ARENAS][32][31][31]: the oracle's observation in front of each tick's step."""
    w = sim_workload()
    assert w.cfg.arenas == SIM_ARENAS and w.cfg.n_agents == 1
    o = Oracle(w)
    o.reset(*w.seeds())
    cmds, obs = sim_commands(), []
    for t in range(SIM_T):
        obs.append(o.observe().reshape(SIM_ARENAS, pc.CHANNELS, pc.GRID, pc.GRID).copy())
        o.step(cmds[t])
    o.close()
    return np.stack(obs)


def test_restatement_equals_dense_from_lists():
    """30 random observations (1 % non-zero) as lists that fit, T = 3 x 10 agents: NCHW / f32 rows of every cell equal
    policy_cases.dense_from_lists, and the observation they came from, bit for bit; the 16-bit rows equal torch's
    conversion of that observation; NHWC is the permutation."""
    rng = np.random.default_rng(11)
    obs = pc.obs_sparse1(rng, 30) + np.float32(0)  # (the maker's zeros are signed; a zero is no list entry)
    keys, vals, counts, _ = pc.lists_from_dense(obs, 512)
    assert counts.max() <= 512 and counts.min() > 0
    cells = rng.permutation(30)
    got, valid = dr.dense_rows(keys, vals, counts, 512, cells)
    want = pc.dense_from_lists(keys, vals, counts)[cells].reshape(30, -1)
    assert valid.all() and np.array_equal(got, want.view(np.uint32))
    assert np.array_equal(got, obs[cells].reshape(30, -1).view(np.uint32))
    for dtype in (dr.BF16, dr.F16):
        g16, _ = dr.dense_rows(keys, vals, counts, 512, cells, dtype=dtype)
        assert np.array_equal(g16, dr.convert(obs[cells].reshape(30, -1), dtype))
    nhwc, _ = dr.dense_rows(keys, vals, counts, 512, cells, layout=dr.NHWC)
    assert np.array_equal(nhwc.reshape(30, 31, 31, 32).transpose(0, 3, 1, 2).reshape(30, -1), got)


@pytest.mark.parametrize("layout", [dr.NCHW, dr.NHWC])
def test_restatement_on_a_hand_written_row(layout):
    """Three entries, unsorted: (channel 31, row 30, column 30) = 2.5, (0, 0, 0) = -1, (3, 7, 11) = 0.5.  NCHW positions
    30 751, 0 and (3 * 31 + 7) * 31 + 11 = 3 111; NHWC positions (30 * 31 + 30) * 32 + 31 = 30 751, 0 and
    (7 * 31 + 11) * 32 + 3 = 7 299.  A second cell holds the marker, a third lies outside the buffer."""
    keys = np.zeros((3, 4), dtype=np.uint32)
    vals = np.zeros((3, 4), dtype=np.float32)
    keys[0, :3] = [dr.key(31, 30, 30), dr.key(0, 0, 0), dr.key(3, 7, 11)]
    vals[0, :3] = [2.5, -1.0, 0.5]
    keys[0, 3], vals[0, 3] = dr.key(5, 5, 5), 9.0  # behind the count: not looked at
    counts = np.array([3, dr.MARKER, 5], dtype=np.uint32)
    got, valid = dr.dense_rows(keys, vals, counts, 4, [0, 1, 2, 3, -1], layout=layout)
    assert valid.tolist() == [1, 0, 0, 0, 0]
    want = np.zeros(dr.ROW, dtype=np.float32)
    where = (30751, 0, 3111) if layout == dr.NCHW else (30751, 0, 7299)
    want[list(where)] = [2.5, -1.0, 0.5]
    assert np.array_equal(got[0].view(np.float32), want) and np.count_nonzero(got[0]) == 3
    assert not got[1:].any()
    # a key that names no position is skipped; of two entries on one position either stays
    keys[0, :3] = [dr.key(3, 7, 11), 32 * 9, dr.key(3, 7, 11)]
    a, _ = dr.dense_rows(keys, vals, counts, 4, [0], layout=layout)
    b, _ = dr.dense_rows(keys, vals, counts, 4, [0], layout=layout, first_stays=True)
    assert a[0].view(np.float32)[where[2]] == 0.5 and b[0].view(np.float32)[where[2]] == 2.5
    assert np.count_nonzero(a[0]) == 1 and np.count_nonzero(b[0]) == 1


def test_sixteen_bit_roundings_of_the_edge_values():
    """65 520 is the f16 tie that overflows to infinity, 1e-6 an f16 subnormal, 1 + 2^-8 the bf16 tie that rounds to even."""
    v = np.array([65520.0, 1e-6, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -0.0, np.inf], dtype=np.float32)
    h, b = dr.convert(v, dr.F16), dr.convert(v, dr.BF16)
    assert h[0] == 0x7C00 and 0 < h[1] < 0x0400 and h[4] == 0x8000 and h[5] == 0x7C00
    assert b[2] == 0x3F80 and b[3] == 0x3F82 and b[4] == 0x8000 and b[5] == 0x7F80


def test_struct_matches_the_header():
    header = open(os.path.join(ROOT, "include", "strikeforce_policy.h")).read()
    body = re.search(r"typedef struct sf_rollout_dense_io \{(.*?)\} sf_rollout_dense_io;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        names += [n.strip(" *\n") for n in re.sub(r"^\s*(const\s+)?\w+\s", "", decl.strip()).split(",") if n.strip()]
    assert names == [f[0] for f in rollout.DenseIO._fields_], names
    assert C.sizeof(rollout.DenseIO) == 8 + 5 * 4 + 4 + 8 + 8  # a pointer, five ints, padding, two pointers
    assert rollout.DenseIO.d_dense.offset == 32 and rollout.DenseIO.d_valid.offset == 40
    for name, value in (("SF_DENSE_F32", dr.F32), ("SF_DENSE_BF16", dr.BF16), ("SF_DENSE_F16", dr.F16), ("SF_DENSE_NCHW", dr.NCHW),
                        ("SF_DENSE_NHWC", dr.NHWC), ("SF_ROLLOUT_DENSE_ROWS_MAX", dr.ROWS_MAX)):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == value, name
    assert (rollout.DENSE_F32, rollout.DENSE_BF16, rollout.DENSE_F16) == (dr.F32, dr.BF16, dr.F16)
    assert (rollout.DENSE_NCHW, rollout.DENSE_NHWC, rollout.DENSE_ROWS_MAX, rollout.DENSE_ROW) == (dr.NCHW, dr.NHWC, dr.ROWS_MAX, dr.ROW)


def test_symbol_is_built_and_refuses_without_a_device():
    """Null handle, rows 0 and SF_ROLLOUT_DENSE_ROWS_MAX + 1, an unknown dtype and layout, a null and a misaligned
    destination: SF_ERR_ARG, each with its own message, none of them touching a device."""
    build.build(verbose=False)
    L = env.load_library()
    assert hasattr(L, "sf_rollout_dense") and "sf_rollout_dense" in rollout.EXPORTS
    assert hasattr(rollout.RolloutBatch, "dense")
    rollout._bind(L)

    def call(handle=None, **kw):
        io = rollout.DenseIO()
        io.rows, io.dtype, io.layout, io.d_dense = 1, dr.F32, dr.NCHW, 4096
        for k, v in kw.items():
            setattr(io, k, v)
        return L.sf_rollout_dense(handle, C.byref(io)), L.sf_last_error().decode()

    assert L.sf_rollout_dense(None, None) == -1
    for kw, word in ((dict(), "null rollout"), (dict(rows=0), "rows"), (dict(rows=dr.ROWS_MAX + 1), "rows"), (dict(rows=-1), "rows"),
                     (dict(dtype=3), "dtype"), (dict(dtype=-1), "dtype"), (dict(layout=2), "layout"), (dict(d_dense=None), "d_dense"),
                     (dict(d_dense=4104), "d_dense")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)


def test_oracle_observations_of_the_end_to_end_case():
    """What tests/test_gpu_rollout_dense.py relies on: at list_cap = 160 at least one observation of the 48 fits with
    count > 0 and at least one does not; at list_cap = 512 every one fits.  The lists of the oracle's observations expand
    to those observations again."""
    obs = sim_oracle_observations()
    flat = obs.reshape(SIM_T * SIM_ARENAS, -1)
    counts = np.count_nonzero(flat, axis=1)
    print("non-zeros per observation: min %d max %d; above %d: %d of %d" % (counts.min(), counts.max(), SIM_SMALL_CAP,
                                                                             (counts > SIM_SMALL_CAP).sum(), counts.size))
    assert SIM_SMALL_CAP % 4 == 0 and SIM_FULL_CAP % 4 == 0
    assert ((counts > 0) & (counts <= SIM_SMALL_CAP)).any() and (counts > SIM_SMALL_CAP).any()
    assert (counts <= SIM_FULL_CAP).all()
    for cap in (SIM_SMALL_CAP, SIM_FULL_CAP):
        keys, vals, cnt, _ = pc.lists_from_dense(flat, cap)
        got, valid = dr.dense_rows(keys, vals, cnt, cap, np.arange(len(cnt)))
        assert np.array_equal(valid, (counts <= cap).astype(np.uint8))
        fits = valid == 1
        assert np.array_equal(got[fits], (flat[fits] + np.float32(0)).view(np.uint32))  # (+ 0: a -0 of the oracle's is no list entry)
        assert not got[~fits].any()
