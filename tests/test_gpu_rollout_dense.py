"""sf_rollout_dense on the device (include/strikeforce_policy.h; rollout.RolloutBatch.dense) against tests/rollout_dense_ref.py.
Every destination starts as a sentinel bit pattern, so an element the kernel leaves out shows.  Bounds: every element of
every row bit for bit (in the 16-bit types a NaN may be any NaN, as the header says); against the simulator's own dense
observation bit for bit; the dense forward on the expanded rows reproduces the stored values and log-probabilities bit for
bit."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import policy_cases as pc
import rollout_dense_ref as dr
import test_gpu_rollout as tg
import test_rollout_dense_ref as cpu
from strikeforce_amd import env, policy, rollout

pytestmark = pytest.mark.gpu

T = 4
_dev, _bits = tg._dev, tg._bits
INT32_MAX = 2 ** 31 - 1
SPECIAL_POS = (0, dr.ROW - 1, 3, 4, 7, 8, 10, 11)  # first, last, both sides of a 16-byte unit (f32: 3 | 4, 16 bit: 7 | 8), one dword's halves
# -0, +-inf, a quiet and a signalling NaN with payloads; the f16 overflow tie, an f16 subnormal, the bf16 ties, neighbours of those
SPECIAL_BITS = np.concatenate([np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFF812345], dtype=np.uint32), np.array(
    [65520.0, 1e-6, 1 + 2.0 ** -8, -65520.0, 1 + 3 * 2.0 ** -8, 65519.0, -1e-6, 3.0e38, 5.9e-8, 2.9e-8], dtype=np.float32).view(np.uint32)])
COMBOS = tuple(itertools.product((dr.F32, dr.BF16, dr.F16), (dr.NCHW, dr.NHWC)))


def _special_triples():
    """(channel, row, column) of SPECIAL_POS read as an NCHW position and as an NHWC one."""
    out = []
    for p in SPECIAL_POS:
        ch, r = divmod(p, dr.GRID * dr.GRID)
        out.append((ch,) + divmod(r, dr.GRID))
        yx, ch = divmod(p, dr.CHANNELS)
        out.append((ch,) + divmod(yx, dr.GRID))
    return list(dict.fromkeys(out))


def counts_for(cap):
    return (0, 1, 3, 4, 5, cap - 1, cap, cap + 1, dr.MARKER)


@functools.lru_cache(maxsize=None)
def synthetic(agents, cap, seed=0):
    """keys, vals [T][agents][cap], counts [T][agents]: every list cap distinct positions in random order — the special
    positions first, rotated by the cell — with special values on every second entry; the counts cycle through counts_for(cap),
    so whatever lies behind a count is a valid-looking entry that must not be used."""
    rng = np.random.default_rng(1000 * agents + cap + seed)
    special = _special_triples()
    taken = {(c * dr.GRID + y) * dr.GRID + x for c, y, x in special}
    n = T * agents
    keys, vals = np.zeros((n, cap), dtype=np.uint32), np.zeros((n, cap), dtype=np.float32)
    counts = np.zeros(n, dtype=np.uint32)
    for c in range(n):
        counts[c] = counts_for(cap)[(2 * c + agents) % 9]
        lead = (special[c % len(special):] + special[:c % len(special)])[:cap]
        rest = [p for p in rng.choice(dr.ROW, size=cap + len(taken), replace=False).tolist() if p not in taken][:cap - len(lead)]
        triples = lead + [(p // 961, (p // 31) % 31, p % 31) for p in rest]
        keys[c] = [dr.key(*t) for t in triples]
        v = rng.uniform(0.25, 2.0, size=cap) * rng.choice(np.array([-1.0, 1.0]), size=cap)
        vals[c] = v.astype(np.float32)
        for j in range(0, min(cap, 2 * len(SPECIAL_BITS)), 2):
            vals[c].view(np.uint32)[j] = SPECIAL_BITS[(c + j // 2) % len(SPECIAL_BITS)]
    for a in (keys, vals, counts):
        a.setflags(write=False)
    return keys.reshape(T, agents, cap), vals.reshape(T, agents, cap), counts.reshape(T, agents)


def _load(rb, keys, vals, counts):
    rb.keys.copy_(_dev(keys)), rb.vals.copy_(_dev(vals)), rb.counts.copy_(_dev(counts))
    torch.cuda.synchronize()


def _sentinel_out(rows, dtype):
    """[rows][ROW] of the sentinel, as integers of the element's width."""
    if dtype == dr.F32:
        return torch.full((rows, dr.ROW), dr.SENTINEL32, dtype=torch.int32, device="cuda")
    return torch.full((rows, dr.ROW), dr.SENTINEL16, dtype=torch.int16, device="cuda")


def _raw(rb, out_ptr, rows, dtype, layout, slot=0, agent0=0, cells_ptr=None, valid_ptr=None):
    io = rollout.DenseIO()
    io.d_cells, io.slot, io.agent0, io.rows, io.dtype, io.layout, io.d_dense, io.d_valid = cells_ptr, slot, agent0, rows, dtype, layout, out_ptr, valid_ptr
    return rb.L.sf_rollout_dense(rb.h, C.byref(io))


def _image(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a.view(np.uint16)


def _check(got, want, dtype, what):
    bad = ~dr.same_elements(got, want, dtype)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())


# ---- 1: edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [8, 16, 512])
@pytest.mark.parametrize("agents", [1, 63, 64, 65, 130])
def test_edges_every_element_of_every_row(agents, cap):
    """T = 4, lists written straight into the buffer: counts 0, 1, 3, 4, 5, cap - 1, cap, cap + 1 and the marker; keys at
    position 0, at 30 751, on both sides of a 16-byte unit and in both halves of a dword, in either layout; unsorted; values
    -0, +-inf, NaN payloads, the f16 overflow tie and subnormals, the bf16 ties.  Three element types x two layouts, slot by
    slot with d_cells NULL, d_valid given (even combinations) or NULL (odd): every element of every row and every valid
    byte equal the restatement; the rows behind a call's `rows`, and the row behind the last, keep the sentinel."""
    keys, vals, counts = synthetic(agents, cap)
    if agents >= 63:
        assert set(counts.reshape(-1).tolist()) == set(counts_for(cap))
        assert any((np.diff(keys.reshape(-1, cap)[c].astype(np.int64)) < 0).any() for c in range(4))  # unsorted
    rb = rollout.RolloutBatch(agents, T, cap)
    _load(rb, keys, vals, counts)
    n = T * agents
    for i, (dtype, layout) in enumerate(COMBOS):
        out = _sentinel_out(n + 1, dtype)
        valid = torch.full((n + 1,), 0xA5, dtype=torch.uint8, device="cuda") if i % 2 == 0 else None
        for t in range(T):
            rc = _raw(rb, out[t * agents].data_ptr(), agents, dtype, layout, slot=t,
                      valid_ptr=None if valid is None else valid[t * agents:].data_ptr())
            assert rc == 0, rb.L.sf_last_error()
            if t == 0:
                rb.synchronize()
                sentinel = dr.SENTINEL32 if dtype == dr.F32 else dr.SENTINEL16
                assert bool((out[agents:] == sentinel).all()) and (valid is None or bool((valid[agents:] == 0xA5).all()))
        rb.synchronize()
        want, want_valid = dr.dense_rows(keys, vals, counts, cap, np.arange(n), dtype, layout)
        got = _image(out)
        _check(got[:n], want, dtype, (dtype, layout))
        assert (got[n] == (dr.SENTINEL32 if dtype == dr.F32 else dr.SENTINEL16)).all()
        if valid is not None:
            assert np.array_equal(valid.cpu().numpy()[:n], want_valid) and valid[n].item() == 0xA5
        if dtype == dr.F32 and agents >= 63:  # the special bit patterns arrived as they are
            assert (got == 0x7FC12345).any() and (got == 0xFF812345).any() and (got == 0x80000000).any()
    rb.close()


def test_repeated_positions_and_keys_that_name_none():
    """A list that names one position twice leaves either value there, in a dword's two halves independently; a key with
    channel 32..56, row 31 or column 31 writes nothing, inside the row or outside it (the rows around keep the sentinel)."""
    cap, agents = 16, 3
    keys, vals = np.zeros((T, agents, cap), dtype=np.uint32), np.zeros((T, agents, cap), dtype=np.float32)
    counts = np.zeros((T, agents), dtype=np.uint32)
    keys[1, 1, :8] = [dr.key(0, 0, 10), dr.key(0, 0, 11), dr.key(0, 0, 10), 32 * 9, 56 * 9 | 30 << 9 | 30 << 14, dr.key(0, 31, 0), dr.key(31, 30, 31),
                      dr.key(0, 0, 11)]
    vals[1, 1, :8] = [1.5, 2.5, 3.5, 7.0, 7.0, 7.0, 7.0, 4.5]
    counts[1, 1] = 8
    rb = rollout.RolloutBatch(agents, T, cap)
    _load(rb, keys, vals, counts)
    cell = _dev(np.array([1 * agents + 1], dtype=np.int32))
    for dtype, layout in COMBOS:
        out = _sentinel_out(3, dtype)
        assert _raw(rb, out[1].data_ptr(), 1, dtype, layout, cells_ptr=cell.data_ptr()) == 0
        rb.synchronize()
        got = _image(out)
        later, _ = dr.dense_rows(keys, vals, counts, cap, [4], dtype, layout)
        first, _ = dr.dense_rows(keys, vals, counts, cap, [4], dtype, layout, first_stays=True)
        assert ((got[1] == later[0]) | (got[1] == first[0])).all() and np.count_nonzero(got[1]) == 2
        sentinel = dr.SENTINEL32 if dtype == dr.F32 else dr.SENTINEL16
        assert (got[0] == sentinel).all() and (got[2] == sentinel).all()
    rb.close()


# ---- 2: cells ---------------------------------------------------------------------------------------------------------------
def test_cells_in_any_order_repeated_and_out_of_range():
    """65 agents, list_cap 16: cells in a random order with repeats and with -1, T * agents and INT32_MAX among them (zero
    row, valid 0, nothing read through them); agent0 > 0 with d_cells NULL; through RolloutBatch.dense, which also returns
    torch's channels_last format for NHWC."""
    agents, cap = 65, 16
    keys, vals, counts = synthetic(agents, cap)
    rb = rollout.RolloutBatch(agents, T, cap)
    _load(rb, keys, vals, counts)
    rng = np.random.default_rng(5)
    cells = rng.integers(0, T * agents, size=90).astype(np.int32)
    cells[[3, 40, 41, 77]] = [-1, T * agents, INT32_MAX, -(2 ** 31)]
    cells[50:53] = cells[10]
    d_cells = _dev(cells)
    for dtype, layout in ((dr.F32, dr.NCHW), (dr.BF16, dr.NHWC), (dr.F16, dr.NCHW)):
        out = _sentinel_out(len(cells), dtype).view(dr.TORCH_DTYPE[dtype])
        d, valid = rb.dense(cells=d_cells, dtype=dr.TORCH_DTYPE[dtype], channels_last=layout == dr.NHWC, out=out)
        rb.synchronize()
        want, want_valid = dr.dense_rows(keys, vals, counts, cap, cells, dtype, layout)
        _check(_image(out.view(torch.int32 if dtype == dr.F32 else torch.int16)), want, dtype, (dtype, layout))
        assert np.array_equal(valid.cpu().numpy(), want_valid)
        assert want_valid[[3, 40, 41, 77]].tolist() == [0, 0, 0, 0] and not want[[3, 40, 41, 77]].any()
    # a slot's agents from agent0 on, tensors allocated by the call
    for channels_last in (False, True):
        d, valid = rb.dense(t=2, agent0=5, rows=17, dtype=torch.bfloat16, channels_last=channels_last)
        rb.synchronize()
        assert tuple(d.shape) == (17, 32, 31, 31) and valid.shape == (17,)
        assert d.is_contiguous(memory_format=torch.channels_last if channels_last else torch.contiguous_format)
        want, want_valid = dr.dense_rows(keys, vals, counts, cap, 2 * agents + 5 + np.arange(17), dr.BF16, dr.NCHW)
        _check(d.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(17, -1), want, dr.BF16, channels_last)
        assert np.array_equal(valid.cpu().numpy(), want_valid)
    d, valid = rb.dense(t=3, agent0=60)  # rows: every agent behind agent0
    assert tuple(d.shape) == (5, 32, 31, 31) and d.dtype == torch.float32
    rb.close()


def test_the_largest_call():
    """rows = SF_ROLLOUT_DENSE_ROWS_MAX, NCHW / f32, 2.02 GB: every row the same cell except the last three (another cell),
    the widest destination offset the call allows.  Checked on the device: the last three rows are equal, the first and the
    row in front of them are equal, and the non-zero bit patterns of the whole buffer are as many as the two lists say."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6 * 2 ** 30:
        pytest.skip("under 6 GB of device memory free")
    agents, cap = 65, 16
    keys, vals, counts = synthetic(agents, cap)
    flat = counts.reshape(-1)
    c0, c1 = int(np.flatnonzero(flat == cap)[0]), int(np.flatnonzero(flat == 5)[0])
    rb = rollout.RolloutBatch(agents, T, cap)
    _load(rb, keys, vals, counts)
    rows = dr.ROWS_MAX
    cells = np.full(rows, c0, dtype=np.int32)
    cells[-3:] = c1
    out = torch.full((rows, dr.ROW), dr.SENTINEL32, dtype=torch.int32, device="cuda")
    d, valid = rb.dense(cells=_dev(cells), out=out.view(torch.float32))
    rb.synchronize()
    want, _ = dr.dense_rows(keys, vals, counts, cap, [c0, c1])
    assert torch.equal(out[-1], out[-2]) and torch.equal(out[-1], out[-3]) and torch.equal(out[0], out[-4])
    assert np.array_equal(_image(out[-1]), want[1]) and np.array_equal(_image(out[0]), want[0])
    assert int(torch.count_nonzero(out).item()) == (rows - 3) * cap + 3 * 5 and bool(valid.all())
    rb.close()


# ---- 3: against the simulator -----------------------------------------------------------------------------------------------
def test_rows_equal_the_simulators_dense_observation():
    """BASELINE configs[1], 8 arenas, T = 6 (tests/test_rollout_dense_ref.py's case): every tick sf_observe_device writes
    D[t] and the lists are recorded, at list_cap 512 and at 160.  dense(t), NCHW / f32, equals D[t] in every bit for every
    row with valid = 1; valid = counts <= list_cap; at 512 every row is valid, at 160 both kinds occur (with a count > 0)."""
    B, TT, CAP = cpu.SIM_ARENAS, cpu.SIM_T, 2048
    sim = env.ArenaBatch(cpu.sim_workload())
    sim.reset(*cpu.sim_workload().seeds())
    caps = (cpu.SIM_FULL_CAP, cpu.SIM_SMALL_CAP)
    rbs = [rollout.RolloutBatch(B, TT, cap, continuing=True) for cap in caps]
    D = torch.full((TT, B, 32, 31, 31), float("nan"), device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    d_keys, d_counts, d_act = torch.zeros((B, CAP), **i32), torch.zeros(B, **i32), torch.zeros(B, **i32)
    d_vals, d_pov = torch.zeros((B, CAP), device="cuda"), torch.zeros((B, 160), device="cuda")
    d_probs, d_one = torch.full((B, 9), 1 / 9, device="cuda"), torch.ones(B, device="cuda")
    lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
    cmds = _dev(cpu.sim_commands())
    torch.cuda.synchronize()
    for t in range(TT):
        sim.observe_device(D[t].data_ptr())
        sim.observe_sparse_device(*lists)
        sim.synchronize()
        for rb in rbs:
            rb.record(d_probs.data_ptr(), d_one.data_ptr(), d_act.data_ptr(), d_one.data_ptr(), *lists)
            rb.synchronize()
        sim.step_device(cmds[t].data_ptr(), 1)
        sim.synchronize()
    oracle = cpu.sim_oracle_observations()
    assert np.array_equal(D.cpu().numpy() != 0, oracle != 0)  # the device saw what the CPU test counted
    for cap, rb in zip(caps, rbs):
        assert rb.status()[0] == B
        stored = rb.counts.cpu().numpy().view(np.uint32)
        fits = stored <= cap
        for t in range(TT):
            out = _sentinel_out(B, dr.F32)
            d, valid = rb.dense(t, out=out.view(torch.float32))
            rb.synchronize()
            assert np.array_equal(valid.cpu().numpy(), fits[t].astype(np.uint8))
            got, want = _image(out), _image(D[t].reshape(B, -1).view(torch.int32))
            assert np.array_equal(got[fits[t]], want[fits[t]]), (cap, t)
            assert not got[~fits[t]].any()
        if cap == cpu.SIM_FULL_CAP:
            assert fits.all()
        else:
            assert (fits & (stored > 0)).any() and (~fits).any()
        print("list_cap %d: %d of %d rows valid" % (cap, fits.sum(), fits.size))
    for x in rbs + [sim]:
        x.close()


# ---- 4: what a dense network reads --------------------------------------------------------------------------------------------
def test_dense_forward_on_the_rows_reproduces_the_stored_block():
    """17 agents, T = 6, parameter set gain-1, the continuing rule, restarts on tick 0 (all) and tick 3 (every second agent),
    observations with 1 % non-zeros as lists.  A second policy replays the block through the DENSE entry:
    reset_memory_n(first[t]), sf_policy_forward on dense(t), update_actions(action[t]).  Every stored value and logp comes
    out again bit for bit (the header: the dense and the list forward agree in every bit)."""
    B, TT, CAP = 17, 6, 512
    rng = np.random.default_rng(17)
    net, net2 = (policy.PolicyBatch(pc.parameters("gain-1"), B) for _ in range(2))
    rb = rollout.RolloutBatch(B, TT, CAP, continuing=True)
    rb2 = rollout.RolloutBatch(B, TT, CAP, store_states=False, continuing=True)
    d_probs, d_value = tg._filled((B, 9)), tg._filled((B,))
    d_act, d_rew = torch.full((B,), 77, dtype=torch.int32, device="cuda"), torch.zeros(B, device="cuda")
    d_cmd = torch.zeros(B, dtype=torch.uint8, device="cuda")
    for t in range(TT):
        keys, vals, counts, pov = pc.lists_from_dense(pc.obs_sparse1(rng, B), CAP)
        assert counts.max() <= CAP
        flags = np.ones(B, dtype=np.uint8) if t == 0 else (np.arange(B) % 2 == 0).astype(np.uint8) if t == 3 else np.zeros(B, dtype=np.uint8)
        d = [_dev(x) for x in (keys, vals, counts, pov, flags)]
        lists = (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), CAP)
        net.predict_sparse(*lists, B, d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr(), seed=9, d_action_ptr=d_act.data_ptr(),
                           d_reset_mask_ptr=d[4].data_ptr())
        net.synchronize()
        rb.record(d_probs.data_ptr(), d_value.data_ptr(), d_act.data_ptr(), d_rew.data_ptr(), *lists, d_reset_mask_ptr=d[4].data_ptr())
        rb.synchronize()
    assert rb.status() == (B, 0, 0) and net.sparse_overflows() == 0
    assert rb.first.cpu().numpy().sum(axis=1).tolist() == [B, 0, 0, 9, 0, 0]
    p2, v2 = tg._filled((B, 9)), tg._filled((B,))
    for t in range(TT):
        out = _sentinel_out(B, dr.F32)
        dense, valid = rb.dense(t, out=out.view(torch.float32))
        rb.synchronize()
        assert bool(valid.all())
        net2.reset_memory(rb.first[t].data_ptr(), agents=B)
        net2.forward(dense.data_ptr(), B, p2.data_ptr(), v2.data_ptr())
        net2.update_actions(rb.action[t].data_ptr(), B)
        net2.synchronize()
        rb2.record(p2.data_ptr(), v2.data_ptr(), rb.action[t].data_ptr(), d_rew.data_ptr(), d_reset_mask_ptr=rb.first[t].data_ptr())
        rb2.synchronize()
    for name in ("value", "logp", "first"):
        assert np.array_equal(_bits(getattr(rb2, name)), _bits(getattr(rb, name))), name
    assert len(np.unique(_bits(rb.value))) > TT
    for x in (net, net2, rb, rb2):
        x.close()


# ---- 5: misuse on the device --------------------------------------------------------------------------------------------------
def test_misuse_is_refused_and_writes_nothing():
    agents, cap = 5, 8
    keys, vals, counts = synthetic(agents, cap)
    rb = rollout.RolloutBatch(agents, T, cap)
    _load(rb, keys, vals, counts)
    out = _sentinel_out(agents + 1, dr.F32)
    f32 = out.view(torch.float32)
    nostate = rollout.RolloutBatch(agents, T, cap, store_states=False)
    with pytest.raises(env.StrikeForceError, match=r"\(-4\).*keeps no states"):
        nostate.dense(0, out=f32)
    for kw in (dict(t=T), dict(t=-1), dict(t=0, agent0=1, rows=agents), dict(t=0, agent0=-1, rows=2), dict(t=0, rows=0), dict(t=0, agent0=agents)):
        with pytest.raises(env.StrikeForceError, match=r"\(-1\)"):
            rb.dense(out=f32, **kw)
    assert _raw(rb, out.data_ptr() + 4, 1, dr.F32, dr.NCHW) == -1 and b"16-byte" in rb.L.sf_last_error()  # misaligned
    assert _raw(rb, None, 1, dr.F32, dr.NCHW) == -1
    assert _raw(rb, out.data_ptr(), 1, 3, dr.NCHW) == -1 and _raw(rb, out.data_ptr(), 1, dr.F32, 2) == -1
    assert _raw(rb, out.data_ptr(), dr.ROWS_MAX + 1, dr.F32, dr.NCHW, cells_ptr=out.data_ptr()) == -1
    with pytest.raises(ValueError, match="at most 16384"):
        rb.dense(cells=torch.zeros(dr.ROWS_MAX + 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        rb.dense(0, dtype=torch.float64)
    rb.synchronize()
    assert bool((out == dr.SENTINEL32).all())
    d, valid = rb.dense(0, out=f32)  # and the good call writes
    rb.synchronize()
    want, want_valid = dr.dense_rows(keys, vals, counts, cap, np.arange(agents))
    assert np.array_equal(_image(out)[:agents], want) and (_image(out)[agents] == dr.SENTINEL32).all()
    assert np.array_equal(valid.cpu().numpy(), want_valid)
    for x in (rb, nostate):
        x.close()
