"""sf_state_put_device / sf_load_arena on the MI355X (k_put_init / k_put_check / k_put_write) through the C-ABI and the Python
surface: the inverse of sf_state_device.  Every comparison is bit for bit.

Environment A is a case of tests/state_records_cases.py played to its step; environment B has the same configuration, other
seeds and a few steps of its own, so that every buffer holds foreign state.  What sf_state_device writes for A is put into
B; then all ten outputs and the digests are equal, and under the continuation rows of tests/state_put_cases.py the digest
after every step, observations at three steps, results and sf_done at the end.  The oracle's dumps go the same way
(put_state and, for one arena, sf_load_arena) and device and oracle agree at every step after.  Forks, untouched arenas,
cuts, parts, refusals (one field at its first bad value per row, beside good rows), a captured graph, misuse."""
import ctypes as C

import numpy as np
import pytest

import state_put_cases as pc
import state_records_cases as sc
import state_records_ref as ref
from strikeforce_amd import abi, env

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SF_ERR_ARG, SF_ERR_STATE = -1, -4
PARTS = ("hdr",) + ref.TABLES + ("cell_flags", "cell_dmg", "cell_portal")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def play(name, foreign=False, steps=None):
    """The case on the device at its step; foreign: other seeds and nine steps of the case's rows instead."""
    c = sc.case(name)
    g = env.ArenaBatch(c.w)
    if foreign:
        tb, sr = c.w.seeds(base_tb=1_600_000_000 + 77 * sc.NAMES.index(name))
        g.reset(tb, sr)
        rows = c.rows[:9]
    else:
        g.reset(c.tb, c.sr)
        rows = c.rows if steps is None else c.rows[:steps]
    cmds = dev(rows)
    g.step_device(cmds.data_ptr(), len(rows))
    g.synchronize()
    return c, g


def records(g, **kw):
    """All ten outputs of sf_state_device as host arrays."""
    x = g.state_records(cells=True, digest=True, **kw)["raw"]
    g.synchronize()
    return {n: t.cpu().numpy().copy() for n, t in x.items()}


def same_records(what, x, y, skip_episodes=True):
    for n in ref.OUTPUTS:
        a, b = x[n], y[n]
        if n == "hdr" and skip_episodes:
            a, b = a.copy(), b.copy()
            a[:, 18:20] = 0
            b[:, 18:20] = 0
        assert np.array_equal(a, b), (what, n, np.argwhere(a != b)[:4].tolist())


def oracle_records(name):
    """The oracle's dumps of the case as the raw record tensors put_state takes, on the device."""
    arrs = [ref.arena_arrays(d) for d in sc.oracle_dumps(name)[0]]
    return {n: dev(np.stack([a[n] for a in arrs])) for n in PARTS}, arrs


def episodes(g):
    return g.state_records(humans=0, zombies=0, bullets=0, portals=0)["hdr"]["episodes"].cpu().numpy().copy()


@pytest.mark.parametrize("name", sc.NAMES)
def test_round_trip_and_continuation(name):
    c, a = play(name)
    _, b = play(name, foreign=True)
    try:
        src = a.state_records(cells=True, digest=True)["raw"]
        st, sel = b.put_state({n: src[n] for n in PARTS}, selected=True)
        assert st.cpu().tolist() == [0] * c.w.cfg.arenas and bool((sel == 1).all())
        xa, xb = records(a), records(b)
        same_records(name, xa, xb)
        assert np.array_equal(xb["digest"].view(np.uint64), b.digest()) and np.array_equal(a.digest(), b.digest())
        assert not np.array(b.done()).any() or not c.w.cfg.auto_reset  # the restart flag of a written arena is cleared
        assert np.array(b.phase_draws()).sum() == 0
        gap = episodes(a) - episodes(b)
        rows = pc.continuation(name)
        cmds = dev(rows)
        for s in range(len(rows)):
            a.step_device(cmds[s].data_ptr(), 1), b.step_device(cmds[s].data_ptr(), 1)
            da, db = a.digest_device().cpu().numpy(), b.digest_device().cpu().numpy()
            assert np.array_equal(da, db), (name, s, np.argwhere(da != db)[:4].tolist())
            if s in (0, len(rows) // 2, len(rows) - 1):
                assert np.array_equal(a.observe().view(np.int32), b.observe().view(np.int32)), (name, s)
                assert np.array_equal(a.action_mask_host(), b.action_mask_host()), (name, s)
        assert np.array_equal(a.done(), b.done())
        if name == "tiny":  # games ended on the way: the latch holds a later game's record in both
            assert (episodes(a) - gap - episodes(b) == 0).all() and (episodes(b) >= 2).all()
            assert np.array_equal(a.results(), b.results())
        assert np.array_equal(episodes(a) - episodes(b), gap)
    finally:
        a.close(), b.close()


@pytest.mark.parametrize("name", sc.NAMES)
def test_import_from_the_oracle(name):
    _, b = play(name, foreign=True)
    try:
        recs, arrs = oracle_records(name)
        A = b.cfg.arenas
        assert b.put_state(recs).cpu().tolist() == [0] * A
        dig, eps, done, results, _ = pc.oracle_continuation(name)
        assert np.array_equal(b.digest(), dig[0]) and np.array_equal(b.digest(), sc.oracle_dumps(name)[1])
        # one arena once more through the host mirror, over foreign state again
        last = A - 1
        b.reset_arenas(mask_ptr=dev(np.array([0] * last + [1], dtype=np.uint8)).data_ptr())
        d = sc.oracle_dumps(name)[0][last]
        H, Z, B, P = b.cfg.cap_humans, b.cfg.cap_zombies, b.cfg.cap_bullets, b.cfg.cap_portals
        b.load_arena(last, d.hdr, (abi.HumanRec * H)(*d.humans), (abi.ZombieRec * Z)(*d.zombies), (abi.BulletRec * B)(*d.bullets),
                     (abi.PortalRec * P)(*d.portals), d.flags, d.dmg, d.pidx)
        assert np.array_equal(b.digest(), dig[0])
        rows = pc.continuation(name)
        cmds = dev(rows)
        for s in range(len(rows)):
            b.step_device(cmds[s].data_ptr(), 1)
            got = b.digest_device().cpu().numpy().view(np.uint64)
            assert np.array_equal(got, dig[s + 1]), (name, s, np.argwhere(got != dig[s + 1])[:4].tolist())
        assert np.array_equal(np.array(b.done()).reshape(-1)[:A] != 0, done != 0) or b.cfg.auto_reset
        if (eps[1] > eps[0]).any():
            ended = eps[1] > eps[0]
            assert np.array_equal(np.array(b.results())[ended], results[ended])
    finally:
        b.close()


def snapshot_blobs(g, arenas):
    s = g.snapshot(len(arenas))
    try:
        m = np.full(g.cfg.arenas, -1, dtype=np.int32)
        m[arenas] = np.arange(len(arenas))
        s.save(m)
        return [bytes(s.export(i)) for i in range(len(arenas))]
    finally:
        s.close()


def test_fork_and_untouched_arenas():
    name = "mid"
    _, b = play(name, foreign=True)
    try:
        recs, arrs = oracle_records(name)
        A = b.cfg.arenas
        rows3 = {n: t[[5, 17, 64]].contiguous() for n, t in recs.items()}
        rmap = np.array([(i % 3) if i % 5 else -1 for i in range(A)], dtype=np.int32)
        rmap[[7, 11, 13]] = [3, -2, 2**31 - 1]  # out of range: never an address
        named, quiet = np.nonzero((rmap >= 0) & (rmap < 3))[0], np.nonzero((rmap < 0) | (rmap >= 3))[0]
        before, blobs = records(b), snapshot_blobs(b, quiet)
        b.put_status()
        guard = torch.full((A + 32,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        gsel = torch.full((A * b.cfg.n_agents + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        io, keep = b.state_put_io(rows3, dev(rmap), status=False)
        io.d_status, io.d_selected = guard[16:].data_ptr(), gsel[32:].data_ptr()
        b.state_put_device(io)
        after = records(b)
        src = [5, 17, 64]
        want = ref.expected(arrs, [src[rmap[i]] for i in named], (b.cfg.cap_humans, b.cfg.cap_zombies, b.cfg.cap_bullets, b.cfg.cap_portals),
                            sc.oracle_dumps(name)[1])
        same_records("named", {n: after[n][named] for n in ref.OUTPUTS},
                     {n: (want[n].view(after[n].dtype) if n == "digest" else want[n]) for n in ref.OUTPUTS})
        same_records("quiet", {n: after[n][quiet] for n in ref.OUTPUTS}, {n: before[n][quiet] for n in ref.OUTPUTS}, skip_episodes=False)
        assert snapshot_blobs(b, quiet) == blobs
        st = guard.cpu().numpy()
        assert (st[:16] == 0x5A5A5A5A).all() and (st[16 + A:] == 0x5A5A5A5A).all()
        exp = np.where(rmap == -1, -1, np.where((rmap < -1) | (rmap >= 3), abi.PUT_BAD_ROW, 0))
        assert np.array_equal(st[16:16 + A], exp)
        se = gsel.cpu().numpy()
        assert (se[:32] == 0xA5).all() and (se[32 + A * b.cfg.n_agents:] == 0xA5).all()
        assert np.array_equal(se[32:32 + A * b.cfg.n_agents].reshape(A, -1), np.repeat((exp == 0)[:, None], b.cfg.n_agents, 1).astype(np.uint8))
        assert b.put_status() == {"written": len(named), "refused": 0, "row_out_of_range": 3, "reserved": 0}
        assert b.put_status()["written"] == 0  # cleared
    finally:
        b.close()


@pytest.mark.parametrize("name", ["mid", "large"])
def test_cuts_and_parts(name):
    c, b = play(name, foreign=True)
    try:
        recs, arrs = oracle_records(name)
        caps = (b.cfg.cap_humans, b.cfg.cap_zombies, b.cfg.cap_bullets, b.cfg.cap_portals)
        A = b.cfg.arenas
        rows = pc.continuation(name)[:1]
        seen = set()
        for n in (0, 1, 63, 64, 65, None):
            cuts = tuple(cap if n is None else min(n, cap) for cap in caps)
            if cuts in seen:
                continue
            seen.add(cuts)
            part = dict(recs)
            for t, k in zip(ref.TABLES, cuts):
                # (a table of 0 slots is still given: its whole pool becomes empty)
                part[t] = recs[t][:, :k].contiguous() if k else torch.zeros((A, 0, ref.WORDS[t]), dtype=torch.int32, device="cuda")
            # four bytes off a 16-byte boundary: the dword head and tail of the coalesced loads
            for t in ref.TABLES:
                flat = torch.zeros(part[t].numel() + 4, dtype=torch.int32, device="cuda")
                flat[1:1 + part[t].numel()] = part[t].reshape(-1)
                part[t] = flat[1:1 + part[t].numel()].view(part[t].shape)
                assert part[t].data_ptr() % 16 == 4 or part[t].numel() == 0
            assert b.put_state(part).cpu().tolist() == [0] * A
            got = records(b)
            cutarrs = []
            for a in arrs:
                z = dict(a)
                for t, k in zip(ref.TABLES, cuts):
                    z[t] = a[t].copy()
                    z[t][k:] = 0
                z["counts"] = ref.counts_of(z)
                cutarrs.append(z)
            want = ref.expected(cutarrs, range(A), caps, np.array([ref.digest_of(z) for z in cutarrs], dtype=np.uint64))
            same_records((name, cuts), got, {m: (want[m].view(got[m].dtype) if m == "digest" else want[m]) for m in ref.OUTPUTS})
            # one more step plays: the extents and the derived scalars hold (the oracle cannot load a state: determinism
            # against a second put of the same records is what is left to compare)
            cmd = dev(rows)
            b.step_device(cmd.data_ptr(), 1)
            first = b.digest()
            assert b.put_state(part).cpu().tolist() == [0] * A
            b.step_device(cmd.data_ptr(), 1)
            assert np.array_equal(b.digest(), first)
        # each part alone: the others bit for bit as before
        groups = [("hdr",)] + [(t,) for t in ref.TABLES] + [("cell_flags", "cell_dmg", "cell_portal")]
        for grp in groups:
            _, f = play(name, foreign=True)
            try:
                before = records(f)
                assert f.put_state({n: recs[n] for n in grp}).cpu().tolist() == [0] * A
                after = records(f)
                full = ref.expected(arrs, range(A), caps)
                for n in PARTS:
                    e = full[n] if n in grp else before[n]
                    g_, e_ = after[n], e
                    if n == "hdr":
                        g_, e_ = g_.copy(), e_.copy()
                        g_[:, 18:20] = 0
                        e_[:, 18:20] = 0
                    assert np.array_equal(g_, e_), (name, grp, n)
            finally:
                f.close()
    finally:
        b.close()


def bad_rows(cfg, arrs):
    """(part, bit, editor) — one field at its first bad value each."""
    F, N, M, H, P = cfg.floors, cfg.rows, cfg.cols, cfg.cap_humans, cfg.cap_portals
    h = int(np.nonzero(arrs[0]["humans"][:, 0])[0][0])
    z = bu = po = 0  # slot 0 gets a whole good record first, then the one bad field
    BASE = {"zombies": [1, 0, 1, 1, 100, 0, 0], "bullets": [1, 0, 1, 1, 1, 0, 5, 0, 10, 0, 0], "portals": [1, 0, 1, 1]}
    HB, ZB, BB, PB, CB, XB = (abi.PUT_BAD_HUMAN, abi.PUT_BAD_ZOMBIE, abi.PUT_BAD_BULLET, abi.PUT_BAD_PORTAL, abi.PUT_BAD_CELL,
                              abi.PUT_BAD_HDR)

    def s(t, i, w, v):
        def edit(x):
            if t in BASE:
                x[i] = BASE[t]
            x[i, w] = v
        return t, edit

    out = [(HB,) + s("humans", h, 4, F), (HB,) + s("humans", h, 5, N), (HB,) + s("humans", h, 6, M), (HB,) + s("humans", h, 6, -1),
           (HB,) + s("humans", h, 7, 5), (HB,) + s("humans", h, 7, 0), (HB,) + s("humans", h, 3, 2), (HB,) + s("humans", h, 0, 2),
           (HB,) + s("humans", h, 8, 256), (HB,) + s("humans", h, 15, 3), (HB,) + s("humans", h, 15, -2), (HB,) + s("humans", h, 16, 15),
           (HB,) + s("humans", h, 17, 65536), (HB,) + s("humans", h, 24, -1), (HB,) + s("humans", h, 25, 256), (HB,) + s("humans", h, 26, 256),
           (HB,) + s("humans", h, 27, P), (HB,) + s("humans", h, 27, -2),
           (ZB,) + s("zombies", z, 1, F), (ZB,) + s("zombies", z, 3, M), (ZB,) + s("zombies", z, 0, 2), (ZB,) + s("zombies", z, 6, 2),
           (BB,) + s("bullets", bu, 2, N), (BB,) + s("bullets", bu, 4, 0), (BB,) + s("bullets", bu, 4, 5), (BB,) + s("bullets", bu, 5, 65536),
           (BB,) + s("bullets", bu, 7, 32768), (BB,) + s("bullets", bu, 7, -32769), (BB,) + s("bullets", bu, 8, -1),
           (BB,) + s("bullets", bu, 9, H + 1), (BB,) + s("bullets", bu, 10, 2),
           (PB,) + s("portals", po, 1, F), (PB,) + s("portals", po, 0, -1), (PB,) + s("portals", po, 3, M),
           (XB, "hdr", lambda x: x.__setitem__(20, 65537)), (XB, "hdr", lambda x: x.__setitem__(37, -1)),
           (XB, "hdr", lambda x: x.__setitem__(10, 1041)), (XB, "hdr", lambda x: x.__setitem__(11, 1)),
           (XB, "hdr", lambda x: x.__setitem__(38, 2)), (XB, "hdr", lambda x: x.__setitem__(39, 7)),
           (XB, "hdr", lambda x: x.__setitem__(17, -1)), (XB, "hdr", lambda x: x.__setitem__(1, -1)),
           (XB, "hdr", lambda x: x.__setitem__(3, 1)),
           (CB, "cell_flags", lambda x: x.__setitem__(0, 0x40)), (CB, "cell_portal", lambda x: x.__setitem__(0, 0)),
           (CB, "cell_dmg", lambda x: x.__setitem__(0, 1))]
    return out


def test_refusals_beside_good_rows():
    name = "mid"
    _, b = play(name, foreign=True)
    try:
        _, arrs = oracle_records(name)
        cfg = b.cfg
        A = cfg.arenas
        # vec 2 with the weapon table's first index out of range, and a vec -1 that keeps any ind
        bad = bad_rows(cfg, arrs)
        h = int(np.nonzero(arrs[0]["humans"][:, 0])[0][0])
        bad.append((abi.PUT_BAD_HUMAN, "humans", lambda x: (x.__setitem__((h, 15), 2), x.__setitem__((h, 16), 8))))
        bad.append((abi.PUT_BAD_HUMAN, "humans", lambda x: (x.__setitem__((h, 15), 0), x.__setitem__((h, 16), 4))))
        bad.append((abi.PUT_BAD_HUMAN, "humans", lambda x: (x.__setitem__((h, 15), 1), x.__setitem__((h, 16), -1))))
        assert arrs[0]["cell_flags"][0] in (0, 1) and arrs[0]["cell_portal"][0] == -1 and arrs[0]["cell_dmg"][0] == 0
        # a player-built entrance with an exit number at the cap, a map entrance with another number than the map's
        bad.append((abi.PUT_BAD_CELL, "cell_flags", lambda x: x.__setitem__(0, 0x02 | 0x04)))  # (cell_portal -1 stays)
        good = dict((n, arrs[1][n].copy()) for n in PARTS)
        good["humans"][h, 15], good["humans"][h, 16] = -1, 14  # last good values ride in the good rows
        rows_np = {n: [] for n in PARTS}
        bits = []
        for k, (bit, part, edit) in enumerate(bad):
            row = {n: arrs[0][n].copy() for n in PARTS}
            edit(row[part])
            for n in PARTS:
                rows_np[n].append(row[n])
            bits.append(bit)
        for n in PARTS:
            rows_np[n].append(good[n])
        R = len(bits) + 1
        assert R <= A
        recs = {n: dev(np.stack(v)) for n, v in rows_np.items()}
        rmap = np.arange(A, dtype=np.int32)
        rmap[R:] = R - 1  # everybody else forks the good row
        before = records(b)
        b.put_status()
        st = b.put_state(recs, dev(rmap)).cpu().numpy()
        assert st[:R - 1].tolist() == bits and (st[R - 1:] == 0).all(), [(i, int(x), y) for i, (x, y) in enumerate(zip(st[:R - 1], bits)) if x != y]
        after = records(b)
        refused = np.arange(R - 1)
        same_records("refused rows' arenas", {n: after[n][refused] for n in ref.OUTPUTS}, {n: before[n][refused] for n in ref.OUTPUTS}, False)
        z = dict(good)
        z["counts"] = ref.counts_of(z)
        for a in (R - 1, A - 1):
            for n in PARTS:
                e, g_ = z[n], after[n][a]
                if n == "hdr":
                    e, g_ = e.copy(), g_.copy()
                    e[18:20] = 0
                    g_[18:20] = 0
                assert np.array_equal(g_, e), (a, n)
        assert b.put_status() == {"written": A - (R - 1), "refused": R - 1, "row_out_of_range": 0, "reserved": 0}
        # the host mirror names the reason
        d = sc.oracle_dumps(name)[0][0]
        hs = (abi.HumanRec * cfg.cap_humans)(*d.humans)
        hs[h].way = 5
        rc = b.L.sf_load_arena(b.h, 0, None, C.addressof(hs), None, None, None, None, None, None)
        assert rc == SF_ERR_ARG and b"a human" in b.L.sf_last_error()
        hs[h].way = d.humans[h].way
        assert b.L.sf_load_arena(b.h, 0, None, C.addressof(hs), None, None, None, None, None, None) == 0
    finally:
        b.close()


def test_captured_with_a_step_launch_and_replayed_three_times():
    name = "battle"
    c = sc.case(name)
    recs, _ = oracle_records(name)
    g, eager = env.ArenaBatch(c.w), env.ArenaBatch(sc.case(name).w)
    try:
        stream = torch.cuda.Stream()
        g.set_stream(stream.cuda_stream)
        g.reset(c.tb, c.sr), eager.reset(c.tb, c.sr)
        cmds = dev(pc.continuation(name)[:2])
        io, keep = g.state_put_io(recs)
        g.state_put_device(io)  # (the verdict rows are allocated outside the capture)
        g.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            g.state_put_device(io)
            g.step_device(cmds.data_ptr(), 2)
        for _ in range(3):
            with torch.cuda.stream(stream):
                graph.replay()
            stream.synchronize()
            eager.put_state(recs)
            eager.step_device(cmds.data_ptr(), 2)
            assert np.array_equal(g.digest(), eager.digest())
            assert np.array_equal(g.digest(), pc.oracle_continuation(name)[0][2])
        del graph
    finally:
        g.close(), eager.close()


def test_misuse_is_refused_with_nothing_launched():
    name = "tiny"
    c = sc.case(name)
    recs, _ = oracle_records(name)
    g = env.ArenaBatch(c.w)
    try:
        L = g.L
        io, keep = g.state_put_io(recs)
        assert L.sf_state_put_device(g.h, C.byref(io)) == SF_ERR_STATE and b"before sf_reset" in L.sf_last_error()
        g.reset(c.tb, c.sr)
        cmds = dev(c.rows[:3])
        g.step_device(cmds.data_ptr(), 3)
        before = g.digest()
        g.step_begin()
        mid = g.digest()
        assert L.sf_state_put_device(g.h, C.byref(io)) == SF_ERR_STATE and b"sf_step_begin" in L.sf_last_error()
        assert np.array_equal(g.digest(), mid)
        g.step_end(c.rows[3])
        before = g.digest()
        assert L.sf_state_put_device(None, C.byref(io)) == SF_ERR_ARG and L.sf_state_put_device(g.h, None) == SF_ERR_ARG
        assert L.sf_state_put_status(g.h, None) == SF_ERR_ARG

        def refused(word, **edits):
            io2 = abi.StatePutIO.from_buffer_copy(io)
            for f, v in edits.items():
                setattr(io2, f, v)
            assert L.sf_state_put_device(g.h, C.byref(io2)) == SF_ERR_ARG and word in L.sf_last_error(), (edits, L.sf_last_error())

        refused(b"rows", rows=0)
        refused(b"d_row_of_arena", d_row_of_arena=None)
        for f, cap in (("humans", g.cfg.cap_humans), ("zombies", g.cfg.cap_zombies), ("bullets", g.cfg.cap_bullets), ("portals", g.cfg.cap_portals)):
            refused(b"cap", **{f: -1})
            refused(b"cap", **{f: cap + 1})
        refused(b"all or none", d_cell_dmg=None)
        refused(b"all or none", d_cell_flags=None, d_cell_portal=None)
        refused(b"every part", **{p: None for p in abi.STATE_PUT_PARTS})
        host = np.zeros(4096, dtype=np.int32)
        refused(b"not device memory", d_hdr=host.ctypes.data)
        refused(b"aligned", d_zombies=io.d_zombies + 2)
        refused(b"aligned", d_hdr=io.d_hdr + 4)
        # extents are checked against the allocation: allocations of exactly the documented size (torch's tensors are
        # carved out of larger ones), one element short, and starting too late
        import test_gpu_signals as sig
        H = sig._hip()
        A = g.cfg.arenas
        sizes = {"d_row_of_arena": 4 * A, "d_hdr": 160 * io.rows, "d_humans": 112 * io.rows * io.humans, "d_cell_flags": io.rows * 63,
                 "d_cell_portal": 4 * io.rows * 63, "d_status": 4 * A, "d_selected": A * g.cfg.n_agents}
        bufs = []
        try:
            for field, nbytes in sizes.items():
                unit = {"d_hdr": 8, "d_cell_flags": 1, "d_selected": 1}.get(field, 4)
                exact, short = C.c_void_p(), C.c_void_p()
                assert H.hipMalloc(C.byref(exact), nbytes) == 0 and H.hipMalloc(C.byref(short), nbytes - unit) == 0
                bufs += [exact, short]
                refused(b"past the end", **{field: short.value})
                refused(b"past the end", **{field: exact.value + unit})
                assert field.encode() in L.sf_last_error() and b"sf_state_put_device" in L.sf_last_error()
            hdr_exact = bufs[2]
            assert H.hipMemset(hdr_exact, 0, sizes["d_hdr"]) == 0
            refused(b"past the end", d_hdr=hdr_exact.value, rows=io.rows + 1)  # one row more than the allocation holds
        finally:
            for q in bufs:
                H.hipFree(q)
        assert np.array_equal(g.digest(), before)
        assert g.put_status() == {"written": 0, "refused": 0, "row_out_of_range": 0, "reserved": 0}
        # a replay loaded
        w2 = sc.case("battle")
        r = env.ArenaBatch(w2.w)
        try:
            r.reset(w2.tb, w2.sr)
            A, n = w2.w.cfg.arenas, w2.w.cfg.n_agents
            r.replay_load([bytes(w2.rows[:4, a, :].reshape(-1)) for a in range(A)])
            recs2, _ = oracle_records("battle")
            io3, keep3 = r.state_put_io(recs2)
            assert L.sf_state_put_device(r.h, C.byref(io3)) == SF_ERR_STATE and b"replay" in L.sf_last_error()
        finally:
            r.close()
    finally:
        g.close()


def test_episode_log_and_result_latch_survive_a_put():
    name = "tiny"
    c = sc.case(name)
    g = env.ArenaBatch(c.w)
    try:
        g.enable_episode_log(8)
        g.reset(c.tb, c.sr)
        cmds = dev(c.rows)
        g.step_device(cmds.data_ptr(), len(c.rows))
        latch = np.array(g.results()).copy()
        ring = np.array(g.episode_ring()).copy()
        recs, _ = oracle_records(name)
        eps = episodes(g)
        assert (eps >= 2).all() and g.put_state(recs).cpu().tolist() == [0] * c.w.cfg.arenas
        assert np.array_equal(g.results(), latch) and np.array_equal(np.array(g.episode_ring()), ring)
        assert np.array_equal(episodes(g), eps)
        got = g.episodes()
        assert len(got[0] if isinstance(got, tuple) else got) > 0  # the pending records are still delivered
    finally:
        g.close()


def test_example_runs():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "scenario_start.py"), "--arenas", "64", "--steps", "60"],
                       capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "outcomes" in r.stdout and "written 64" in r.stdout, r.stdout[-1000:]
