"""sf_state_device on the MI355X (k_state_init, k_state_records) through the C-ABI, against the arrays tests/state_records_ref.py
builds from the oracle's dumps, bit for bit: no tolerance anywhere.

Every case of tests/state_records_cases.py is played on the device with the case's commands (one k-step launch) and kept for
the whole module: the call writes nothing of the environment.  Every output buffer has exactly the size sf_state_bytes names,
is filled with a sentinel and has guard bytes behind it.  Checked: all outputs for all arenas and for an id list with
duplicates and ids out of range; every cut in {0, 1, 63, 64, 65, cap} the cap allows; each output alone; the device digest
against sf_state_digest and the oracle's, also between sf_step_begin and sf_step_end; sf_state_digest unchanged by the calls;
a captured graph of sf_step_device + sf_state_device replayed three times against an eager run; every misuse of the contract."""
import ctypes as C

import numpy as np
import pytest

import state_records_cases as sc
import state_records_ref as ref
from oracle_lib import ArenaDump, diff_dumps
from strikeforce_amd import abi, env

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SF_ERR_ARG, SF_ERR_STATE = -1, -4
SENTINEL, GUARD = 0xA5, 64  # the byte every output holds before the call; guard bytes behind every buffer
DTYPES = {"cell_flags": np.uint8, "digest": np.uint64}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Played:
    """One case on the device, stepped to where the oracle's dumps were taken."""

    def __init__(self, name, steps=None):
        self.c = sc.case(name)
        self.cfg = self.c.w.cfg
        self.g = env.ArenaBatch(self.c.w)
        self.g.reset(self.c.tb, self.c.sr)
        rows = self.c.rows if steps is None else self.c.rows[:steps]
        self.cmds = dev(rows)
        self.g.step_device(self.cmds.data_ptr(), len(rows))
        self.g.synchronize()
        self.caps = (self.cfg.cap_humans, self.cfg.cap_zombies, self.cfg.cap_bullets, self.cfg.cap_portals)
        self.cells = self.cfg.floors * self.cfg.rows * self.cfg.cols

    def shapes(self, rows, cuts):
        s = {"hdr": (rows, 40), "cell_flags": (rows, self.cells), "cell_dmg": (rows, self.cells), "cell_portal": (rows, self.cells),
             "counts": (rows, 8), "digest": (rows,)}
        s.update({t: (rows, n, ref.WORDS[t]) for t, n in zip(ref.TABLES, cuts)})
        return s

    def io(self, ids, cuts, ptrs):
        io = abi.StateIO()
        if ids is not None:
            io.d_arena_ids, io.rows = ids.data_ptr(), ids.numel()
        io.humans, io.zombies, io.bullets, io.portals = cuts
        for n, p in ptrs.items():
            setattr(io, "d_" + n, p)
        return io

    def call(self, ids=None, cuts=None, outs=ref.OUTPUTS, expect=0):
        """One sf_state_device: the outputs `outs` as numpy arrays (guards checked), or the sentinel check after a refusal."""
        cuts = self.caps if cuts is None else cuts
        d_ids = None if ids is None else dev(np.asarray(ids, dtype=np.int32))
        rows = self.cfg.arenas if ids is None else len(ids)
        shapes = self.shapes(rows, cuts)
        sizes = dict(zip(ref.OUTPUTS, self.g.state_bytes(self.io(d_ids, cuts, {}))))
        bufs = {}
        for n in outs:
            nbytes = int(np.prod(shapes[n])) * np.dtype(DTYPES.get(n, np.int32)).itemsize
            assert sizes[n] == nbytes, (n, sizes[n], nbytes)  # what sf_state_bytes names is the documented size
            bufs[n] = torch.full((nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = self.g.L.sf_state_device(self.g.h, C.byref(self.io(d_ids, cuts, {n: b.data_ptr() for n, b in bufs.items()})))
        assert rc == expect, (rc, self.g.L.sf_last_error())
        self.g.synchronize()
        out = {}
        for n, b in bufs.items():
            h = b.cpu().numpy()
            assert (h[len(h) - GUARD:] == SENTINEL).all(), (n, "guard bytes overwritten")
            if expect:
                assert (h == SENTINEL).all(), (n, "a refused call wrote")
            out[n] = h[:len(h) - GUARD].view(DTYPES.get(n, np.int32)).reshape(shapes[n])
        return out

    def close(self):
        self.g.close()


_played = {}


@pytest.fixture(scope="module", autouse=True)
def _close_all():
    yield
    for p in _played.values():
        p.close()
    _played.clear()


def played(name):
    if name not in _played:
        _played[name] = Played(name)
    return _played[name]


def want(name, ids, cuts):
    dumps, digests = sc.oracle_dumps(name)
    A = len(dumps)
    return ref.expected([arrays(name, a) for a in range(A)], range(A) if ids is None else ids, cuts, digests)


_arrays = {}


def arrays(name, a):
    if (name, a) not in _arrays:
        _arrays[name, a] = ref.arena_arrays(sc.oracle_dumps(name)[0][a])
    return _arrays[name, a]


def same(what, got, exp):
    for n, g in got.items():
        e = exp[n]
        assert g.shape == e.shape and g.dtype == e.dtype, (what, n, g.shape, e.shape, g.dtype, e.dtype)
        if not np.array_equal(g, e):
            at = np.argwhere(g != e)
            raise AssertionError((what, n, len(at), at[:4].tolist(), g[g != e][:4].tolist(), e[g != e][:4].tolist()))


@pytest.mark.parametrize("name", sc.NAMES)
def test_every_output_of_every_arena_equals_the_reference(name):
    p = played(name)
    before = p.g.digest()
    assert np.array_equal(before, sc.oracle_dumps(name)[1])  # the device is where the oracle is
    a = p.cfg.arenas - 1
    assert diff_dumps(ArenaDump(*p.g.dump_raw(a)).as_dict(), sc.oracle_dumps(name)[0][a].as_dict()) is None
    got = p.call()
    same(name, got, want(name, None, p.caps))
    assert np.array_equal(got["digest"], before) and np.array_equal(p.g.digest(), before)  # bit for bit, and nothing changed


@pytest.mark.parametrize("name", sc.NAMES)
def test_id_list_with_duplicates_and_ids_out_of_range(name):
    p = played(name)
    A = p.cfg.arenas
    ids = [A - 1, 0, 0, -1, A, 2 % A, 2**31 - 1, -2**31, A - 1] + list(range(A))[::-1]
    same(name, p.call(ids=ids), want(name, ids, p.caps))
    one = [A // 2]
    same(name + ", one row", p.call(ids=one), want(name, one, p.caps))


@pytest.mark.parametrize("name", sc.NAMES)
def test_every_cut_the_caps_allow(name):
    p = played(name)
    ids = [0, -1, p.cfg.arenas - 1]
    seen = set()
    for n in (0, 1, 63, 64, 65, None):
        cuts = tuple(cap if n is None else min(n, cap) for cap in p.caps)
        if cuts in seen:
            continue
        seen.add(cuts)
        outs = ref.TABLES + ("counts", "digest")
        e = want(name, None, cuts)
        same((name, cuts), p.call(cuts=cuts, outs=outs), {k: e[k] for k in outs})
        e = want(name, ids, cuts)
        same((name, cuts, "ids"), p.call(ids=ids, cuts=cuts, outs=ref.TABLES), {k: e[k] for k in ref.TABLES})
    for t, cap in enumerate(p.caps):  # one table cut alone, the others whole
        cuts = tuple(cap - 1 if j == t else c for j, c in enumerate(p.caps))
        e = want(name, None, cuts)
        same((name, cuts), p.call(cuts=cuts, outs=ref.TABLES), {k: e[k] for k in ref.TABLES})


@pytest.mark.parametrize("name", sc.NAMES)
def test_each_output_alone(name):
    p = played(name)
    e = want(name, None, p.caps)
    for n in ref.OUTPUTS:
        same((name, "only " + n), p.call(outs=(n,)), {n: e[n]})
    ids = [p.cfg.arenas - 1, p.cfg.arenas, 0]
    e = want(name, ids, p.caps)
    for n in ("counts", "digest", "cell_portal"):
        same((name, "ids, only " + n), p.call(ids=ids, outs=(n,)), {n: e[n]})
    assert p.g.L.sf_state_device(p.g.h, C.byref(p.io(None, p.caps, {}))) == 0  # all outputs NULL: nothing to do


@pytest.mark.parametrize("name", ["tiny", "battle"])
def test_between_the_halves_of_a_step(name):
    p = Played(name, steps=len(sc.case(name).rows) - 1)
    try:
        p.g.step_begin()
        host = p.g.digest()
        got = p.call()
        assert np.array_equal(got["digest"], host)
        for a in range(p.cfg.arenas):
            arr = ref.arena_arrays(ArenaDump(*p.g.dump_raw(a)))
            for n in ("hdr",) + ref.TABLES + ("cell_flags", "cell_dmg", "cell_portal", "counts"):
                assert np.array_equal(got[n][a], arr[n]), (name, a, n)
        assert np.array_equal(p.g.digest(), host)
        p.g.step_end(p.c.rows[-1])
        same(name, p.call(), want(name, None, p.caps))  # and the step ends where the oracle's whole step does
    finally:
        p.close()


def test_python_surface():
    p = played("battle")
    x = p.g.state_records(cells=True, digest=True)
    e = want("battle", None, p.caps)
    for n, t in x["raw"].items():
        h = t.cpu().numpy()
        assert np.array_equal(h.view(np.uint64) if n == "digest" else h, e[n]), n
    d = sc.oracle_dumps("battle")[0][2]
    assert x["humans"]["hp"][2].cpu().tolist() == [h.hp for h in d.humans] and x["hdr"]["tb"][2].item() == d.hdr.tb
    assert x["counts"]["zombies_alive"][2].item() == sum(z.alive for z in d.zombies)
    again = p.g.state_records(cells=True, digest=True)
    assert again["raw"]["hdr"].data_ptr() == x["raw"]["hdr"].data_ptr()  # allocated once per shape of request
    ids = torch.tensor([2, 2, 7], dtype=torch.int32, device="cuda")
    y = p.g.state_records(arena_ids=ids, zombies=1, bullets=0, hdr=False)
    assert set(y["raw"]) == {"humans", "zombies", "portals", "counts"} and y["raw"]["zombies"].shape == (3, 1, 7)
    assert y["counts"]["humans_alive"].cpu().tolist() == [int(e["counts"][2, 0])] * 2 + [-1]
    assert np.array_equal(p.g.digest_device().cpu().numpy().view(np.uint64), p.g.digest())


def test_captured_behind_a_step_launch_and_replayed_three_times():
    name, k = "battle", 2
    c = sc.case(name)
    A, n = c.w.cfg.arenas, c.w.cfg.n_agents
    g, eager = env.ArenaBatch(c.w), env.ArenaBatch(sc.case(name).w)
    stream = torch.cuda.Stream()
    g.set_stream(stream.cuda_stream)
    g.reset(c.tb, c.sr), eager.reset(c.tb, c.sr)
    cmds = dev(c.rows[:k])
    outs = lambda: {"hdr": torch.zeros((A, 40), dtype=torch.int32, device="cuda"),
                    "humans": torch.zeros((A, c.w.cfg.cap_humans, 28), dtype=torch.int32, device="cuda"),
                    "bullets": torch.zeros((A, 5, 11), dtype=torch.int32, device="cuda"),
                    "cell_portal": torch.zeros((A, 64 * 64), dtype=torch.int32, device="cuda"),
                    "counts": torch.zeros((A, 8), dtype=torch.int32, device="cuda"),
                    "digest": torch.zeros((A,), dtype=torch.int64, device="cuda")}

    def io_of(bufs):
        io = abi.StateIO()
        io.humans, io.bullets = c.w.cfg.cap_humans, 5
        for m, t in bufs.items():
            setattr(io, "d_" + m, t.data_ptr())
        return io

    mine, theirs = outs(), outs()
    torch.cuda.synchronize()
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            g.step_device(cmds.data_ptr(), k)
            g.state_device(io_of(mine))
        torch.cuda.synchronize()
        assert np.array_equal(g.digest(), eager.digest())  # (capture launched nothing)
        for i in range(3):
            with torch.cuda.stream(stream):
                graph.replay()
            stream.synchronize()
            eager.step_device(cmds.data_ptr(), k)
            eager.state_device(io_of(theirs))
            eager.synchronize()
            for m in mine:
                assert torch.equal(mine[m], theirs[m]), (i, m)
            assert np.array_equal(mine["digest"].cpu().numpy().view(np.uint64), g.digest()), i
            assert mine["hdr"].cpu().numpy()[:, 16].tolist() == [k * (i + 1)] * A  # steps: the replays do step
    finally:
        g.close(), eager.close()


def test_refusals_by_state_and_argument():
    c = sc.case("tiny")
    g = env.ArenaBatch(c.w)
    L, A = g.L, c.w.cfg.arenas
    out = torch.full((A * 8 + 2,), -7, dtype=torch.int32, device="cuda")
    io = abi.StateIO()
    io.d_counts = out.data_ptr()
    sizes = (C.c_int64 * 10)()
    try:
        assert L.sf_state_device(g.h, C.byref(io)) == SF_ERR_STATE and b"before sf_reset" in L.sf_last_error()
        assert L.sf_state_bytes(g.h, C.byref(io), C.byref(sizes)) == SF_ERR_STATE
        g.reset(c.tb, c.sr)
        assert L.sf_state_device(None, C.byref(io)) == SF_ERR_ARG and L.sf_state_device(g.h, None) == SF_ERR_ARG
        assert L.sf_state_bytes(g.h, C.byref(io), None) == SF_ERR_ARG and L.sf_state_bytes(None, C.byref(io), C.byref(sizes)) == SF_ERR_ARG
        import test_gpu_signals as sig  # (its hipMalloc: an allocation of exactly four ids, for the extent check)
        H, q = sig._hip(), C.c_void_p()
        assert H.hipMalloc(C.byref(q), 16) == 0 and H.hipMemset(q, 0, 16) == 0
        for field, bad in (("humans", -1), ("humans", 9), ("zombies", 25), ("bullets", 65), ("portals", 17), ("portals", -2**31)):
            io2 = abi.StateIO()
            io2.d_counts = out.data_ptr()
            setattr(io2, field, bad)
            assert L.sf_state_device(g.h, C.byref(io2)) == SF_ERR_ARG and b"cap" in L.sf_last_error(), (field, bad)
        for rows in (0, -1):
            io2 = abi.StateIO()
            io2.d_counts, io2.d_arena_ids, io2.rows = out.data_ptr(), q.value, rows
            assert L.sf_state_device(g.h, C.byref(io2)) == SF_ERR_ARG and b"rows" in L.sf_last_error()
        host = np.zeros(64, dtype=np.int32)
        io2 = abi.StateIO()
        io2.d_counts, io2.d_arena_ids, io2.rows = out.data_ptr(), host.ctypes.data, 4
        assert L.sf_state_device(g.h, C.byref(io2)) == SF_ERR_ARG and b"d_arena_ids" in L.sf_last_error()
        io2.d_arena_ids, io2.rows = q.value, 5  # one id more than the allocation holds
        assert L.sf_state_device(g.h, C.byref(io2)) == SF_ERR_ARG and b"past the end" in L.sf_last_error()
        io2.d_arena_ids = q.value + 2
        assert L.sf_state_device(g.h, C.byref(io2)) == SF_ERR_ARG and b"aligned" in L.sf_last_error()
        g.synchronize()
        assert (out.cpu().numpy() == -7).all()  # nothing was launched by any of them
        assert L.sf_state_device(g.h, C.byref(io)) == 0
        g.synchronize()
        h = out.cpu().numpy()
        assert (h[:A * 8] != -7).all() and (h[A * 8:] == -7).all()
        H.hipFree(q)
    finally:
        g.close()


def test_host_pointers_misaligned_and_short_buffers_are_refused_before_any_launch():
    import test_gpu_signals as sig  # (its hipMalloc: allocations of their own, the extent check is made against them)
    p = played("tiny")
    L, A = p.g.L, p.cfg.arenas
    H, bufs = sig._hip(), []
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def alloc(nbytes):
        q = C.c_void_p()
        assert H.hipMalloc(C.byref(q), nbytes) == 0 and H.hipMemset(q, SENTINEL, nbytes) == 0
        bufs.append((q, nbytes))
        return q.value

    sizes = dict(zip(abi.STATE_OUTPUTS, p.g.state_bytes(p.io(None, p.caps, {}))))
    align = {"d_hdr": 8, "d_digest": 8, "d_cell_flags": 1}
    host = np.zeros(max(sizes.values()) + 64, dtype=np.uint8)
    exact = {}
    try:
        for field, nbytes in sizes.items():
            unit = align.get(field, 4)
            exact[field], short, big = alloc(nbytes), alloc(nbytes - unit), alloc(nbytes + 64)

            def call(q):
                io = p.io(None, p.caps, {})
                setattr(io, field, q)
                return L.sf_state_device(p.g.h, C.byref(io))

            assert call(host.ctypes.data) == SF_ERR_ARG and b"not device memory" in L.sf_last_error(), field
            assert field.encode() in L.sf_last_error() and b"sf_state_device" in L.sf_last_error()
            assert call(short) == SF_ERR_ARG and b"past the end" in L.sf_last_error(), field  # one element short
            assert call(big + 64 + unit) == SF_ERR_ARG and b"past the end" in L.sf_last_error(), field  # starts too late
            if unit > 1:
                assert call(big + unit // 2) == SF_ERR_ARG and b"aligned" in L.sf_last_error(), field
        torch.cuda.synchronize()
        back = np.zeros(max(sizes.values()) + 64, dtype=np.uint8)
        for q, nbytes in bufs:  # no refused call had launched
            assert H.hipMemcpy(back.ctypes.data, q, nbytes, 2) == 0 and (back[:nbytes] == SENTINEL).all()
        # the exact extents, each ending on its allocation's last byte, at the least alignment the contract asks for
        io = p.io(None, p.caps, {})
        for field in sizes:
            setattr(io, field, exact[field])
        assert L.sf_state_device(p.g.h, C.byref(io)) == 0
        p.g.synchronize()
        e = want("tiny", None, p.caps)
        for field, nbytes in sizes.items():
            assert H.hipMemcpy(back.ctypes.data, exact[field], nbytes, 2) == 0
            n = field[2:]
            assert np.array_equal(back[:nbytes].view(DTYPES.get(n, np.int32)).reshape(e[n].shape), e[n]), field
        # bases that are 4- but not 16-byte aligned: the head and tail dwords of the 16-byte stores
        odd = {n: torch.full((sizes["d_" + n] + 16 + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda") for n in ref.TABLES}
        for shift in (4, 8, 12):
            io = p.io(None, p.caps, {n: t.data_ptr() + shift for n, t in odd.items()})
            assert L.sf_state_device(p.g.h, C.byref(io)) == 0
            p.g.synchronize()
            for n, t in odd.items():
                h, nbytes = t.cpu().numpy(), sizes["d_" + n]
                assert np.array_equal(h[shift:shift + nbytes].view(np.int32).reshape(e[n].shape), e[n]), (n, shift)
                assert (h[:shift] == SENTINEL).all() and (h[shift + nbytes:] == SENTINEL).all(), (n, shift)
                t.fill_(SENTINEL)
    finally:
        for q, _ in bufs:
            H.hipFree(q)


def test_the_examples_nearest_enemy_and_its_loop():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "custom_observation.py")
    spec = importlib.util.spec_from_file_location("custom_observation", path)
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    for name in ("mid", "large"):
        p = played(name)
        n = p.cfg.n_agents
        got = ex.nearest_enemy(p.g.state_records(bullets=0, portals=0, hdr=False), n).cpu().numpy()
        for a, d in enumerate(sc.oracle_dumps(name)[0]):
            for g in range(n):
                me = d.humans[g]
                foes = [z for z in d.zombies if z.alive] + [h for h in d.humans if h.alive and h.team != me.team]
                dist = [abs(me.r - o.r) + abs(me.c - o.c) + 60 * (me.f != o.f) + 5 * abs(me.f - o.f) for o in foes]
                assert got[a, g] == (min(dist) if me.alive and dist else ex.FAR), (name, a, g)
    order, dist, closest = ex.run(2, 3, 2)
    assert order.shape == (2, 9) and sorted(order[0].tolist()) == list(range(9)) and dist.shape == (2, 9) and closest.shape == (18, 1)
    assert (closest <= np.minimum(dist.reshape(18, 1), ex.FAR)).all()
