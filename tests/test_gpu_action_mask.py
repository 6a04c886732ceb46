"""sf_action_mask_device on the MI355X (k_action_mask) through the C-ABI against the truth, bit for bit: the product's own obey
run on the CPU over the oracle's dump of the same moment (tests/action_mask/mask_main.cpp, the plain build).

Every case of tests/action_mask_cases.py is played on the device with the case's commands; after each of its last few steps
the mask is taken into sentinel-filled buffers of exact size with guard bytes behind them: the command words alone, the action
words alone for three action strings ("+xzqeawsd", the full table, 32 characters with repeats), and both together; the state
digests are unchanged by the calls.  The shapes: 1 / 3 / 65 arenas, 1 / 2 / 16 agents, 1 and 64 human slots, 64 and 65 zombie
slots, 64 and 65 exits, 64 / 65 / 256 bullet slots, a flag plane that stays in HBM and planes that do not, three floors.  Then
the mask between sf_step_begin and sf_step_end, the Python surface, the call captured in a graph behind sf_step_device, and the
refusals, which leave the sentinels in place."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import action_mask_cases as mc
from oracle_lib import Oracle
from strikeforce_amd import abi, env

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SF_ERR_ARG, SF_ERR_STATE = -1, -4
GUARD = 64
STRINGS = ("+xzqeawsd", mc.COMMANDS, "__+xzqeawsd[]uu3fghjkl;'cvbnm,./")


def sentinel(n):
    """n words of 0xA5A5A5A5 with GUARD bytes of the same behind them."""
    return torch.full((4 * n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")


def words(buf, A, n):
    raw = buf.cpu().numpy()
    assert (raw[4 * A * n:] == 0xA5).all(), "guard bytes overwritten"
    return raw[:4 * A * n].view(np.uint32).reshape(A, n)


def actions_of(commands, string):
    out = np.zeros_like(commands)
    for j, ch in enumerate(string):
        out |= ((commands >> np.uint32(mc.COMMANDS.index(ch))) & np.uint32(1)) << np.uint32(j)
    return out


def check_every_request(g, want, where):
    A, n = want.shape
    before = g.digest()
    cm = sentinel(A * n)
    g.action_mask_device(commands_ptr=cm.data_ptr())
    g.synchronize()
    got = words(cm, A, n)
    assert np.array_equal(got, want), (where, np.argwhere(got != want)[:4].tolist(), [hex(x) for x in got.reshape(-1)[:4]],
                                       [hex(x) for x in want.reshape(-1)[:4]])
    for s in STRINGS:
        ac, cm2, ac2 = sentinel(A * n), sentinel(A * n), sentinel(A * n)
        g.action_mask_device(action_string=s, actions_ptr=ac.data_ptr())
        g.action_mask_device(cm2.data_ptr(), s, ac2.data_ptr())
        g.synchronize()
        assert np.array_equal(words(ac, A, n), actions_of(want, s)), (where, s)
        assert np.array_equal(words(cm2, A, n), want) and np.array_equal(words(ac2, A, n), actions_of(want, s)), (where, s)
    assert np.array_equal(g.action_mask_host(), want), where
    assert (g.digest() == before).all(), where


@pytest.mark.parametrize("name", mc.NAMES + mc.SHAPE_NAMES)
def test_device_mask_equals_the_truth(name):
    c = mc.case(name)
    want = {k: tr for k, _, tr in mc.oracle_moments(name)}
    g = env.ArenaBatch(c.w)
    try:
        g.reset(c.tb, c.sr)
        for k in range(len(c.rows) + 1):
            if k:
                g.step(c.rows[k - 1])
            if k in want:
                check_every_request(g, want[k], (name, k))
        assert want
    finally:
        g.close()


def test_the_shapes_the_issue_names():
    cfgs = [mc.case(n).w.cfg for n in mc.NAMES + mc.SHAPE_NAMES]
    has = lambda f: sorted({f(c) for c in cfgs})
    assert {1, 3, 65} <= set(has(lambda c: c.arenas)) and {1, 2, 16} <= set(has(lambda c: c.n_agents))
    assert {1, 64} <= set(has(lambda c: c.cap_humans)) and {64, 65} <= set(has(lambda c: c.cap_zombies))
    assert {64, 65} <= set(has(lambda c: c.cap_portals)) and {64, 65, 256} <= set(has(lambda c: c.cap_bullets))
    assert any(c.floors == 1 and c.rows == 128 and c.cols == 128 for c in cfgs) and any(c.floors == 3 for c in cfgs)


def test_between_step_begin_and_step_end():
    c = mc.case("battle2")
    o, g = Oracle(c.w), env.ArenaBatch(c.w)
    try:
        o.reset(c.tb, c.sr), g.reset(c.tb, c.sr)
        for row in c.rows[:-1]:
            o.step(row), g.step(row)
        o.step_begin(), g.step_begin()
        want = mc.truth([o.dump(a) for a in range(c.w.cfg.arenas)], c.w)
        check_every_request(g, want, "between the halves")
        o.step_end(c.rows[-1]), g.step_end(c.rows[-1])
        assert (o.digest() == g.digest()).all()
        check_every_request(g, mc.oracle_moments("battle2")[-1][2], "behind the second half")
    finally:
        o.close(), g.close()


def test_python_surface_owns_its_tensors():
    c = mc.case("battle16")
    g = env.ArenaBatch(c.w)
    try:
        g.reset(c.tb, c.sr)
        for row in c.rows:
            g.step(row)
        want = mc.oracle_moments("battle16")[-1][2]
        cm = g.action_mask()
        assert cm.dtype == torch.int32 and tuple(cm.shape) == want.shape and cm.is_cuda
        cm2, ac = g.action_mask("+xzqeawsd")
        g.synchronize()
        assert cm2.data_ptr() == cm.data_ptr() and g.action_mask("+xzqeawsd")[1].data_ptr() == ac.data_ptr()
        g.synchronize()
        assert np.array_equal(cm.cpu().numpy().view(np.uint32), want)
        assert np.array_equal(ac.cpu().numpy().view(np.uint32), actions_of(want, "+xzqeawsd"))
        m = env.decode_action_mask(cm.cpu().numpy())
        assert m.shape == want.shape + (30,) and not m[0, 3].any() and m[0, 0, 0] and not m[..., 3].any()  # agent 3 quit; '3' never
    finally:
        g.close()


def test_captured_behind_a_step_launch_and_replayed_three_times():
    """sf_step_device + sf_action_mask_device on one stream (no parallel branches), against the same calls made eagerly."""
    c = mc.case("mix")
    A, n = c.w.cfg.arenas, c.w.cfg.n_agents
    g, eager = env.ArenaBatch(c.w), env.ArenaBatch(mc.case("mix").w)
    stream = torch.cuda.Stream()
    try:
        g.set_stream(stream.cuda_stream)
        g.reset(c.tb, c.sr), eager.reset(c.tb, c.sr)
        k = 3
        cmds = torch.from_numpy(np.ascontiguousarray(c.rows[:k])).cuda()
        cm, ac = sentinel(A * n), sentinel(A * n)
        ecm, eac = sentinel(A * n), sentinel(A * n)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            g.step_device(cmds.data_ptr(), k)
            g.action_mask_device(cm.data_ptr(), "+xzqeawsd", ac.data_ptr())
        torch.cuda.synchronize()
        assert (g.digest() == eager.digest()).all()  # (capture launched nothing)
        for i in range(3):
            with torch.cuda.stream(stream):
                graph.replay()
            stream.synchronize()
            eager.step_device(cmds.data_ptr(), k)
            eager.action_mask_device(ecm.data_ptr(), "+xzqeawsd", eac.data_ptr())
            eager.synchronize()
            assert (g.digest() == eager.digest()).all(), i
            assert np.array_equal(words(cm, A, n), words(ecm, A, n)) and np.array_equal(words(ac, A, n), words(eac, A, n)), i
            assert (words(cm, A, n) & 1).any()
    finally:
        g.close(), eager.close()


def _hip():
    lib = sorted(glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so*")))
    H = C.CDLL(lib[0] if lib else "libamdhip64.so")
    H.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    H.hipFree.argtypes = [C.c_void_p]
    H.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    H.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return H


def test_every_misuse_is_refused_and_leaves_the_sentinels():
    c = mc.case("battle2")
    g = env.ArenaBatch(c.w)
    L, A, n = g.L, c.w.cfg.arenas, c.w.cfg.n_agents
    cm, ac = sentinel(A * n), sentinel(A * n)
    host = np.full(4 * A * n, 0xA5, dtype=np.uint8)
    # an allocation of its own, one word short (the extent check is made against the runtime's allocation, and a tensor's may
    # be larger than the tensor)
    H, short = _hip(), C.c_void_p()
    assert H.hipMalloc(C.byref(short), 4 * A * n - 4) == 0 and H.hipMemset(short, 0xA5, 4 * A * n - 4) == 0

    def call(commands=None, string=None, actions=None, handle=g.h):
        return L.sf_action_mask_device(handle, C.byref(abi.ActionMaskIO(commands, string, actions)))

    try:
        assert call(cm.data_ptr()) == SF_ERR_STATE and b"before sf_reset" in L.sf_last_error()
        assert L.sf_action_mask(g.h, host.ctypes.data_as(C.c_void_p)) == SF_ERR_STATE
        g.reset(c.tb, c.sr)
        before = g.digest()
        assert call(cm.data_ptr(), handle=None) == SF_ERR_ARG and L.sf_action_mask_device(g.h, None) == SF_ERR_ARG
        assert L.sf_action_mask(g.h, None) == SF_ERR_ARG
        assert call() == SF_ERR_ARG and b"no output" in L.sf_last_error()
        assert call(cm.data_ptr(), None, ac.data_ptr()) == SF_ERR_ARG and b"both" in L.sf_last_error()
        assert call(cm.data_ptr(), b"+xzqeawsd", None) == SF_ERR_ARG and b"both" in L.sf_last_error()
        assert call(None, b"+xzqeawsd", None) == SF_ERR_ARG
        assert call(cm.data_ptr(), b"+xzqeawsD", ac.data_ptr()) == SF_ERR_ARG and b"not in SF_COMMANDS" in L.sf_last_error()
        assert call(cm.data_ptr(), b"+" * 33, ac.data_ptr()) == SF_ERR_ARG and b"1..32" in L.sf_last_error()
        assert call(cm.data_ptr(), b"", ac.data_ptr()) == SF_ERR_ARG and b"1..32" in L.sf_last_error()
        assert call(host.ctypes.data) == SF_ERR_ARG and b"not device memory" in L.sf_last_error()
        assert call(cm.data_ptr(), b"+", host.ctypes.data) == SF_ERR_ARG and b"d_actions" in L.sf_last_error()
        assert call(cm.data_ptr() + 2) == SF_ERR_ARG and b"aligned" in L.sf_last_error()
        assert call(short.value) == SF_ERR_ARG and b"past the end" in L.sf_last_error()
        assert call(cm.data_ptr(), b"+", short.value) == SF_ERR_ARG and b"past the end" in L.sf_last_error()
        assert call(short.value + 4) == SF_ERR_ARG and b"past the end" in L.sf_last_error()  # starts too late
        g.synchronize()
        back = np.zeros(4 * A * n - 4, dtype=np.uint8)
        assert H.hipMemcpy(back.ctypes.data, short, back.size, 2) == 0
        for buf in (cm.cpu().numpy(), ac.cpu().numpy(), back):
            assert (buf == 0xA5).all()  # nothing was launched by any of them
        assert (host == 0xA5).all() and (g.digest() == before).all()
        assert call(cm.data_ptr(), b"+" * 32, ac.data_ptr()) == 0  # 32 characters are taken
        g.synchronize()
        assert (words(cm, A, n) & 1).all()  # every agent is present after the reset, and '+' is always set
        assert (words(ac, A, n) == np.uint32(0xFFFFFFFF)).all()
    finally:
        g.close()
        H.hipFree(short)
