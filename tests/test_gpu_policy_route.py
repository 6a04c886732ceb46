"""Routing agents to several networks (include/strikeforce_policy.h sf_route_*, strikeforce_amd.policy.Router) against its
restatement, tests/route_ref.py.  Every destination buffer starts as a sentinel pattern, so memory the kernels must not
write is checked too.  Everything is a copy: every comparison is bit for bit, except the logs a rollout buffer takes of the
probabilities it is handed (within 2 f32 steps of the correctly rounded log, the bound tests/test_gpu_rollout.py holds
log_f32 to)."""
import ctypes as C

import numpy as np
import pytest
import torch

import policy_cases as pc
import reward_cases as rc
import rollout_ref as rr
import route_ref as ref
from strikeforce_amd import config, env, policy, rollout

pytestmark = pytest.mark.gpu

AGENTS = (1, 63, 64, 65, 130)


def _assign(agents, nets, nobody=True):
    """Networks of uneven size, interleaved; every seventh agent nobody's."""
    return [(-1 if nobody and a % 7 == 3 else (a * a + a // 3) % nets) for a in range(agents)]


def _dev(a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    torch.cuda.synchronize()
    return t


class _Buf:
    """A device buffer of 32-bit words or bytes that starts `odd` words behind an allocation's start (odd = 1: rows are not
    16-byte aligned, the dword path), filled from `init` (bit patterns)."""

    def __init__(self, init, odd=0):
        init = np.ascontiguousarray(init)
        self.shape, self.bytes = init.shape, init.dtype.itemsize == 1
        flat = init.reshape(-1)
        if self.bytes:
            self.t = _dev(np.concatenate([np.zeros(odd, dtype=np.uint8), flat.view(np.uint8)]))
        else:
            self.t = _dev(np.concatenate([np.zeros(odd, dtype=np.uint32), flat.view(np.uint32)]))
        self.odd = odd
        self.ptr = (self.t.data_ptr() + odd * (1 if self.bytes else 4)) if flat.size else None

    def bits(self):
        a = self.t.cpu().numpy()[self.odd:]
        return (a if self.bytes else a.view(np.uint32)).reshape(self.shape)


def _source(agents, cap, seed):
    rng = np.random.default_rng(seed)
    cycle = (0, 1, 3, 4, 5, cap - 1, cap, cap + 1, ref.MARKER)
    dense = (np.arange(agents * ref.DENSE, dtype=np.uint32) * np.uint32(2654435761)).reshape(agents, ref.DENSE)
    return dict(keys=rng.integers(0, 2 ** 32, size=(agents, cap), dtype=np.uint32), vals=rng.standard_normal((agents, cap)).astype(np.float32),
                counts=np.array([cycle[(a + seed) % len(cycle)] for a in range(agents)], dtype=np.uint32),
                pov=rng.standard_normal((agents, ref.HIDDEN)).astype(np.float32), dense=dense,
                reset=(rng.uniform(size=agents) < 0.4).astype(np.uint8))


def _flags(reset, form):
    """The device form of one flag per agent: a byte mask, or words read as (a // group) * stride.  In the words form the
    agents of a group share a flag and the words between the strides are set."""
    agents = len(reset)
    if form is None:
        return np.zeros(agents, dtype=np.uint8), {}, None
    if form == "mask":
        payload = np.where(reset != 0, 0x80, 0).astype(np.uint8)  # (any non-zero byte)
        return reset, dict(mask=True), payload
    group, stride = form
    groups = (agents + group - 1) // group
    gflag = reset[np.arange(groups) * group] != 0
    words = np.ones(groups * stride, dtype=np.int32)
    words[::stride] = np.where(gflag, -5, 0)
    return np.repeat(gflag, group)[:agents].astype(np.uint8), dict(stride=stride, group=group), words


def _gather_once(router, assign, nets, cap, src, form, odd, src_dense, dst_dense, skip=()):
    """One sf_route_gather into fresh sentinel-filled buffers with two spare rows each, against the restatement."""
    agents = len(assign)
    flags, how, payload = _flags(src["reset"], form)
    _, agents_of = ref.slots(assign, nets)
    want = [None if k in skip else ref.empty_dst(len(agents_of[k]) + 2, cap, dense=dst_dense) for k in range(nets)]
    ref.gather(assign, nets, dict(src, reset=flags, dense=src["dense"] if src_dense else None), want)
    s_keys, s_vals, s_pov = _Buf(src["keys"], odd), _Buf(src["vals"], odd), _Buf(src["pov"], odd)
    s_counts, s_dense = _Buf(src["counts"]), _Buf(src["dense"], odd)
    s = policy.RouteSrc()
    s.d_keys, s.d_vals, s.d_counts, s.d_pov, s.cap = s_keys.ptr, s_vals.ptr, s_counts.ptr, s_pov.ptr, cap
    s.d_dense = s_dense.ptr if src_dense else None
    d_flags = None
    if payload is not None:
        d_flags = _dev(payload)
        if "mask" in how:
            s.d_reset_mask = d_flags.data_ptr()
        else:
            s.d_reset_words, s.reset_stride, s.reset_group = d_flags.data_ptr(), how["stride"], how["group"]
    got = []
    dst = (policy.RouteDst * nets)()
    for k in range(nets):
        if want[k] is None:
            got.append(None)
            continue
        b = {}
        for name, v in want[k].items():  # (the restatement wrote into `want`: the device buffers start as the sentinel)
            fill = np.full(v.shape, ref.SENTINEL_U8 if v.dtype == np.uint8 else ref.SENTINEL, dtype=v.dtype)
            b[name] = _Buf(fill, 0 if name in ("counts", "reset") else odd)
        got.append(b)
        dst[k] = policy.RouteDst(b["keys"].ptr, b["vals"].ptr, b["counts"].ptr, b["pov"].ptr, cap,
                                 b["dense"].ptr if dst_dense else None, b["reset"].ptr)
    rc_ = router.L.sf_route_gather(router.h, C.byref(s), dst)
    assert rc_ == 0, router.L.sf_last_error()
    router.synchronize()
    what = (agents, nets, cap, form, odd, src_dense, dst_dense)
    for k in range(nets):
        if want[k] is None:
            continue
        for name, w in want[k].items():
            g = got[k][name].bits()
            assert np.array_equal(g, w), (what, k, name, np.argwhere(g != w)[:5].tolist())
    return want


@pytest.mark.parametrize("cap", [8, 9, 16])
@pytest.mark.parametrize("nets", [1, 2, 3])
@pytest.mark.parametrize("agents", AGENTS)
def test_gather_matches_the_restatement(agents, nets, cap):
    """Counts cycle through 0, 1, 3, 4, 5, cap-1, cap, cap+1 and the marker; four launches: a byte mask with aligned bases;
    words of group 1 with every base one dword off a 16-byte boundary (the dword path, cap 8 and 16 too); words of group 6
    without a source dense buffer; no flags, odd bases, without destination dense buffers.  Every buffer of every network,
    its two spare rows included, equals the restatement's: entries behind the count, rows behind count(k), and dense rows
    of agents whose list fitted still hold the sentinel."""
    assign = _assign(agents, nets)
    router = policy.Router(assign, nets, cap=cap)
    assert [router.count(k) for k in range(nets)] == [len(x) for x in ref.slots(assign, nets)[1]]
    over = 0
    for i, (form, odd, sd, dd) in enumerate([("mask", 0, True, True), ((1, 3), 1, True, True), ((6, 2), 0, False, True), (None, 1, True, False)]):
        src = _source(agents, cap, seed=100 * agents + 10 * nets + i)
        want = _gather_once(router, assign, nets, cap, src, form, odd, sd, dd)
        if sd and dd:
            over += sum(int((w["dense"][:, 0] != ref.SENTINEL).sum()) for w in want)
        else:
            assert all("dense" not in w or (w["dense"] == ref.SENTINEL).all() for w in want)
    if agents >= 63:
        assert over > 0  # (lists that did not fit were among the assigned agents)
    router.close()


def test_gather_network_without_agents_skipped_networks_and_nobodys():
    """Network 1 of 3 has no agents (its tensors are empty: NULL pointers); a dst[k] of NULLs is skipped and the others are
    still written; with every agent on -1 nothing is written at all."""
    cap, agents = 8, 65
    assign = [(-1 if a % 5 == 0 else 2 * (a % 2)) for a in range(agents)]
    router = policy.Router(assign, 3, cap=cap)
    assert router.count(1) == 0 and router.agents_of(1).numel() == 0
    for k in (0, 2):
        assert router.agents_of(k).cpu().tolist() == ref.slots(assign, 3)[1][k]
    _gather_once(router, assign, 3, cap, _source(agents, cap, 1), "mask", 0, True, True)
    _gather_once(router, assign, 3, cap, _source(agents, cap, 2), "mask", 0, True, True, skip=(0,))
    router.close()
    nobody = [-1] * agents
    router = policy.Router(nobody, 2, cap=cap)
    assert router.count(0) == 0 and router.count(1) == 0
    _gather_once(router, nobody, 2, cap, _source(agents, cap, 3), "mask", 0, True, True)
    router.scatter({})
    router.synchronize()
    router.close()


def _rows(n, rng):
    return dict(cmd=rng.integers(32, 127, size=n).astype(np.uint8), action=rng.integers(0, 9, size=n).astype(np.int32),
                probs=rng.uniform(size=(n, 9)).astype(np.float32), value=rng.uniform(size=n).astype(np.float32),
                reward=rng.standard_normal(n).astype(np.float32), disc=rng.uniform(size=n).astype(np.float32))


def _env_rows(agents):
    return {f: np.full((agents, 9) if f == "probs" else agents, ref.SENTINEL_U8 if f == "cmd" else ref.SENTINEL,
                       dtype=np.uint8 if f == "cmd" else np.uint32) for f in ref.ROW_FIELDS}


@pytest.mark.parametrize("agents", [1, 65, 130])
def test_scatter_matches_the_restatement(agents):
    """Two networks whose rows interleave in the environment's order; all fields, then each field NULL in turn on the
    environment's side, then on one network's side: the other fields arrive, the NULL one and the rows of the agents on -1
    keep the sentinel (a scripted command survives)."""
    nets = 2 if agents > 1 else 1
    assign = _assign(agents, nets)
    router = policy.Router(assign, nets, cap=8)
    _, agents_of = ref.slots(assign, nets)
    rng = np.random.default_rng(agents)
    rows = [_rows(len(agents_of[k]), rng) for k in range(nets)]
    d_rows = [{f: _Buf(ref.bits(v)) for f, v in r.items()} for r in rows]
    cases = [(None, None)] + [(f, "env") for f in ref.ROW_FIELDS] + [(f, "net") for f in ref.ROW_FIELDS]
    for field, side in cases:
        want = _env_rows(agents)
        got = {f: _Buf(v) for f, v in want.items()}
        rows_w = [dict(r) for r in rows]
        if side == "env":
            want[field] = None
        if side == "net":
            rows_w[nets - 1][field] = None
        ref.scatter(assign, nets, rows_w, want)
        c_rows = (policy.RouteRows * nets)(*[policy.RouteRows(*[None if rows_w[k][f] is None else d_rows[k][f].ptr for f in ref.ROW_FIELDS])
                                             for k in range(nets)])
        c_env = policy.RouteRows(*[None if want[f] is None else got[f].ptr for f in ref.ROW_FIELDS])
        assert router.L.sf_route_scatter(router.h, c_rows, C.byref(c_env)) == 0, router.L.sf_last_error()
        router.synchronize()
        for f in ref.ROW_FIELDS:
            w = want[f] if want[f] is not None else _env_rows(agents)[f]  # (a NULL field: the buffer was not handed over)
            assert np.array_equal(got[f].bits(), w), (agents, field, side, f)
        if field is None and agents > 1:
            mine = np.array(assign) >= 0
            assert (got["cmd"].bits()[~mine] == ref.SENTINEL_U8).all() and (got["cmd"].bits()[mine] != ref.SENTINEL_U8).all()
    router.close()


# ---- routing changes no result ---------------------------------------------------------------------------------------------
ROUTED_CAP = 320  # obs_sparse1 has about 307 non-zeros: some lists do not fit and are evaluated from their dense rows
PARAM_NAMES = ("gain-1", "gain-3", "gain-0.3")
RESTART_TICKS = (0, 3, 5)


def _memory(net, n):
    return [net.get_memory(i) for i in range(n)]


@pytest.mark.parametrize("greedy", [True, False], ids=["greedy", "sampled"])
@pytest.mark.parametrize("nets", [2, 3])
@pytest.mark.parametrize("agents", [17, 65])
def test_routing_changes_no_result(agents, nets, greedy):
    """Six ticks of tests/policy_cases.py's 1 %-dense observations, restart masks (three agents in ten) on ticks 0, 3 and 5.
    Network k — a policy and a reward model on parameter set k — behind the route answers, bit for bit, what a second pair
    of objects with the same parameters and count(k) agents answers to the numpy-gathered rows through the existing entries:
    probs, value, cmd, action, D, log D every tick, and every slot's h_state / action_input at the end.  The scattered
    environment-order rows equal the numpy scatter."""
    assign = _assign(agents, nets)
    _, agents_of = ref.slots(assign, nets)
    rng = np.random.default_rng(1000 * agents + nets)
    router = policy.Router(assign, nets, cap=ROUTED_CAP, dense=True)
    counts_k = [router.count(k) for k in range(nets)]
    assert counts_k == [len(x) for x in agents_of] and min(counts_k) > 0
    routed = [(policy.PolicyBatch(pc.parameters(PARAM_NAMES[k]), counts_k[k]), policy.RewardBatch(pc.parameters(PARAM_NAMES[k]), counts_k[k]))
              for k in range(nets)]
    plain = [(policy.PolicyBatch(pc.parameters(PARAM_NAMES[k]), counts_k[k]), policy.RewardBatch(pc.parameters(PARAM_NAMES[k]), counts_k[k]))
             for k in range(nets)]
    overflowed = 0
    for tick in range(6):
        obs = pc.obs_sparse1(rng, agents)
        keys, vals, counts, pov = pc.lists_from_dense(obs, ROUTED_CAP)
        overflowed += int((counts > ROUTED_CAP).sum())
        mask = (rng.uniform(size=agents) < 0.3).astype(np.uint8) if tick in RESTART_TICKS else np.zeros(agents, dtype=np.uint8)
        d = dict(keys=_dev(keys), vals=_dev(vals), counts=_dev(counts), pov=_dev(pov), dense=_dev(obs), mask=_dev(mask))
        router.gather((d["keys"].data_ptr(), d["vals"].data_ptr(), d["counts"].data_ptr(), d["pov"].data_ptr(), ROUTED_CAP),
                      d_dense_ptr=d["dense"].data_ptr(), d_reset_mask_ptr=d["mask"].data_ptr())
        env_rows = {f: _Buf(v) for f, v in _env_rows(agents).items()}
        for k in range(nets):
            g = router.net[k]
            for f in ref.ROW_FIELDS:
                getattr(g, f).view(torch.uint8 if f == "cmd" else torch.int32).fill_(ref.SENTINEL_U8 if f == "cmd" else ref.SENTINEL)
            torch.cuda.synchronize()
            routed[k][0].predict_sparse(**router.inputs(k), **router.outputs(k), seed=500 + k, greedy=greedy)
            routed[k][1].reward_sparse(**router.inputs(k), d_action_ptr=g.action.data_ptr(), d_disc_ptr=g.disc.data_ptr(),
                                       d_reward_ptr=g.reward.data_ptr())
        router.scatter({f: b.ptr for f, b in env_rows.items()})
        router.synchronize()
        answers = []
        for k in range(nets):
            idx, n = agents_of[k], counts_k[k]
            p = dict(keys=_dev(keys[idx]), vals=_dev(vals[idx]), counts=_dev(counts[idx]), pov=_dev(pov[idx]), dense=_dev(obs[idx]),
                     mask=_dev(mask[idx]))
            o = {f: _Buf(v) for f, v in _env_rows(n).items()}
            lists = (p["keys"].data_ptr(), p["vals"].data_ptr(), p["counts"].data_ptr(), p["pov"].data_ptr(), ROUTED_CAP, n)
            plain[k][0].predict_sparse(*lists, o["probs"].ptr, o["value"].ptr, o["cmd"].ptr, seed=500 + k, greedy=greedy,
                                       d_action_ptr=o["action"].ptr, d_dense_ptr=p["dense"].data_ptr(), d_reset_mask_ptr=p["mask"].data_ptr())
            plain[k][1].reward_sparse(*lists, o["action"].ptr, d_disc_ptr=o["disc"].ptr, d_reward_ptr=o["reward"].ptr,
                                      d_dense_ptr=p["dense"].data_ptr(), d_reset_mask_ptr=p["mask"].data_ptr())
            plain[k][0].synchronize(), plain[k][1].synchronize()
            ans = {f: b.bits() for f, b in o.items()}
            for f in ref.ROW_FIELDS:
                got = ref.bits(getattr(router.net[k], f).cpu().numpy())
                assert (ans[f] != (ref.SENTINEL_U8 if f == "cmd" else ref.SENTINEL)).all(), (tick, k, f)
                assert np.array_equal(got, ans[f]), (tick, k, f, np.argwhere(got != ans[f])[:5].tolist())
            answers.append(ans)
        want = _env_rows(agents)
        ref.scatter(assign, nets, answers, want)
        for f in ref.ROW_FIELDS:
            assert np.array_equal(env_rows[f].bits(), want[f]), (tick, f)
    assert overflowed > 0  # (the dense rows were needed)
    for k in range(nets):
        for kind in (0, 1):
            for s, ((h1, a1), (h2, a2)) in enumerate(zip(_memory(routed[k][kind], counts_k[k]), _memory(plain[k][kind], counts_k[k]))):
                assert np.array_equal(h1.view(np.uint32), h2.view(np.uint32)) and np.array_equal(a1, a2), (k, kind, s)
    for pair in routed + plain:
        pair[0].close(), pair[1].close()
    router.close()


# ---- the closed loop -------------------------------------------------------------------------------------------------------
def test_closed_loop_equals_everybody_evaluates_everybody():
    """KITS (6 commanded humans, teams 1,2,3,1,2,3), 2 arenas, 40 ticks, two greedy networks assigned by team parity.  The
    routed loop (observe, gather, one predict per network on its own agents, scatter, step) issues the commands, and leaves
    the environment in the state (sf_state_digest after every tick), of the loop in which both networks evaluate every agent
    and the host selects per agent."""
    arenas, ticks, CAP = 2, 40, 2048
    w = config.baseline_workload("KITS", arenas=arenas)
    B = arenas * w.cfg.n_agents
    teams = [1, 2, 3, 1, 2, 3]
    assign = [teams[a % 6] % 2 for a in range(B)]
    params = [policy.init_parameters(seed=21), policy.init_parameters(seed=22, gain=3.0)]
    tb, sr = w.seeds()

    def buffers():
        return dict(keys=torch.zeros((B, CAP), dtype=torch.int32, device="cuda"), vals=torch.zeros((B, CAP), dtype=torch.float32, device="cuda"),
                    counts=torch.zeros(B, dtype=torch.int32, device="cuda"), pov=torch.zeros((B, 160), dtype=torch.float32, device="cuda"),
                    dense=torch.zeros((B, 32, 31, 31), dtype=torch.float32, device="cuda"))

    def observe(sim, b):
        sim.observe_sparse_device(b["keys"].data_ptr(), b["vals"].data_ptr(), b["counts"].data_ptr(), b["pov"].data_ptr(), CAP)
        sim.observe_overflow_device(b["counts"].data_ptr(), CAP, b["dense"].data_ptr(), b["pov"].data_ptr())

    # the routed loop
    sim = env.ArenaBatch(w)
    sim.reset(tb, sr)
    router = policy.Router(assign, 2, cap=CAP, dense=True)
    nets = [policy.PolicyBatch(params[k], router.count(k)) for k in range(2)]
    b, d_cmd = buffers(), torch.zeros(B, dtype=torch.uint8, device="cuda")
    d_probs, d_value = torch.zeros((B, 9), dtype=torch.float32, device="cuda"), torch.zeros(B, dtype=torch.float32, device="cuda")
    restarted = sim.done_view_device()
    routed_cmds, routed_digests, routed_probs, routed_value = [], [], [], []
    for t in range(ticks):
        observe(sim, b)
        router.gather((b["keys"].data_ptr(), b["vals"].data_ptr(), b["counts"].data_ptr(), b["pov"].data_ptr(), CAP),
                      d_dense_ptr=b["dense"].data_ptr(), reset_words=restarted)
        for k in range(2):
            nets[k].predict_sparse(**router.inputs(k), **router.outputs(k), greedy=True)
        router.scatter({"cmd": d_cmd, "probs": d_probs, "value": d_value})
        sim.step_device(d_cmd.data_ptr(), 1)
        sim.synchronize()
        routed_cmds.append(d_cmd.cpu().numpy().copy()), routed_digests.append(sim.digest().copy())
        routed_probs.append(d_probs.cpu().numpy().copy()), routed_value.append(d_value.cpu().numpy().copy())
    for n in nets:
        n.close()
    router.close(), sim.close()

    # both networks evaluate every agent; the host selects
    sim = env.ArenaBatch(w)
    sim.reset(tb, sr)
    nets = [policy.PolicyBatch(params[k], B) for k in range(2)]
    b = buffers()
    out = [dict(probs=torch.zeros((B, 9), dtype=torch.float32, device="cuda"), value=torch.zeros(B, dtype=torch.float32, device="cuda"),
                cmd=torch.zeros(B, dtype=torch.uint8, device="cuda")) for _ in range(2)]
    restarted = sim.done_view_device()
    owner = np.array(assign)
    for t in range(ticks):
        observe(sim, b)
        for k in range(2):
            nets[k].predict_sparse(b["keys"].data_ptr(), b["vals"].data_ptr(), b["counts"].data_ptr(), b["pov"].data_ptr(), CAP, B,
                                   out[k]["probs"].data_ptr(), out[k]["value"].data_ptr(), out[k]["cmd"].data_ptr(), greedy=True,
                                   d_dense_ptr=b["dense"].data_ptr(), reset_words=restarted)
            nets[k].synchronize()
        cmd = np.where(owner == 0, out[0]["cmd"].cpu().numpy(), out[1]["cmd"].cpu().numpy()).astype(np.uint8)
        assert np.array_equal(cmd, routed_cmds[t]), (t, cmd.tobytes(), routed_cmds[t].tobytes())
        probs = np.where((owner == 0)[:, None], out[0]["probs"].cpu().numpy(), out[1]["probs"].cpu().numpy())
        value = np.where(owner == 0, out[0]["value"].cpu().numpy(), out[1]["value"].cpu().numpy())
        assert np.array_equal(probs.view(np.uint32), routed_probs[t].view(np.uint32)), t
        assert np.array_equal(value.view(np.uint32), routed_value[t].view(np.uint32)), t
        d_sel = _dev(cmd)
        sim.step_device(d_sel.data_ptr(), 1)
        sim.synchronize()
        assert np.array_equal(sim.digest(), routed_digests[t]), t
    assert len({x.tobytes() for x in routed_probs}) == ticks  # (the networks' answers changed from tick to tick)
    for n in nets:
        n.close()
    sim.close()


# ---- a rollout buffer behind one routed network -----------------------------------------------------------------------------
@pytest.mark.parametrize("agents", [17, 65])
def test_rollout_behind_a_routed_network_records_its_agents(agents):
    """T = 4, six ticks: a RolloutBatch of count(1) agents records network 1's gathered rows (lists, counts, pov, the byte
    restart mask the gather wrote) and its compact answers; its buffers, cursors and counters equal tests/rollout_ref.py fed
    the numpy-gathered rows."""
    nets, cap, T, K = 2, 8, 4, 1
    assign = _assign(agents, nets)
    _, agents_of = ref.slots(assign, nets)
    idx, n = agents_of[K], len(agents_of[K])
    router = policy.Router(assign, nets, cap=cap)
    rb = rollout.RolloutBatch(n, T, cap)
    want = rr.RefRollout(n, T, cap, store_disc=False, store_imitate=False)
    for name in ("keys", "vals", "counts", "pov", "action", "logp", "value", "reward"):
        getattr(rb, name).view(torch.int32).fill_(rr.SENTINEL)
    torch.cuda.synchronize()
    rng = np.random.default_rng(agents)
    for tick in range(6):
        src = _source(agents, cap, seed=agents + tick)
        src["reset"] = (rng.uniform(size=agents) < 0.25).astype(np.uint8)
        d = {f: _dev(src[f]) for f in ("keys", "vals", "counts", "pov", "reset")}
        router.gather((d["keys"].data_ptr(), d["vals"].data_ptr(), d["counts"].data_ptr(), d["pov"].data_ptr(), cap),
                      d_reset_mask_ptr=d["reset"].data_ptr())
        rows = _rows(n, rng)
        rows["probs"] = rng.uniform(1e-6, 1.0, size=(n, 9)).astype(np.float32)
        g = router.net[K]
        for f in ("probs", "value", "action", "reward"):
            getattr(g, f).copy_(torch.from_numpy(rows[f]))
        torch.cuda.synchronize()
        rb.record(g.probs.data_ptr(), g.value.data_ptr(), g.action.data_ptr(), g.reward.data_ptr(), **router.inputs(K, record=True))
        rb.synchronize()
        want.record(tick, rows["probs"], rows["value"], rows["action"], rows["reward"], keys=src["keys"][idx], vals=src["vals"][idx],
                    counts=src["counts"][idx], pov=src["pov"][idx], cap=cap, reset=src["reset"][idx])
    for name, w in want.image.items():
        if name != "probs":
            got = ref.bits(getattr(rb, name).cpu().numpy())
            assert np.array_equal(got, w), (name, np.argwhere(got != w)[:5].tolist())
    logp, probs = rb.logp.cpu().numpy(), want.image["probs"].view(np.float32)
    assert (ref.bits(logp)[~want.written] == rr.SENTINEL).all()
    assert rc.log_ulps(logp[want.written], probs[want.written]) <= 2
    assert np.array_equal(rb.fill().cpu().numpy(), want.fill())
    ready, dropped, missing = rb.status()
    assert (ready, dropped, missing) == (int(want.ready().sum()), want.dropped, want.missing_states)
    assert dropped > 0 and missing > 0 and 0 < ready < n
    rb.close(), router.close()


# ---- misuse ----------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_with_a_message():
    L = env.load_library()
    policy._bind_route(L)
    err = lambda: L.sf_last_error().decode()
    for assign, nets, text in [([0, 2], 2, "assign[1]"), ([0, -2], 2, "assign[1]"), ([0, 0], 0, "nets must be"), ([0, 0], 9, "nets must be")]:
        with pytest.raises(env.StrikeForceError, match=r"sf_route_create failed \(-1\)") as e:
            policy.Router(assign, nets)
        assert text in str(e.value)
    cap = 8
    router = policy.Router([0, 1, 0], 2, cap=cap)
    n = C.c_int32()
    for net in (-1, 2):
        assert L.sf_route_count(router.h, net, C.byref(n)) == -1 and "network index out of range" in err()
        assert L.sf_route_agents_device(router.h, net, C.byref(C.c_void_p())) == -1 and "network index out of range" in err()
    assert L.sf_route_gather(router.h, None, router._dst) == -1 and "null src" in err()
    src = _source(3, cap, 0)
    d = {f: _dev(src[f]) for f in ("keys", "vals", "counts", "pov")}
    lists = (d["keys"].data_ptr(), d["vals"].data_ptr(), d["counts"].data_ptr(), d["pov"].data_ptr())
    with pytest.raises(env.StrikeForceError, match=r"sf_route_gather failed \(-1\).*cap differs"):
        router.gather(lists + (cap + 4,))
    with pytest.raises(env.StrikeForceError, match=r"sf_route_gather failed \(-1\)"):
        router.gather((None,) + lists[1:] + (cap,))
    s = policy.RouteSrc(*lists, cap)
    half = (policy.RouteDst * 2)(router._dst[0], policy.RouteDst(d_keys=router._dst[1].d_keys, cap=cap))
    assert L.sf_route_gather(router.h, C.byref(s), half) == -1 and "dst[1] has a null list buffer" in err()
    assert L.sf_route_scatter(router.h, None, None) == -1 and "null rows or env" in err()
    router.gather(lists + (cap,))  # (and the object still works)
    router.synchronize()
    assert router.net[0].counts.cpu().numpy().view(np.uint32).tolist() == [int(src["counts"][0]), int(src["counts"][2])]
    router.close()
