"""The device rollout buffer (include/strikeforce_policy.h sf_rollout_*, strikeforce_amd.rollout.RolloutBatch) against its
restatement, tests/rollout_ref.py.  Every buffer the kernels may write starts as a sentinel pattern, so memory they must
not write is checked too.  Bounds: copies, cursors and counters bit for bit; logs within 2 f32 steps of the correctly
rounded log (rc.log_ulps, the bound the project already holds log_f32 to); returns and statistics bit for bit against
the torch / sequential-f32 restatement; the advantage bit for bit against the f32 difference of the device's own returns
and log V; a replay of the stored rows bit for bit against the live tick."""
import numpy as np
import pytest
import torch

import policy_cases as pc
import reward_cases as rc
import rollout_ref as rr
from strikeforce_amd import config, env, policy, rollout

pytestmark = pytest.mark.gpu

GROUP, STRIDE = 2, 3  # the words form of the restart flags: agent a reads word (a // GROUP) * STRIDE
COUNTS = (0, 1, 3, 4, 7, 8, 9, rr.MARKER)
SPECIAL_PROBS = np.array([1e-8, 1.0, 1.0000001e-8, 0.0], dtype=np.float32)


def _dev(a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    torch.cuda.synchronize()
    return t


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _sentinel(rb):
    """Every tensor of a RolloutBatch to the pattern."""
    for name in ("keys", "vals", "counts", "pov", "action", "logp", "value", "reward", "disc"):
        t = getattr(rb, name)
        if t is not None:
            t.view(torch.int32).fill_(rr.SENTINEL)
    if rb.imitate is not None:
        rb.imitate.fill_(rr.SENTINEL_U8)
    torch.cuda.synchronize()


def _filled(shape):
    return torch.full(shape, rr.SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _compare(rb, ref, what):
    """Every buffer against the restatement's image, the cursors and the counters."""
    rb.synchronize()
    for name, want in ref.image.items():
        if name == "probs":
            continue
        got = _bits(getattr(rb, name))
        assert np.array_equal(got, want), (what, name, np.argwhere(got != want)[:5].tolist())
    # logs: untouched where no tick was ever written, else within 2 steps of the f32 log of the probability stored there
    logp, probs = rb.logp.cpu().numpy(), ref.image["probs"].view(np.float32)
    assert (_bits(logp)[~ref.written] == rr.SENTINEL).all(), what
    ulps = rc.log_ulps(logp[ref.written], probs[ref.written]) if ref.written.any() else 0
    assert ulps <= 2, (what, ulps)
    assert np.array_equal(rb.fill().cpu().numpy(), ref.fill()), what
    ready, dropped, missing = rb.status()
    assert (ready, dropped, missing) == (int(ref.ready().sum()), ref.dropped, ref.missing_states), what
    assert np.array_equal(rb.ready_mask().cpu().numpy(), ref.ready().astype(np.uint8)), what
    return ulps


class _Ticks:
    """Random buffers of one tick for `agents` agents with caller capacity `cap`."""

    def __init__(self, agents, cap, seed):
        self.agents, self.cap, self.rng = agents, cap, np.random.default_rng(seed)

    def make(self, tick):
        n, cap, rng = self.agents, self.cap, self.rng
        h = dict(keys=rng.integers(0, 2 ** 32, size=(n, cap), dtype=np.uint32), vals=rng.standard_normal((n, cap)).astype(np.float32),
                 counts=np.array([COUNTS[(a + 3 * tick) % len(COUNTS)] for a in range(n)], dtype=np.uint32),
                 pov=rng.standard_normal((n, rr.HIDDEN)).astype(np.float32), probs=rng.uniform(1e-6, 1.0, size=(n, 9)).astype(np.float32),
                 value=rng.uniform(0, 1, size=n).astype(np.float32), action=rng.integers(0, 9, size=n).astype(np.int32),
                 reward=rr.log32(rng.uniform(0, 1, size=n).astype(np.float32)), disc=rng.uniform(0, 1, size=n).astype(np.float32),
                 imitate=rng.integers(0, 2, size=n).astype(np.uint8))
        for a in range(n):  # the special probabilities wander through the nine columns
            h["probs"][a, (a + tick) % 9] = SPECIAL_PROBS[(a + tick) % 4]
        return h


def _flag(i, tick):
    """Every agent (group) restarts each 7th tick; those with i % 4 == 1 each 3rd tick too: they never fill T = 4 slots."""
    return (5 * i + 3 * tick) % 7 == 0 or (i % 4 == 1 and tick % 3 == 2)


def _restart_flags(agents, tick, form):
    """One flag per agent for this tick, and the device form of it.  In the words form agents of a group share a word, and
    the words between the strides are set: a kernel reading with the wrong stride would restart everybody."""
    if form == "mask":
        flags = np.array([_flag(a, tick) for a in range(agents)], dtype=np.uint8)
        return flags, flags
    groups = (agents + GROUP - 1) // GROUP
    gflag = np.array([_flag(g, tick) for g in range(groups)])
    words = np.ones(groups * STRIDE, dtype=np.int32)
    words[::STRIDE] = np.where(gflag, 7, 0)
    return np.repeat(gflag, GROUP)[:agents].astype(np.uint8), words


def _record(rb, ref, tick, h, cap, flags, form, payload):
    d = {k: _dev(v) for k, v in h.items()}
    d_flags = _dev(payload)
    kw = dict(d_reset_mask_ptr=d_flags.data_ptr()) if form == "mask" else dict(reset_words=(d_flags.data_ptr(), STRIDE, GROUP))
    rb.record(d["probs"].data_ptr(), d["value"].data_ptr(), d["action"].data_ptr(), d["reward"].data_ptr(), d["keys"].data_ptr(),
              d["vals"].data_ptr(), d["counts"].data_ptr(), d["pov"].data_ptr(), cap, d_disc_ptr=d["disc"].data_ptr(),
              d_imitate_ptr=d["imitate"].data_ptr(), **kw)
    rb.synchronize()  # (the tick's tensors die with this frame)
    ref.record(tick, h["probs"], h["value"], h["action"], h["reward"], keys=h["keys"], vals=h["vals"], counts=h["counts"], pov=h["pov"], cap=cap,
               disc=h["disc"], imitate=h["imitate"], reset=flags)


# ---- 1 + 2: record against the restatement, the logs ---------------------------------------------------------------------
@pytest.mark.parametrize("form", ["mask", "words"])
@pytest.mark.parametrize("cap", [8, 9, 16])
@pytest.mark.parametrize("agents", [1, 63, 64, 65, 130])
def test_record_matches_the_restatement(agents, cap, form):
    """T = 4, list_cap = 8, the caller's rows 8, 9 (rows not 16-byte aligned: the dword copy) and 16 wide; counts cycle through
    0, 1, 3, 4, 7, 8, 9 and the marker; restart flags as a byte mask or as words (group 2, stride 3) fall on slot 0, on the
    middle of a buffer, on slot T - 1 and on ready agents; probabilities include 1e-8, 1, 1.0000001e-8 and 0.  11 ticks (agents
    go ready and drop ticks, others never do), release of the ready agents, 5 more ticks, a masked release of agents ready and not: after
    each phase every buffer, the cursors, the ready mask and the three counters equal the restatement's."""
    T, LIST_CAP = 4, 8
    rb = rollout.RolloutBatch(agents, T, LIST_CAP, store_disc=True, store_imitate=True)
    ref = rr.RefRollout(agents, T, LIST_CAP)
    _sentinel(rb)
    ticks = _Ticks(agents, cap, seed=1000 * agents + cap)
    seen = set()  # where a restart flag met its agent: slot 0, middle, T - 1, ready
    for tick in range(11):
        flags, payload = _restart_flags(agents, tick, form)
        for a in np.flatnonzero(flags):
            f = int(ref.fill()[a])
            seen.add("first" if f == 0 else "ready" if f == T else "last" if f == T - 1 else "middle")
        _record(rb, ref, tick, ticks.make(tick), cap, flags, form, payload)
    if agents >= 63:
        assert seen == {"first", "middle", "last", "ready"}, seen
        assert ref.dropped > 0 and ref.missing_states > 0 and 0 < ref.ready().sum() < agents
    worst = _compare(rb, ref, "11 ticks")
    rb.release()
    ref.release()
    _compare(rb, ref, "release of the ready agents")
    for tick in range(11, 16):
        flags, payload = _restart_flags(agents, tick, form)
        _record(rb, ref, tick, ticks.make(tick), cap, flags, form, payload)
    worst = max(worst, _compare(rb, ref, "5 more ticks"))
    mask = np.zeros(agents, dtype=np.uint8)
    mask[::3] = 1  # (ready or not)
    if agents >= 63:
        assert (ref.fill()[mask == 1] == T).any() and ((ref.fill()[mask == 1] > 0) & (ref.fill()[mask == 1] < T)).any()
    rb.release(_dev(mask))
    ref.release(mask)
    _compare(rb, ref, "masked release")
    print("record %d agents cap %d %s: logs within %d ulp" % (agents, cap, form, worst))
    rb.close()


def test_record_of_fewer_agents_and_unaligned_rows_stays_inside_its_rows():
    """A buffer for 70 agents asked to record 65, from list rows that start 4 bytes off a 16-byte boundary (cap 8: the dword
    copy is chosen by the addresses) and without the optional buffers: agents 65..69 keep the sentinel everywhere and
    their cursor stays 0."""
    N, agents, T, LIST_CAP, cap = 70, 65, 4, 8, 8
    rb = rollout.RolloutBatch(N, T, LIST_CAP)
    ref = rr.RefRollout(N, T, LIST_CAP, store_disc=False, store_imitate=False)
    _sentinel(rb)
    h = _Ticks(agents, cap, seed=5).make(0)
    d = {k: _dev(v) for k, v in h.items()}
    off_k, off_v = _dev(np.zeros(agents * cap + 1, dtype=np.int32)), _dev(np.zeros(agents * cap + 1, dtype=np.float32))
    off_k[1:] = d["keys"].reshape(-1)
    off_v[1:] = d["vals"].reshape(-1)
    torch.cuda.synchronize()
    for tick in range(2):
        rb.record(d["probs"].data_ptr(), d["value"].data_ptr(), d["action"].data_ptr(), d["reward"].data_ptr(), off_k.data_ptr() + 4,
                  off_v.data_ptr() + 4, d["counts"].data_ptr(), d["pov"].data_ptr(), cap, agents=agents)
        ref.record(tick, h["probs"], h["value"], h["action"], h["reward"], keys=h["keys"], vals=h["vals"], counts=h["counts"], pov=h["pov"], cap=cap)
    _compare(rb, ref, "65 of 70")
    assert rb.fill().cpu().numpy()[agents:].tolist() == [0] * (N - agents)
    rb.close()


# ---- 3: returns, log V, advantages, statistics -----------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", rr.RETURNS_GAMMAS)
@pytest.mark.parametrize("T", rr.RETURNS_T)
def test_returns_match_the_reference_arithmetic(T, gamma):
    """130 agents, states not kept, T ticks recorded from the committed inputs (one reward of -inf, one value of 0); the last
    tick restarts agents 3, 64 and 129, which are therefore not ready.  d_returns equals the torch restatement bit for bit
    (NaNs as NaNs); d_logv is within 2 steps of the f32 log of the stored value; d_adv equals the f32 difference of the
    device's own d_returns and d_logv bit for bit; the statistics equal the sequential-f32 restatement bit for bit; rows of
    the agents that are not ready still hold the sentinel."""
    A = rr.RETURNS_AGENTS
    rewards, values, actions = rr.returns_case(T)
    rb = rollout.RolloutBatch(A, T, 8, store_states=False)
    d_r, d_v, d_a = _dev(rewards), _dev(values), _dev(actions)
    d_probs = _dev(np.full((A, 9), 1 / 9, dtype=np.float32))
    late = np.zeros(A, dtype=np.uint8)
    late[[3, 64, 129]] = 1
    d_late = _dev(late)
    for t in range(T):
        rb.record(d_probs.data_ptr(), d_v[t].data_ptr(), d_a[t].data_ptr(), d_r[t].data_ptr(), d_reset_mask_ptr=d_late.data_ptr() if t == T - 1 else None)
    ready = late == 0
    assert rb.status() == (int(ready.sum()), 0, 0)
    assert np.array_equal(_bits(rb.reward)[:, ready], _bits(rewards)[:, ready]) and np.array_equal(_bits(rb.value)[:, ready], _bits(values)[:, ready])
    out = (_filled((T, A)), _filled((T, A)), _filled((T, A)), _filled((A, 4)))
    rb.returns(gamma, out=out)
    rb.synchronize()
    ret, logv, adv, stats = (x.cpu().numpy() for x in out)
    for x in (ret, logv, adv):
        assert (_bits(x)[:, ~ready] == rr.SENTINEL).all()
    assert (_bits(stats)[~ready] == rr.SENTINEL).all()
    want = rr.returns_torch(rewards, gamma)
    same = (_bits(ret) == _bits(want)) | (np.isnan(ret) & np.isnan(want))
    print("T=%d gamma=%s: %d of %d returns differ" % (T, gamma, int((~same[:, ready]).sum()), int(ready.sum()) * T))
    assert same[:, ready].all()
    assert np.isneginf(ret[: T // 2 + 1, 1]).all()
    ulps = rc.log_ulps(logv[:, ready], values[:, ready])
    print("T=%d gamma=%s: log V within %d ulp" % (T, gamma, ulps))
    assert ulps <= 2 and np.isneginf(logv[T // 2, 2])
    with np.errstate(invalid="ignore"):
        diff = ret - logv  # (f32 - f32 in numpy: one rounding)
    same = (_bits(adv) == _bits(diff)) | (np.isnan(adv) & np.isnan(diff))
    assert same[:, ready].all() and adv[T // 2, 2] == np.inf
    ws = rr.stats_ref(rewards, actions)
    same = (_bits(stats) == _bits(ws)) | (np.isnan(stats) & np.isnan(ws))
    assert same[ready].all(), np.argwhere(~same)[:5].tolist()
    rb.close()


# ---- 4: the closed loop, and the replay of what it stored -----------------------------------------------------------------
@pytest.mark.parametrize("arenas", [6, 48])
def test_closed_loop_rows_replay_bit_for_bit(arenas):
    """6 arenas of BASELINE configs[2] — one agent per arena — and 48 of them (48 agents: three of k_tail's 16-row workgroups),
    T = 8, 20 ticks of observe-sparse, predict, reward, record, step with a
    test-written restart mask given to all three objects; probabilities, values, D and log D cloned on the side per tick.  A
    second policy and a second reward model replay rows 0..T-1 from reset_memory: forward_sparse on state(t) then
    update_actions(action[t]); reward_sparse on state(t) with action[t].  For every agent and every slot it has filled, the
    replay equals the live tick's clone bit for bit (slot -> tick by the restatement), and the stored row equals both."""
    T, LIST_CAP, CAP, TICKS = 8, 1024, 2048, 20
    w = config.baseline_workload("C3", arenas=arenas)
    sim = env.ArenaBatch(w)
    sim.reset(*w.seeds())
    B = w.cfg.arenas * w.cfg.n_agents
    assert B == arenas
    net, net2 = (policy.PolicyBatch(pc.parameters("gain-1"), B) for _ in range(2))
    rew, rew2 = (policy.RewardBatch(rc.parameters("gain-3"), B) for _ in range(2))
    rb = rollout.RolloutBatch(B, T, LIST_CAP, store_disc=True)
    ref = rr.RefRollout(B, T, LIST_CAP, store_states=False, store_imitate=False)
    _sentinel(rb)
    i32 = dict(dtype=torch.int32, device="cuda")
    d_keys, d_counts, d_act = torch.zeros((B, CAP), **i32), torch.zeros(B, **i32), torch.full((B,), 77, **i32)
    d_vals, d_pov = torch.zeros((B, CAP), device="cuda"), torch.zeros((B, 160), device="cuda")
    d_probs, d_value, d_disc, d_rew = _filled((B, 9)), _filled((B,)), _filled((B,)), _filled((B,))
    d_cmd = torch.zeros(B, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(404 + B)
    live = []
    for tick in range(TICKS):
        flags = (rng.random(B) < 0.15).astype(np.uint8)
        d_mask = _dev(flags)
        lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
        sim.observe_sparse_device(*lists)
        net.predict_sparse(*lists, B, d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr(), seed=9, d_action_ptr=d_act.data_ptr(),
                           d_reset_mask_ptr=d_mask.data_ptr())
        rew.reward_sparse(*lists, B, d_act.data_ptr(), d_disc.data_ptr(), d_rew.data_ptr(), d_reset_mask_ptr=d_mask.data_ptr())
        rb.record(d_probs.data_ptr(), d_value.data_ptr(), d_act.data_ptr(), d_rew.data_ptr(), *lists, d_disc_ptr=d_disc.data_ptr(),
                  d_reset_mask_ptr=d_mask.data_ptr())
        sim.synchronize(), net.synchronize(), rew.synchronize(), rb.synchronize()
        h = {k: v.cpu().numpy() for k, v in dict(probs=d_probs, value=d_value, action=d_act, reward=d_rew, disc=d_disc).items()}
        ref.record(tick, h["probs"], h["value"], h["action"], h["reward"], disc=h["disc"], reset=flags)
        live.append(h)
        sim.step_device(d_cmd.data_ptr(), 1)
    fill = ref.fill()
    assert np.array_equal(rb.fill().cpu().numpy(), fill)
    ready, dropped, missing = rb.status()
    assert ready == int((fill == T).sum()) and ready >= 5 and dropped == ref.dropped > 0 and missing == 0
    assert ((fill > 0) & (fill < T)).any() and net.sparse_overflows() == 0 and rew.sparse_overflows() == 0
    for name in ("action", "value", "reward", "disc"):
        assert np.array_equal(_bits(getattr(rb, name)), ref.image[name]), name
    # the replay
    p2, v2, dd2, r2 = _filled((B, 9)), _filled((B,)), _filled((B,)), _filled((B,))
    net2.reset_memory(), rew2.reset_memory()
    compared = 0
    for t in range(T):
        st = rb.state(t)
        assert st[4] == LIST_CAP
        net2.forward_sparse(*st, B, p2.data_ptr(), v2.data_ptr())
        net2.update_actions(rb.action[t].data_ptr(), B)
        rew2.reward_sparse(*st, B, rb.action[t].data_ptr(), dd2.data_ptr(), r2.data_ptr())
        net2.synchronize(), rew2.synchronize()
        got = dict(probs=_bits(p2), value=_bits(v2), disc=_bits(dd2), reward=_bits(r2))
        for a in np.flatnonzero(fill > t):
            was = live[ref.tick_of(a, t)]
            for k in got:
                assert np.array_equal(got[k][a], _bits(was[k])[a]), (t, a, k)
            assert _bits(rb.reward)[t, a] == got["reward"][a] and _bits(rb.disc)[t, a] == got["disc"][a]
            assert rc.log_ulps(rb.logp[t, a].cpu().numpy(), was["probs"][a]) <= 2
            compared += 1
    # (a slot no tick was ever written to holds the sentinel as its count: "did not fit", evaluated blank and counted)
    unfilled = int((~ref.written).sum())
    assert net2.sparse_overflows() == unfilled and rew2.sparse_overflows() == unfilled
    # ready agents: returns, then reset both memories with the ready mask and release
    ret, logv, adv, stats = rb.returns(0.99)
    rmask = rb.ready_mask()
    net.reset_memory(rmask.data_ptr()), rew.reset_memory(rmask.data_ptr())
    rb.release()
    rb.synchronize(), net.synchronize()
    is_ready = fill == T
    want = rr.returns_torch(ref.image["reward"].view(np.float32)[:, is_ready], 0.99)
    assert np.array_equal(_bits(ret)[:, is_ready], _bits(want)) and torch.isnan(ret[:, torch.from_numpy(~is_ready).cuda()]).all()
    assert np.array_equal(rb.fill().cpu().numpy(), np.where(is_ready, 0, fill))
    for a in np.flatnonzero(is_ready)[:3]:
        hm, am = net.get_memory(int(a))
        assert not hm.any() and am.tolist() == [1] + [0] * 8
    print("closed loop: %d agents x %d ticks, %d ready, %d dropped, %d (agent, slot) rows replayed" % (B, TICKS, ready, dropped, compared))
    for x in (net, net2, rew, rew2, rb, sim):
        x.close()


# ---- 5: update_actions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["policy", "reward"])
def test_update_actions_sets_the_one_hot(kind):
    """Indices -1, 0, 8, 9 and 4 for agents 0..4 of 7, on both kinds of object: get_memory shows the one-hot (outside [0, 9):
    action 0), h is not touched, agents 5 and 6 keep what was stored."""
    B = 7
    nb = policy.PolicyBatch(pc.parameters("gain-1"), B) if kind == "policy" else policy.RewardBatch(rc.parameters("gain-1"), B)
    rng = np.random.default_rng(3)
    h0 = rng.standard_normal((B, 2, 160)).astype(np.float32)
    for b in range(B):
        nb.set_memory(b, h0[b], np.eye(9, dtype=np.float32)[5])
    d_idx = _dev(np.array([-1, 0, 8, 9, 4, 2, 2], dtype=np.int32))
    nb.update_actions(d_idx.data_ptr(), 5)
    nb.synchronize()
    for b, want in enumerate([0, 0, 8, 0, 4, 5, 5]):
        h, a = nb.get_memory(b)
        assert np.array_equal(a, np.eye(9, dtype=np.float32)[want]) and np.array_equal(_bits(h), _bits(h0[b])), b
    nb.close()


# ---- 6: misuse -------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused_and_changes_nothing():
    B, T, LIST_CAP = 5, 4, 8
    for bad in (dict(T=3), dict(T=0), dict(list_cap=6), dict(list_cap=2052), dict(list_cap=0), dict(agents=0)):
        args = dict(agents=B, T=T, list_cap=LIST_CAP)
        args.update(bad)
        with pytest.raises(env.StrikeForceError, match=r"\(-1\)"):
            rollout.RolloutBatch(**args)
    rollout.RolloutBatch(B, T, 6, store_states=False).close()  # (list_cap is not looked at when no states are kept)
    rb = rollout.RolloutBatch(B, T, LIST_CAP, store_disc=True)
    _sentinel(rb)
    h = _Ticks(B, 8, seed=1).make(0)
    d = {k: _dev(v) for k, v in h.items()}
    good = dict(d_probs_ptr=d["probs"].data_ptr(), d_value_ptr=d["value"].data_ptr(), d_action_ptr=d["action"].data_ptr(),
                d_reward_ptr=d["reward"].data_ptr(), d_keys_ptr=d["keys"].data_ptr(), d_vals_ptr=d["vals"].data_ptr(),
                d_counts_ptr=d["counts"].data_ptr(), d_pov_ptr=d["pov"].data_ptr(), cap=8, d_disc_ptr=d["disc"].data_ptr())
    for bad in (dict(cap=0), dict(cap=2049), dict(d_keys_ptr=None), dict(d_pov_ptr=None), dict(d_probs_ptr=None), dict(d_reward_ptr=None),
                dict(d_disc_ptr=None), dict(agents=B + 1), dict(agents=0), dict(reset_words=(d["action"].data_ptr(), 0, 1))):
        with pytest.raises(env.StrikeForceError, match=r"\(-1\)"):
            rb.record(**dict(good, **bad))
    for t in (-1, T):
        with pytest.raises(env.StrikeForceError, match=r"\(-1\).*slot out of range"):
            rb.state(t)
    with pytest.raises(env.StrikeForceError, match=r"\(-1\)"):
        rb.returns(0.99, out=(None, None, None, None))
    nostate = rollout.RolloutBatch(B, T, LIST_CAP, store_states=False)
    with pytest.raises(env.StrikeForceError, match=r"\(-4\).*keeps no states"):
        nostate.state(0)
    pb = policy.PolicyBatch(pc.parameters("gain-1"), B)
    for call in (lambda: pb.update_actions(d["action"].data_ptr(), B + 1), lambda: pb.update_actions(None, B)):
        with pytest.raises(env.StrikeForceError, match=r"\(-1\)"):
            call()
    rb.synchronize(), pb.synchronize()
    ref = rr.RefRollout(B, T, LIST_CAP, store_imitate=False)
    _compare(rb, ref, "after the refused calls")  # every buffer still the sentinel, cursors 0, counters 0
    assert pb.get_memory(0)[1].tolist() == [1] + [0] * 8
    rb.record(**good)  # and the good call records
    ref.record(0, h["probs"], h["value"], h["action"], h["reward"], keys=h["keys"], vals=h["vals"], counts=h["counts"], pov=h["pov"], cap=8, disc=h["disc"])
    _compare(rb, ref, "the good call")
    for x in (rb, nostate, pb):
        x.close()
