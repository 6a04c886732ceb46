"""The continuing rollout buffer and sf_rollout_gae on the device (include/strikeforce_policy.h; rollout.RolloutBatch(...,
continuing=True), RolloutBatch.gae) against tests/rollout_gae_ref.py.  Every buffer the kernels may write starts as a
sentinel pattern.  Bounds: copies, `first`, cursors and counters bit for bit; the stored logs within 2 f32 steps of the
correctly rounded log, as tests/test_gpu_rollout.py holds them; returns, V and advantages bit for bit against the
uncontracted numpy f32 recursion (NaNs as NaNs); the reference configuration bit for bit against sf_rollout_returns on the
same buffer; a replay of a stored block across game ends bit for bit against what was stored."""
import ctypes as C

import numpy as np
import pytest
import torch

import policy_cases as pc
import rollout_gae_ref as gr
import rollout_ref as rr
import test_gpu_rollout as tg
from strikeforce_amd import config, env, policy, rollout

pytestmark = pytest.mark.gpu

STRIDE = 3  # the words form: agent a reads word (a // group) * STRIDE
_dev, _bits, _filled = tg._dev, tg._bits, tg._filled


def _sentinel(rb):
    tg._sentinel(rb)
    if rb.first is not None:
        rb.first.fill_(rr.SENTINEL_U8)
    torch.cuda.synchronize()


def _flag(i, tick):
    """Every agent (group) restarts each 7th tick; those with i % 4 == 1 on two ticks of three, one behind the other."""
    return (5 * i + 3 * tick) % 7 == 0 or (i % 4 == 1 and tick % 3 != 0)


def _restart_flags(agents, tick, form):
    """One flag per agent, and its device form: bytes, or words shared by `group` agents with the words between the strides set."""
    if form == "mask":
        flags = np.array([_flag(a, tick) for a in range(agents)], dtype=np.uint8)
        return flags, flags, {}
    group = int(form[5:])
    groups = (agents + group - 1) // group
    gflag = np.array([_flag(g, tick) for g in range(groups)])
    words = np.ones(groups * STRIDE, dtype=np.int32)
    words[::STRIDE] = np.where(gflag, 7, 0)
    return np.repeat(gflag, group)[:agents].astype(np.uint8), words, dict(group=group)


def _record(rb, ref, tick, h, cap, flags, payload, group=None):
    d = {k: _dev(v) for k, v in h.items()}
    d_flags = _dev(payload)
    kw = dict(d_reset_mask_ptr=d_flags.data_ptr()) if group is None else dict(reset_words=(d_flags.data_ptr(), STRIDE, group))
    rb.record(d["probs"].data_ptr(), d["value"].data_ptr(), d["action"].data_ptr(), d["reward"].data_ptr(), d["keys"].data_ptr(),
              d["vals"].data_ptr(), d["counts"].data_ptr(), d["pov"].data_ptr(), cap, d_disc_ptr=d["disc"].data_ptr(),
              d_imitate_ptr=d["imitate"].data_ptr(), **kw)
    rb.synchronize()
    ref.record(tick, h["probs"], h["value"], h["action"], h["reward"], keys=h["keys"], vals=h["vals"], counts=h["counts"], pov=h["pov"], cap=cap,
               disc=h["disc"], imitate=h["imitate"], reset=flags)


# ---- 1: record under the continuing rule ----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["mask", "words1", "words6"])
@pytest.mark.parametrize("cap", [8, 9, 16])
@pytest.mark.parametrize("agents", [1, 63, 64, 65, 130])
def test_continuing_record_matches_the_restatement(agents, cap, form):
    """T = 4, list_cap = 8, test_gpu_rollout.py's ticks (counts 0..9 and the marker, caller rows 8 / 9 / 16 wide, special
    probabilities); restart flags as bytes or as words shared by 1 or 6 agents.  6 ticks (everybody is ready after 4: two are
    dropped, their flags ignored), release, 3 ticks, a masked release of every third agent, 3 ticks (the released agents hold
    3 slots, the others are ready and dropped twice): after each phase every buffer, `first`, the cursors, the ready mask
    and the counters equal the restatement's.  Then sf_rollout_continue(NULL): the per-game rule again, cursors 0, `first`
    no longer written."""
    T, LIST_CAP = 4, 8
    rb = rollout.RolloutBatch(agents, T, LIST_CAP, store_disc=True, store_imitate=True, continuing=True)
    ref = gr.RefRolloutCont(agents, T, LIST_CAP)
    _sentinel(rb)
    ticks = tg._Ticks(agents, cap, seed=2000 * agents + cap)
    seen, prev = set(), np.zeros(agents, dtype=bool)

    def run(first_tick, n):
        nonlocal prev
        for tick in range(first_tick, first_tick + n):
            flags, payload, kw = _restart_flags(agents, tick, form)
            fill = ref.fill()
            for a in np.flatnonzero(flags):
                f = int(fill[a])
                seen.add("first" if f == 0 else "ready" if f == T else "last" if f == T - 1 else "middle")
                if prev[a] and 0 < f < T:
                    seen.add("consecutive")
            prev = flags.astype(bool) & (fill < T)
            _record(rb, ref, tick, ticks.make(tick), cap, flags, payload, **kw)

    run(0, 6)
    assert ref.ready().all() and ref.dropped == 2 * agents
    worst = tg._compare(rb, ref, "6 ticks")
    rb.release()
    ref.release()
    tg._compare(rb, ref, "release of the ready agents")
    run(6, 3)
    assert (ref.fill() == 3).all()
    mask = np.zeros(agents, dtype=np.uint8)
    mask[::3] = 1
    rb.release(_dev(mask))
    ref.release(mask)
    tg._compare(rb, ref, "masked release")
    run(9, 3)
    assert np.array_equal(ref.fill(), np.where(mask == 1, 3, T))
    worst = max(worst, tg._compare(rb, ref, "3 more ticks"))
    if agents >= 63:
        assert seen == {"first", "middle", "last", "ready", "consecutive"}, seen
        first = ref.image["first"]
        assert (first == 1).any() and (first == 0).any() and ref.missing_states > 0
    # back to the per-game rule
    rb._ck(rb.L.sf_rollout_continue(rb.h, None), "sf_rollout_continue")
    old, counted = gr.RefRolloutCont(agents, T, LIST_CAP), (ref.dropped, ref.missing_states)  # (old: only for its sentinel image of `first`)
    ref = rr.RefRollout(agents, T, LIST_CAP)
    ref.dropped, ref.missing_states = counted  # (the counters count since sf_rollout_create)
    _sentinel(rb)
    for tick in range(12, 19):
        flags, payload, kw = _restart_flags(agents, tick, form)
        _record(rb, ref, tick, ticks.make(tick), cap, flags, payload, **kw)
    tg._compare(rb, ref, "the per-game rule again")
    assert np.array_equal(_bits(rb.first), old.image["first"])
    if agents >= 63:
        assert 0 < ref.ready().sum() < agents  # (restarts rewound some agents: this is the old rule)
    print("continuing record %d agents cap %d %s: logs within %d ulp" % (agents, cap, form, worst))
    rb.close()


# ---- 2: sf_rollout_gae ------------------------------------------------------------------------------------------------------
def _same(got, want):
    return (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))


def _fill_block(T, continuing=True):
    """A rollout without states filled from rollout_gae_ref.gae_case(T) by T record calls, its game ends as the restart mask;
    NOT_READY's agents are released in front of the last tick, so they hold one slot."""
    A = gr.GAE_AGENTS
    rewards, values, actions, first, nxt, nv = gr.gae_case(T)
    rb = rollout.RolloutBatch(A, T, 8, store_states=False, continuing=continuing)
    _sentinel(rb)
    d_r, d_v, d_a, d_f = _dev(rewards), _dev(values), _dev(actions), _dev(first)
    d_probs = _dev(np.full((A, 9), 1 / 9, dtype=np.float32))
    late = np.zeros(A, dtype=np.uint8)
    late[list(gr.NOT_READY)] = 1
    for t in range(T):
        if t == T - 1:
            rb.release(_dev(late))
        rb.record(d_probs.data_ptr(), d_v[t].data_ptr(), d_a[t].data_ptr(), d_r[t].data_ptr(), d_reset_mask_ptr=d_f[t].data_ptr())
    ready = late == 0
    if continuing:
        assert rb.status() == (int(ready.sum()), 0, 0)
    return rb, ready, (rewards, values, first, nxt, nv)


@pytest.mark.parametrize("lam", gr.GAE_LAMBDAS)
@pytest.mark.parametrize("gamma", gr.GAE_GAMMAS)
@pytest.mark.parametrize("T", gr.GAE_T)
def test_gae_matches_the_recursion(T, gamma, lam):
    """130 agents, the committed inputs: game ends at first[1], the middle, first[T - 1], the next tick's flag, adjacent and
    random ones; a reward of -inf and a value of 0 beside a game end.  reward_scale = 1.f - gamma.  log_values 0 and 1, each
    without a next value and with one (the next flags as bytes, and as words of group 2): returns, V and advantages equal
    the numpy f32 recursion bit for bit, nothing is NaN, the -inf stays in its game, the agents that are not ready keep the
    sentinel.  Each output NULL in turn leaves the others as they were.  With `first` zeroed, the reference configuration
    equals sf_rollout_returns on the same buffer in every bit."""
    A = gr.GAE_AGENTS
    rb, ready, (rewards, values, first, nxt, nv) = _fill_block(T)
    assert np.array_equal(_bits(rb.first)[:, ready], first[:, ready])
    assert np.array_equal(_bits(rb.reward)[:, ready], _bits(rewards)[:, ready])
    scale = float(np.float32(1) - np.float32(gamma))
    d_nv, d_nm = _dev(nv), _dev(nxt)
    words = np.ones(((A + 1) // 2) * STRIDE, dtype=np.int32)
    words[::STRIDE] = 5 * nxt.reshape(-1, 2).max(axis=1)
    nxt_words = np.repeat(nxt.reshape(-1, 2).max(axis=1), 2).astype(np.uint8)
    d_nw = _dev(words)
    for log_values in (False, True):
        for boot in (False, True):
            kw, ref_kw = {}, {}
            if boot and log_values:
                kw, ref_kw = dict(next_value=d_nv, next_words=(d_nw.data_ptr(), STRIDE, 2)), dict(next_value=nv, next_end=nxt_words)
            elif boot:
                kw, ref_kw = dict(next_value=d_nv, next_mask=d_nm), dict(next_value=nv, next_end=nxt)
            out = (_filled((T, A)), _filled((T, A)), _filled((T, A)))
            rb.gae(gamma, lam, reward_scale=scale, log_values=log_values, out=out, **kw)
            rb.synchronize()
            got = [x.cpu().numpy() for x in out]
            want = gr.gae_numpy(rewards, values, first, gamma, lam, reward_scale=scale, log_values=log_values, **ref_kw)
            for name, g, w in zip(("returns", "v", "adv"), got, want):
                bad = ~_same(g, w)[:, ready]
                print("T=%d gamma=%s lambda=%s log=%d boot=%d %s: %d of %d differ" % (T, gamma, lam, log_values, boot, name, int(bad.sum()), bad.size))
                assert not bad.any(), (name, np.argwhere(bad)[:5].tolist())
                assert (_bits(g)[:, ~ready] == rr.SENTINEL).all(), name
            G, V, Adv = got
            assert not np.isnan(G[:, ready]).any() and not np.isnan(Adv[:, ready]).any()
            assert np.isneginf(G[T // 2, 2]) and np.isfinite(G[: T // 2, 2]).all()
            if log_values:
                assert np.isneginf(V[T // 2, 10]) and np.isfinite(G[: T // 2, 10]).all() and Adv[T // 2, 10] == np.inf
            if boot:  # each output NULL in turn (with d_v NULL and log_values the library's own V array is used)
                for skip in range(3):
                    part = [None if k == skip else _filled((T, A)) for k in range(3)]
                    rb.gae(gamma, lam, reward_scale=scale, log_values=log_values, out=tuple(part), **kw)
                    rb.synchronize()
                    for k in range(3):
                        assert k == skip or np.array_equal(_bits(part[k]), _bits(out[k])), (skip, k)
    # the reference configuration
    rb.first.zero_()
    torch.cuda.synchronize()
    ref_out = (_filled((T, A)), _filled((T, A)), _filled((T, A)), _filled((A, 4)))
    rb.returns(gamma, out=ref_out)
    out = (_filled((T, A)), _filled((T, A)), _filled((T, A)))
    rb.gae(gamma, 1.0, reward_scale=scale, log_values=True, out=out)
    rb.synchronize()
    for k, name in enumerate(("returns", "log V", "adv")):
        assert np.array_equal(_bits(out[k]), _bits(ref_out[k])), name
    assert (_bits(out[0])[:, ready] != rr.SENTINEL).all()
    rb.close()


def test_gae_under_the_per_game_rule_sees_no_game_ends():
    """A per-game rollout (no `first`): sf_rollout_gae runs with `first` counting as all zero."""
    T, A = 4, gr.GAE_AGENTS
    rb, _, (rewards, values, first, nxt, nv) = _fill_block(T, continuing=False)
    # (under the per-game rule the recorded flags rewound agents: take the buffer as it stands)
    rb.synchronize()
    ready = rb.ready_mask().cpu().numpy() != 0
    assert ready.sum() > 10 and rb.first is None
    stored_r, stored_v = rb.reward.cpu().numpy(), rb.value.cpu().numpy()
    out = (_filled((T, A)), _filled((T, A)), _filled((T, A)))
    rb.gae(0.99, 0.95, reward_scale=0.25, next_value=_dev(nv), out=out)
    rb.synchronize()
    want = gr.gae_numpy(stored_r[:, ready], stored_v[:, ready], None, 0.99, 0.95, reward_scale=0.25, next_value=nv[ready])
    for g, w in zip(out, want):
        g = g.cpu().numpy()
        assert _same(g[:, ready], w).all() and (_bits(g)[:, ~ready] == rr.SENTINEL).all()
    rb.close()


# ---- 3: the closed loop across game ends, replayed ------------------------------------------------------------------------
def test_closed_loop_block_replays_across_game_ends():
    """64 arenas of BASELINE configs[1] without auto_reset, sf_reset_arenas(done, max_steps = 10) behind every step, its
    `selected` bytes the restart flags of the next tick's predict and record; T = 64, 64 ticks: one block, every agent
    ready.  A second policy replays it — reset_memory_n(first[t]), forward_sparse on state(t), update_actions(action[t]) —
    into a second rollout: its logp and value equal the stored ones bit for bit.  At least 5 game ends per agent lie inside
    the block."""
    T, LIST_CAP, CAP, B = 64, 1024, 2048, 64
    w = config.baseline_workload("C2", arenas=B, auto_reset=0)
    assert w.cfg.arenas * w.cfg.n_agents == B
    sim = env.ArenaBatch(w)
    sim.reset(*w.seeds())
    net, net2 = (policy.PolicyBatch(pc.parameters("gain-1"), B) for _ in range(2))
    rb = rollout.RolloutBatch(B, T, LIST_CAP, continuing=True)
    rb2 = rollout.RolloutBatch(B, T, LIST_CAP, store_states=False, continuing=True)
    _sentinel(rb), _sentinel(rb2)
    i32 = dict(dtype=torch.int32, device="cuda")
    d_keys, d_counts, d_act = torch.zeros((B, CAP), **i32), torch.zeros(B, **i32), torch.full((B,), 77, **i32)
    d_vals, d_pov = torch.zeros((B, CAP), device="cuda"), torch.zeros((B, 160), device="cuda")
    d_probs, d_value, d_rew = _filled((B, 9)), _filled((B,)), torch.zeros(B, device="cuda")
    d_cmd = torch.zeros(B, dtype=torch.uint8, device="cuda")
    d_selected = torch.ones(B, dtype=torch.uint8, device="cuda")  # every game is new at the first tick
    lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
    torch.cuda.synchronize()
    for tick in range(T):
        sim.observe_sparse_device(*lists)
        net.predict_sparse(*lists, B, d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr(), seed=9, d_action_ptr=d_act.data_ptr(),
                           d_reset_mask_ptr=d_selected.data_ptr())
        sim.synchronize(), net.synchronize()  # (three objects, three streams)
        rb.record(d_probs.data_ptr(), d_value.data_ptr(), d_act.data_ptr(), d_rew.data_ptr(), *lists, d_reset_mask_ptr=d_selected.data_ptr())
        rb.synchronize()
        sim.step_device(d_cmd.data_ptr(), 1)
        sim.reset_arenas(done=True, max_steps=10, selected_ptr=d_selected.data_ptr())
        sim.synchronize()
    assert rb.status() == (B, 0, 0) and net.sparse_overflows() == 0
    first = rb.first.cpu().numpy()
    assert (first[0] == 1).all() and set(np.unique(first)) == {0, 1}
    inside = first[1:].sum(axis=0)
    print("closed loop: game ends inside the block per agent: min %d max %d" % (inside.min(), inside.max()))
    assert inside.min() >= 5
    p2, v2 = _filled((B, 9)), _filled((B,))
    for t in range(T):
        net2.reset_memory(rb.first[t].data_ptr(), agents=B)
        net2.forward_sparse(*rb.state(t), B, p2.data_ptr(), v2.data_ptr())
        net2.update_actions(rb.action[t].data_ptr(), B)
        net2.synchronize()
        rb2.record(p2.data_ptr(), v2.data_ptr(), rb.action[t].data_ptr(), d_rew.data_ptr(), d_reset_mask_ptr=rb.first[t].data_ptr())
        rb2.synchronize()
    assert net2.sparse_overflows() == 0
    for name in ("logp", "value", "first", "action"):
        assert np.array_equal(_bits(getattr(rb2, name)), _bits(getattr(rb, name))), name
    assert (_bits(rb.value) != rr.SENTINEL).all() and len(np.unique(_bits(rb.value))) > T
    # without the resets at the game ends the replay is another sequence: the flags matter
    net2.reset_memory()
    net2.forward_sparse(*rb.state(0), B, p2.data_ptr(), v2.data_ptr())
    net2.update_actions(rb.action[0].data_ptr(), B)
    for t in range(1, int(np.argmax(first[1:].any(axis=1))) + 2):
        net2.forward_sparse(*rb.state(t), B, p2.data_ptr(), v2.data_ptr())
        net2.update_actions(rb.action[t].data_ptr(), B)
    net2.synchronize()
    assert not np.array_equal(_bits(v2), _bits(rb.value[t]))
    for x in (net, net2, rb, rb2, sim):
        x.close()


# ---- 4: misuse ----------------------------------------------------------------------------------------------------------------
def test_gae_misuse_is_refused_and_writes_nothing():
    T, A = 4, gr.GAE_AGENTS
    rb, ready, (_, _, _, nxt, nv) = _fill_block(T)
    out = (_filled((T, A)), _filled((T, A)), _filled((T, A)))
    d_nm, d_nw, d_nv = _dev(nxt), _dev(np.zeros(A, dtype=np.int32)), _dev(nv)
    for bad in (dict(lam=1.5), dict(lam=-0.1), dict(lam=float("nan")), dict(gamma=1.01), dict(gamma=float("nan")),
                dict(next_mask=d_nm, next_words=(d_nw.data_ptr(), 1, 1)), dict(next_words=(d_nw.data_ptr(), 0, 1)),
                dict(next_words=(d_nw.data_ptr(), 1, 0)), dict(out=(None, None, None))):
        args = dict(gamma=0.99, lam=0.95, next_value=d_nv, out=out)
        args.update(bad)
        with pytest.raises(env.StrikeForceError, match=r"\(-1\)"):
            rb.gae(**args)
    io = rollout.GaeIO()
    io.gamma, io.lam, io.reward_scale, io.d_returns = 0.99, 0.95, 1.0, out[0].data_ptr()
    assert rb.L.sf_rollout_gae(None, C.byref(io)) == -1 and rb.L.sf_rollout_gae(rb.h, None) == -1
    assert rb.L.sf_rollout_continue(None, None) == -1
    rb.synchronize()
    for x in out:
        assert (_bits(x) == rr.SENTINEL).all()
    assert rb.status() == (int(ready.sum()), 0, 0)
    rb.gae(0.99, 0.95, next_value=d_nv, out=out)  # and the good call writes
    rb.synchronize()
    assert (_bits(out[0])[:, ready] != rr.SENTINEL).all()
    rb.close()
