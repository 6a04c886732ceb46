"""bot-1's reward network on the device (include/strikeforce_policy.h: sf_reward_create / sf_reward_forward /
sf_reward_sparse; strikeforce_amd.policy.RewardBatch) against the float64 form of the restatement —
oracle/policy_ref.forward_batched fed one_hot(action) as the last action, its value output being D — under the gates of
tests/reward_cases.py:
    |D - D64| <= g = 1e-6 + 5e-5 D64                                  (the project's value gate)
    |state - state64| <= 1e-5 + 5e-5 |state64|                        (its state gate)
    |r - log D64| <= g / (D64 - g) + 2^-22 |log D64|   where D64 >= 1e-3  (the value gate through the log + logf's rounding)
    r within 2 ulp of the f32 log of the device's own D; D == 0 gives -inf; nothing is NaN      (always)
tests/test_reward_ref.py proves on the CPU, for every case run here, that the f32 restatement — pinned on the reference's
compiled model — uses at most half of each gate against f64.  Every comparison below is device against f64 unless it says
"bit for bit"."""

import numpy as np
import pytest
import torch

import policy_cases as pc
import reward_cases as rc
from strikeforce_amd import config, env, policy

pytestmark = pytest.mark.gpu

ENV_NAMES = ("SF_POLICY_LAYERED", "SF_POLICY_FUSED_TAIL", "SF_POLICY_DENSE_CONV0", "SF_POLICY_F32_CONV")
# path -> (environment at sf_reward_create, launches per forward as sf_policy_kernel_time_by_kernel counts them — k_gemm,
# k_gemm_b3, the launch that takes the non-zeros, k_tail — for the dense entry, for the list entry).  Separate tail: gru0's
# and gru1's paired products, combined_processor and the three ResB layers of the one head = 6 k_gemm launches and no k_tail;
# layered form: conv1 + conv2 = 2 k_gemm launches, conv0 on a list is the timed launch that takes the non-zeros.
PATHS = {
    "composed+fused": ({}, (0, 0, 1, 1), (0, 0, 1, 1)),
    "layered+fused": ({"SF_POLICY_LAYERED": "1"}, (2, 0, 0, 1), (2, 0, 1, 1)),
    "composed+separate": ({"SF_POLICY_FUSED_TAIL": "0"}, (6, 0, 1, 0), None),
}
FILL_BITS = 0x7FC0DEAD  # a quiet NaN nobody computes: what an output row nobody may write still has to hold
CAP = 2048


def _select(monkeypatch, name):
    for n in ENV_NAMES:
        monkeypatch.delenv(n, raising=False)
    for k, v in PATHS[name][0].items():
        monkeypatch.setenv(k, v)
    return name


@pytest.fixture(params=["composed+fused", "layered+fused"])
def form(request, monkeypatch):
    """The two forms of the convolution stack in front of the fused tail."""
    return _select(monkeypatch, request.param)


def _dev(a):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    torch.cuda.synchronize()
    return t


def _filled(shape, dtype=torch.float32):
    return torch.full(shape, FILL_BITS, dtype=torch.int32, device="cuda").view(dtype)


def _untouched(t, first):
    return bool((t[first:].contiguous().view(torch.int32) == FILL_BITS).all().item())


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype.itemsize == 4 else x


def _memory(rb, B):
    h = np.zeros((2, B, 160), dtype=np.float32)
    a = np.zeros((B, 9), dtype=np.float32)
    for b in range(B):
        h[:, b], a[b] = rb.get_memory(b)
    return h, a


def _set_memory(rb, h, a, first=0):
    for b in range(first, h.shape[1]):
        rb.set_memory(b, h[:, b], a[b])


def _lists(obs, cap=CAP):
    return [_dev(x) for x in pc.lists_from_dense(obs, cap)]


def _sparse(rb, lists, cap, agents, d_act, d_disc, d_rew, **kw):
    rb.reward_sparse(lists[0].data_ptr(), lists[1].data_ptr(), lists[2].data_ptr(), lists[3].data_ptr(), cap, agents, d_act.data_ptr(),
                     d_disc.data_ptr() if d_disc is not None else None, d_rew.data_ptr() if d_rew is not None else None, **kw)


def _check(disc, reward, h, d64, h64, what):
    """One step of device outputs against f64 under the gates, and the reward against the device's own D; returns the
    fractions of the gates used (D, reward, state)."""
    fd, fr, fh = pc.gate_fraction(disc, d64), rc.reward_fraction(reward, d64), pc.gate_fraction(h, h64, state=True)
    ulps = rc.log_ulps(reward, disc)
    print("%s: %.3f / %.3f / %.3f of the gate (D / reward / state), log within %d ulp" % (what, fd, fr, fh, ulps))
    assert fd <= 1 and fr <= 1 and fh <= 1 and ulps <= 2, (what, fd, fr, fh, ulps)
    return fd, fr, fh


# ---- every path ------------------------------------------------------------------------------------------------------------
RUNS = [(p, e) for p in PATHS for e in ("forward", "sparse") if not (e == "sparse" and PATHS[p][2] is None)]


@pytest.mark.parametrize("key", sorted(k for k in rc.CASES if not k.startswith("partial")))
@pytest.mark.parametrize("pathname,entry", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_every_path_matches_float64(monkeypatch, pathname, entry, key):
    """Every case of tests/reward_cases.py — 30 % dense observations at 1, 17 and 33 agents, 40 recurrent steps at 1 % with
    three agents restarted in the middle, the eight edge images, and the saturated head — through sf_reward_forward
    (composed + fused tail, layered + fused tail, composed + separate tail) and sf_reward_sparse (both forms in front of
    the fused tail; the lists come with their dense rows, 30 % dense images do not fit a list): D, reward and both states of
    every agent at every step, the stored one-hot, and the launch counts that say which kernels ran.  A restart is
    sf_policy_reset_memory in front of the dense entry and the mask of the list entry."""
    _select(monkeypatch, pathname)
    case, ref = rc.CASES[key], rc.reference64(key)
    B, acts = case.B, case.actions()
    rb = policy.RewardBatch(rc.parameters(case.params), B)
    d_disc, d_rew = _filled((B,)), _filled((B,))
    rb.kernel_time_by_kernel(True)
    worst = np.zeros(3)
    for t, obs in enumerate(case.observations()):
        d_obs, d_act = _dev(obs), _dev(acts[t])
        mask = np.zeros(B, dtype=np.uint8)
        mask[list(case.resets.get(t, ()))] = 1
        d_mask = _dev(mask)
        if entry == "forward":
            if mask.any():
                rb.reset_memory(d_mask.data_ptr())
            rb.forward(d_obs.data_ptr(), d_act.data_ptr(), B, d_disc.data_ptr(), d_rew.data_ptr())
        else:
            _sparse(rb, _lists(obs), CAP, B, d_act, d_disc, d_rew, d_dense_ptr=d_obs.data_ptr(), d_reset_mask_ptr=d_mask.data_ptr())
        rb.synchronize()
        disc, rew = d_disc.cpu().numpy(), d_rew.cpu().numpy()
        hg, ag = _memory(rb, B)
        worst = np.maximum(worst, _check(disc, rew, hg, ref.disc[t], ref.h[t], "%s %s %s step %d" % (pathname, entry, key, t)))
        assert np.array_equal(ag, rc.one_hot(acts[t]))
        if key == "saturated":
            assert (disc == 0).all() and np.isneginf(rew).all()
    launches = tuple(n for (_, _, n) in rb.kernel_time_by_kernel(False))
    assert launches == tuple(case.steps * n for n in PATHS[pathname][1 if entry == "forward" else 2]), (pathname, entry, launches)
    assert rb.sparse_overflows() == 0
    print("%s %s %s: %.3f / %.3f / %.3f of the gate (D / reward / state)" % ((pathname, entry, key) + tuple(worst)))
    rb.close()


# ---- the action ------------------------------------------------------------------------------------------------------------
def test_the_action_given_is_the_one_hot_of_this_tick(form):
    """Agents 0..8 are given actions 0..8, agents 9 and 10 the indices -1 and 9 on agent 0's observation and memory: they
    equal agent 0 bit for bit ("no action").  Two steps, the second from a running memory.  The reward object fed action a
    equals — D and both states, under the gate around f64 — a policy object (same parameters) whose memory was set to
    that one-hot in front of sf_policy_forward (different bits are allowed: the tile schedules differ); it stores the
    one-hot given whatever was stored, a policy forward leaves the stored one alone."""
    B = 11
    params = rc.parameters("gain-3")
    rng = np.random.default_rng(61)
    given = np.array(list(range(9)) + [-1, 9], dtype=np.int32)
    meant = np.where((given >= 0) & (given < 9), given, 0)
    rb, pb = policy.RewardBatch(params, B), policy.PolicyBatch(params, B)
    d_disc, d_rew, d_probs, d_value = _filled((B,)), _filled((B,)), _filled((B, 9)), _filled((B,))
    h = pc.fresh_memory(B)[0]
    for t in range(2):
        obs = pc.obs_sparse1(rng, B)
        obs[9:] = obs[0]
        if t == 1:
            h = np.array(hr)
            h[:, 9:] = h[:, :1]
            _set_memory(rb, h, rc.one_hot((meant + 4) % 9))  # (another action is stored: it must not be read)
        d64, _, h64 = rc.step_reference(params, obs, h, meant, torch.float64)
        d_obs, d_act = _dev(obs), _dev(given)
        rb.forward(d_obs.data_ptr(), d_act.data_ptr(), B, d_disc.data_ptr(), d_rew.data_ptr())
        _set_memory(pb, h, rc.one_hot(meant))
        pb.forward(d_obs.data_ptr(), B, d_probs.data_ptr(), d_value.data_ptr())
        rb.synchronize(), pb.synchronize()
        disc, rew, value = d_disc.cpu().numpy(), d_rew.cpu().numpy(), d_value.cpu().numpy()
        (hr, ar), (hp, ap) = _memory(rb, B), _memory(pb, B)
        _check(disc, rew, hr, d64, h64, "%s action step %d" % (form, t))
        assert pc.gate_fraction(value, d64) <= 1 and pc.gate_fraction(hp, h64, state=True) <= 1
        assert (np.abs(disc.astype(np.float64) - value) <= pc.gate(d64)).all()
        assert (np.abs(hr.astype(np.float64) - hp) <= pc.gate(h64, state=True)).all()
        assert np.array_equal(ar, rc.one_hot(meant)) and np.array_equal(ap, rc.one_hot(meant))
        for b in (9, 10):
            assert _bits(disc)[b] == _bits(disc)[0] and _bits(rew)[b] == _bits(rew)[0] and np.array_equal(_bits(hr[:, b]), _bits(hr[:, 0]))
    rb.close(), pb.close()


# ---- lists -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [2048, 130])
def test_lists_equal_the_dense_image_bit_for_bit(form, cap):
    """One agent each with 0, 1, 63, 64, 65, 128, 129, cap and cap + 1 non-zeros, one with the 0xffffffff marker, and the
    images that lie in one pair of channels / change pair at every entry; two recurrent steps.  sf_reward_sparse equals
    sf_reward_forward on the dense image bit for bit — D, reward, state — for every agent whose list fits, and counts the
    others exactly; with d_dense it equals the dense call bit for bit for ALL agents and counts nothing.  The dense call
    itself is held to f64."""
    rng = np.random.default_rng(cap + 1)
    e = pc.edge_images()
    sizes = [0, 1, 63, 64, 65, 128, 129, cap, cap + 1, 200]
    obs = np.stack([pc.obs_with_count(rng, n) for n in sizes] + [e[4], e[5], e[6]])
    B, MARKED = len(obs), 9
    keys, vals, counts, pov = pc.lists_from_dense(obs, cap)
    assert counts[:10].tolist() == sizes
    counts[MARKED] = 0xFFFFFFFF
    fits = (counts <= cap) & (counts != 0xFFFFFFFF)
    assert (~fits).sum() == (2 if cap == 2048 else 3) and fits[7] and not fits[8]
    params = rc.parameters("gain-1")
    dense, sparse, either = (policy.RewardBatch(params, B) for _ in range(3))
    fallback = obs.copy()
    fallback[fits] = np.nan  # rows nobody may read
    d_obs, d_fallback = _dev(obs), _dev(fallback)
    lists = [_dev(keys), _dev(vals), _dev(counts), _dev(pov)]
    out = [(_filled((B,)), _filled((B,))) for _ in range(3)]
    h = pc.fresh_memory(B)[0]
    for step in range(2):
        acts = rng.integers(0, 9, size=B).astype(np.int32)
        d_act = _dev(acts)
        dense.forward(d_obs.data_ptr(), d_act.data_ptr(), B, out[0][0].data_ptr(), out[0][1].data_ptr())
        _sparse(sparse, lists, cap, B, d_act, out[1][0], out[1][1])
        _sparse(either, lists, cap, B, d_act, out[2][0], out[2][1], d_dense_ptr=d_fallback.data_ptr())
        for x in (dense, sparse, either):
            x.synchronize()
        d, r = [_bits(o[0].cpu().numpy()) for o in out], [_bits(o[1].cpu().numpy()) for o in out]
        hd, hs, he = (_memory(x, B)[0] for x in (dense, sparse, either))
        for b in np.flatnonzero(fits):
            assert d[1][b] == d[0][b] and r[1][b] == r[0][b] and np.array_equal(_bits(hs[:, b]), _bits(hd[:, b])), (step, b)
        assert np.array_equal(d[2], d[0]) and np.array_equal(r[2], r[0]) and np.array_equal(_bits(he), _bits(hd)), step
        assert sparse.sparse_overflows() == int((~fits).sum()) and sparse.sparse_overflows() == 0
        assert either.sparse_overflows() == 0
        d64, _, h64 = rc.step_reference(params, obs, h, acts, torch.float64)
        _check(out[0][0].cpu().numpy(), out[0][1].cpu().numpy(), hd, d64, h64, "%s lists cap %d step %d" % (form, cap, step))
        h = hd  # (the device's own state goes on: one step of error at a time)
    for x in (dense, sparse, either):
        x.close()


# ---- partial batches -------------------------------------------------------------------------------------------------------
GROUP, STRIDE = 2, 3  # the words form: agent a reads word (a // GROUP) * STRIDE


@pytest.mark.parametrize("agents", rc.PARTIAL_AGENTS)
def test_partial_batches_stay_inside_their_rows(form, agents):
    """A reward object of 64 agents asked for fewer, every agent holding a running agent's state and some stored action,
    both outputs 64 rows of a NaN pattern, every input 64 valid rows.  For sf_reward_forward and for sf_reward_sparse with
    the restart flags as a mask and as words (reset_group 2, stride 3): rows < agents meet the gates against f64 and equal
    BIT FOR BIT what an object of exactly `agents` agents returns; rows >= agents of both outputs still hold the pattern;
    state and stored action of agents >= agents are exactly what was set.  Every flag from `agents` on — mask bytes, the
    words of later groups, the words between the strides — is set: a kernel that looked there would wipe those agents.
    k_tail's ragged last workgroup (agents % 16 != 0) computes its missing rows on the last agent and stores nothing."""
    N = rc.PARTIAL_MAX
    params = rc.parameters("gain-1")
    case = rc.CASES["partial/gain-1"]
    ref, ref_restarted = rc.reference64("partial/gain-1"), rc.reference64("partial-restarted/gain-1")
    obs, acts, h0 = case.observations()[0], case.actions()[0], case.memory()
    a0 = rc.one_hot((acts + 5) % 9)  # what is stored before the call: never the action given
    rows = slice(0, agents)
    big, exact = policy.RewardBatch(params, N), policy.RewardBatch(params, agents)
    d_obs, d_act, lists = _dev(obs), _dev(acts), _lists(obs)
    restarted = [b for b in rc.PARTIAL_RESET if b < agents]
    mask = np.ones(N, dtype=np.uint8)
    mask[:agents] = 0
    mask[restarted] = 1
    d_mask = _dev(mask)
    groups = sorted({b // GROUP for b in rc.PARTIAL_RESET})
    words = np.ones(((N + GROUP - 1) // GROUP) * STRIDE, dtype=np.int32)
    for g in range((agents + GROUP - 1) // GROUP):  # the groups this call reads: clear unless restarted
        words[g * STRIDE] = 7 if g in groups else 0
    d_words = _dev(words)
    by_words = [b for b in range(N) if b // GROUP in groups]
    hw = np.array(h0)
    hw[:, by_words] = 0
    dw64, _, hw64 = rc.step_reference(params, obs, hw, acts, torch.float64)

    def both(call):
        _set_memory(big, h0, a0)
        _set_memory(exact, h0[:, rows], a0[rows])
        ob, oe = (_filled((N,)), _filled((N,))), (_filled((agents,)), _filled((agents,)))
        call(big, ob), call(exact, oe)
        big.synchronize(), exact.synchronize()
        (hb, ab), (he, ae) = _memory(big, N), _memory(exact, agents)
        for i in range(2):
            assert np.array_equal(_bits(ob[i][rows].cpu().numpy()), _bits(oe[i].cpu().numpy())) and _untouched(ob[i], agents), i
        assert np.array_equal(_bits(hb[:, rows]), _bits(he)) and np.array_equal(ab[rows], ae)
        assert np.array_equal(_bits(hb[:, agents:]), _bits(h0[:, agents:])) and np.array_equal(ab[agents:], a0[agents:])
        assert np.array_equal(ab[rows], rc.one_hot(acts[rows]))
        return ob[0][rows].cpu().numpy(), ob[1][rows].cpu().numpy(), hb[:, rows]

    d, r, h = both(lambda x, o: x.forward(d_obs.data_ptr(), d_act.data_ptr(), agents, o[0].data_ptr(), o[1].data_ptr()))
    _check(d, r, h, ref.disc[0][rows], ref.h[0][:, rows], "%s forward, %d of %d" % (form, agents, N))
    d, r, h = both(lambda x, o: _sparse(x, lists, CAP, agents, d_act, o[0], o[1], d_reset_mask_ptr=d_mask.data_ptr()))
    _check(d, r, h, ref_restarted.disc[0][rows], ref_restarted.h[0][:, rows], "%s sparse + mask, %d of %d" % (form, agents, N))
    d, r, h = both(lambda x, o: _sparse(x, lists, CAP, agents, d_act, o[0], o[1], reset_words=(d_words.data_ptr(), STRIDE, GROUP)))
    _check(d, r, h, dw64[rows], hw64[:, rows], "%s sparse + words, %d of %d" % (form, agents, N))
    if restarted:  # (a restarted agent's D differs from the running agent's: the flags below `agents` were read)
        assert np.abs(ref_restarted.disc[0][restarted] - ref.disc[0][restarted]).max() > 1e-4
    assert big.sparse_overflows() == 0
    big.close(), exact.close()


# ---- the pair as it is used ------------------------------------------------------------------------------------------------
def test_policy_and_reward_in_the_closed_loop(monkeypatch):
    """6 arenas of BASELINE configs[2], 30 steps of observe-sparse, sf_policy_predict_sparse, sf_reward_sparse (reading that
    call's d_action and the same restart words, sf_done_view_device), step, nothing synchronised in between.  The
    observations, actions and restart flags of every step are recorded on the side; a second reward object replays them
    through sf_policy_reset_memory_n + sf_reward_forward: D, reward and the final state equal bit for bit (composed form)."""
    _select(monkeypatch, "composed+fused")
    w = config.baseline_workload("C3", arenas=6)
    sim = env.ArenaBatch(w)
    sim.reset(*w.seeds())
    B = w.cfg.arenas * w.cfg.n_agents
    net = policy.PolicyBatch(pc.parameters("gain-1"), B)
    rew, replay = policy.RewardBatch(rc.parameters("gain-3"), B), policy.RewardBatch(rc.parameters("gain-3"), B)
    i32 = dict(dtype=torch.int32, device="cuda")
    d_keys, d_counts, d_act = torch.zeros((B, CAP), **i32), torch.zeros(B, **i32), torch.full((B,), 77, **i32)
    d_vals, d_pov = torch.zeros((B, CAP), device="cuda"), torch.zeros((B, 160), device="cuda")
    d_dense, d_obs = torch.zeros((B, 32, 31, 31), device="cuda"), torch.zeros((B, 32, 31, 31), device="cuda")
    d_probs, d_value, d_disc, d_rew = _filled((B, 9)), _filled((B,)), _filled((B,)), _filled((B,))
    d_cmd, d_mask = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")
    words = sim.done_view_device()
    rec = []
    for t in range(30):
        sim.observe_sparse_device(d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
        sim.observe_overflow_device(d_counts.data_ptr(), CAP, d_dense.data_ptr(), d_pov.data_ptr())
        net.predict_sparse(d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP, B, d_probs.data_ptr(), d_value.data_ptr(),
                           d_cmd.data_ptr(), seed=5, d_action_ptr=d_act.data_ptr(), d_dense_ptr=d_dense.data_ptr(), reset_words=words)
        _sparse(rew, [d_keys, d_vals, d_counts, d_pov], CAP, B, d_act, d_disc, d_rew, d_dense_ptr=d_dense.data_ptr(), reset_words=words)
        sim.observe_device(d_obs.data_ptr())  # (on the side, for the replay)
        sim.done_device(d_mask.data_ptr())
        sim.synchronize(), net.synchronize(), rew.synchronize()
        rec.append((d_obs.clone(), d_act.clone(), d_mask.clone(), d_disc.cpu().numpy(), d_rew.cpu().numpy()))
        assert np.array_equal(_memory(rew, B)[1], _memory(net, B)[1])  # both hold the one-hot of the action just drawn
        sim.step_device(d_cmd.data_ptr(), 1)
    restarts, actions = 0, set()
    d_disc2, d_rew2 = _filled((B,)), _filled((B,))
    for t, (obs, act, mask, disc, reward) in enumerate(rec):
        assert rc.log_ulps(reward, disc) <= 2 and 0 <= int(act.min()) and int(act.max()) < 9
        replay.reset_memory(mask.data_ptr(), agents=B)
        replay.forward(obs.data_ptr(), act.data_ptr(), B, d_disc2.data_ptr(), d_rew2.data_ptr())
        replay.synchronize()
        assert np.array_equal(_bits(d_disc2.cpu().numpy()), _bits(disc)) and np.array_equal(_bits(d_rew2.cpu().numpy()), _bits(reward)), t
        restarts += int(mask.sum().item())
        actions |= set(act.cpu().numpy().tolist())
    (h1, a1), (h2, a2) = _memory(rew, B), _memory(replay, B)
    assert np.array_equal(_bits(h1), _bits(h2)) and np.array_equal(a1, a2)
    assert len(actions) > 1 and rew.sparse_overflows() == 0
    print("closed loop: %d agents x 30 steps, %d restarts, actions %s, mean reward %.4f" % (B, restarts, sorted(actions), float(np.mean([r[4].mean() for r in rec]))))
    for x in (net, rew, replay, sim):
        x.close()


# ---- the committed reference vectors ---------------------------------------------------------------------------------------
def test_committed_reference_vectors_are_reproduced(form):
    """tests/golden/reward_vectors.json: D and log D of the reference's compiled model (8 agents x 6 steps, two parameter
    sets, two agents restarted in front of step 3), regenerated here from the recorded seeds and run through
    sf_reward_sparse: D under the value gate, log D under the reward gate, the state's checksum within the gate's RTOL."""
    import json
    import os
    import sys
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    sys.path.insert(0, golden)
    import make_reward_vectors as gen
    have = json.load(open(os.path.join(golden, "reward_vectors.json")))
    obs, acts = gen.trajectory()
    B = have["agents"]
    assert [have["obs_seed"], have["action_seed"], have["reset_at"], have["reset"]] == [gen.OBS_SEED, gen.ACTION_SEED, gen.RESET_AT, list(gen.RESET)]
    for s in have["sets"]:
        assert s["init_parameters"] == rc.PARAM_SETS[s["params"]] and s["actions"] == acts.tolist()
        rb = policy.RewardBatch(rc.parameters(s["params"]), B)
        d_disc, d_rew = _filled((B,)), _filled((B,))
        for t, step in enumerate(s["steps"]):
            assert int((obs[t] != 0).sum()) == s["obs_nonzero"][t]
            mask = np.zeros(B, dtype=np.uint8)
            if t == have["reset_at"]:
                mask[have["reset"]] = 1
            d_mask, d_act = _dev(mask), _dev(acts[t].astype(np.int32))
            _sparse(rb, _lists(obs[t]), CAP, B, d_act, d_disc, d_rew, d_reset_mask_ptr=d_mask.data_ptr())
            rb.synchronize()
            disc, rew = d_disc.cpu().numpy(), d_rew.cpu().numpy()
            want = np.array(step["disc"])
            fd, fr = pc.gate_fraction(disc, want), rc.reward_fraction(rew, want)
            print("%s %s step %d: %.3f / %.3f of the gate (D / reward)" % (form, s["params"], t, fd, fr))
            assert want.min() >= rc.D_FLOOR and fd <= 1 and fr <= 1 and rc.log_ulps(rew, disc) <= 2
            hs = [float(np.abs(_memory(rb, B)[0][g]).sum()) for g in range(2)]
            np.testing.assert_allclose(hs, step["h_abs_sum"], rtol=pc.RTOL)
        rb.close()


# ---- misuse ----------------------------------------------------------------------------------------------------------------
def test_misuse_is_refused(monkeypatch):
    """A policy entry on a reward object and a reward entry on a policy object are SF_ERR_STATE with a message; both
    outputs NULL, a NULL action and cap > SF_POLICY_LIST_MAX are SF_ERR_ARG; one output alone is allowed and holds the same
    bits; the list entry refuses the separate tail in sf_policy_forward_sparse's words.  Nothing refused touches memory."""
    _select(monkeypatch, "composed+fused")
    B = 5
    params = rc.parameters("gain-1")
    rb, pb = policy.RewardBatch(params, B), policy.PolicyBatch(params, B)
    obs = pc.obs_sparse1(np.random.default_rng(8), B)
    d_obs, d_act, lists = _dev(obs), _dev(np.arange(B, dtype=np.int32)), _lists(obs)
    d_disc, d_rew, d_probs, d_value = _filled((B,)), _filled((B,)), _filled((B, 9)), _filled((B,))
    d_cmd = torch.zeros(B, dtype=torch.uint8, device="cuda")
    P, R = policy.PolicyBatch, policy.RewardBatch
    la = [x.data_ptr() for x in lists]
    on_reward = [lambda: P.forward(rb, d_obs.data_ptr(), B, d_probs.data_ptr(), d_value.data_ptr()),
                 lambda: P.forward_sparse(rb, la[0], la[1], la[2], la[3], CAP, B, d_probs.data_ptr(), d_value.data_ptr()),
                 lambda: P.forward_sparse(rb, la[0], la[1], la[2], la[3], CAP, B, d_probs.data_ptr(), d_value.data_ptr(), d_dense_ptr=d_obs.data_ptr()),
                 lambda: P.predict_sparse(rb, la[0], la[1], la[2], la[3], CAP, B, d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr()),
                 lambda: P.act(rb, d_probs.data_ptr(), B, d_cmd.data_ptr()),
                 lambda: P.features(rb, d_obs.data_ptr(), B, d_probs.data_ptr())]
    for call in on_reward:
        with pytest.raises(env.StrikeForceError, match=r"\(-4\).*is a reward model"):
            call()
    for call in (lambda: R.forward(pb, d_obs.data_ptr(), d_act.data_ptr(), B, d_disc.data_ptr(), d_rew.data_ptr()),
                 lambda: R.reward_sparse(pb, la[0], la[1], la[2], la[3], CAP, B, d_act.data_ptr(), d_disc.data_ptr(), d_rew.data_ptr())):
        with pytest.raises(env.StrikeForceError, match=r"\(-4\).*is a policy"):
            call()
    with pytest.raises(env.StrikeForceError, match=r"\(-1\).*null buffer"):
        rb.forward(d_obs.data_ptr(), d_act.data_ptr(), B, None, None)
    with pytest.raises(env.StrikeForceError, match=r"\(-1\).*null buffer"):
        rb.forward(d_obs.data_ptr(), None, B, d_disc.data_ptr(), d_rew.data_ptr())
    with pytest.raises(env.StrikeForceError, match=r"\(-1\).*null buffer"):
        _sparse(rb, lists, CAP, B, d_act, None, None)
    with pytest.raises(env.StrikeForceError, match=r"\(-1\).*cap above SF_POLICY_LIST_MAX"):
        _sparse(rb, lists, CAP + 1, B, d_act, d_disc, d_rew)
    with pytest.raises(env.StrikeForceError, match=r"\(-1\).*agents out of range"):
        rb.forward(d_obs.data_ptr(), d_act.data_ptr(), B + 1, d_disc.data_ptr(), d_rew.data_ptr())
    rb.synchronize(), pb.synchronize()
    assert all(_untouched(x, 0) for x in (d_disc, d_rew, d_probs, d_value))
    h, a = _memory(rb, B)
    assert not h.any() and np.array_equal(a, rc.one_hot([0] * B))  # as after reset_memory(): nothing ran
    # one output alone
    one, two = policy.RewardBatch(params, B), policy.RewardBatch(params, B)
    rb.forward(d_obs.data_ptr(), d_act.data_ptr(), B, d_disc.data_ptr(), d_rew.data_ptr())
    only_d, only_r = _filled((B,)), _filled((B,))
    one.forward(d_obs.data_ptr(), d_act.data_ptr(), B, only_d.data_ptr(), None)
    _sparse(two, lists, CAP, B, d_act, None, only_r)
    for x in (rb, one, two):
        x.synchronize()
    assert np.array_equal(_bits(only_d.cpu().numpy()), _bits(d_disc.cpu().numpy())) and np.array_equal(_bits(only_r.cpu().numpy()), _bits(d_rew.cpu().numpy()))
    # the list entry needs the fused tail
    _select(monkeypatch, "composed+separate")
    sep = policy.RewardBatch(params, B)
    with pytest.raises(env.StrikeForceError, match=r"\(-4\).*sf_reward_sparse needs the fused tail \(SF_POLICY_FUSED_TAIL=0 is set\)"):
        _sparse(sep, lists, CAP, B, d_act, d_disc, d_rew)
    for x in (rb, pb, one, two, sep):
        x.close()
