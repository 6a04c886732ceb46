"""sf_policy_act_masked on the MI355X (k_act_masked), exactly: with every bit set it is sf_policy_act bit for bit (command,
action, action_input and the next call's draws, greedy and sampled); with random masks, single-bit masks and the word 0 it
equals a numpy float32 restatement of the pick (the same order of additions, the same hash); d_probs_out is exact, sums to 1
within one rounding per entry and is zero exactly where masked; d_action and d_probs_out may each be NULL.  Then a closed loop
of 40 ticks over 17 agents of a 16-agent Battle (the library commands at most 16 humans per arena: the seventeenth is the
first agent of a second arena): no drawn command ever has a clear bit in the mask it was drawn under."""
import numpy as np
import pytest

import action_mask_cases as mc
from strikeforce_amd import env, policy

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

M64 = (1 << 64) - 1
ALL = (1 << 9) - 1
f32 = np.float32


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def pick_ref(p, mask, seed, draw, greedy, a):
    """act_pick_masked (csrc/sf_policy_mask.hpp) in numpy float32, operation for operation -> (pick, v / tot)."""
    v = p.astype(f32).copy()
    sc = f32(0.5) / f32(f32(f32(1.0) - v[0]) + f32(1e-5))
    for k in range(1, 9):
        v[k] = f32(v[k] * sc)
    v[0] = f32(0.5)
    for k in range(1, 9):
        if not (mask >> k) & 1:
            v[k] = f32(0.0)
    tot = f32(0.0)
    for k in range(9):
        tot = f32(tot + v[k])
    if greedy:
        pick = 0
        for k in range(1, 9):
            if v[k] > v[pick]:
                pick = k
    else:
        r = mix64((mix64(seed ^ mix64(a)) + draw) & M64)
        u = f32(f32(f32(r >> 40) * f32(1.0 / 16777216.0)) * tot)
        c, pick = f32(0.0), 8
        for k in range(8):
            c = f32(c + v[k])
            if u < c:
                pick = k
                break
    return pick, (v / tot).astype(f32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def some_probs(B, seed):
    rng = np.random.RandomState(seed)
    p = rng.gamma(0.7, size=(B, 9)).astype(np.float32)
    p[::7, 0] = 0  # v[0] = 0 and v[0] large
    p = (p / p.sum(axis=1, keepdims=True)).astype(np.float32)
    p[3::11] = np.eye(9, dtype=np.float32)[rng.randint(0, 9, size=len(p[3::11]))]  # one-hot rows: ties at 0 for the arg-max
    return p


def memory(pb, B):
    """action_input of agents [0, B): float32 [B][9]."""
    h = torch.zeros((B, 2, policy.HIDDEN), dtype=torch.float32, device="cuda")
    a = torch.zeros((B, 9), dtype=torch.float32, device="cuda")
    rows = torch.arange(B, dtype=torch.int32, device="cuda")
    pb.memory_rows(True, h.data_ptr(), a.data_ptr(), rows.data_ptr(), B, B)
    pb.synchronize()
    return a.cpu().numpy()


class Run:
    def __init__(self, B, seed=4):
        self.B = B
        self.pb = policy.PolicyBatch(policy.init_parameters(seed), B)
        self.cmd = torch.full((B + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        self.act = torch.full((B + 4,), -7, dtype=torch.int32, device="cuda")
        self.out = torch.full((B * 9 + 4,), -7.0, dtype=torch.float32, device="cuda")

    def results(self):
        self.pb.synchronize()
        B = self.B
        cmd, act, out = self.cmd.cpu().numpy(), self.act.cpu().numpy(), self.out.cpu().numpy()
        assert (cmd[B:] == 0xA5).all() and (act[B:] == -7).all() and (out[9 * B:] == -7.0).all()
        return cmd[:B].copy(), act[:B].copy(), out[:9 * B].reshape(B, 9).copy()


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("greedy", [False, True])
def test_every_bit_set_is_sf_policy_act_bit_for_bit(B, greedy):
    p = dev(some_probs(B, 100 + B))
    a, b = Run(B), Run(B)
    full = dev(np.full(B, ALL, dtype=np.uint32).view(np.int32))
    wide = dev(np.full(B, 0xFFFFFFFF, dtype=np.uint32).view(np.int32))  # bits above the ninth are nobody's
    for call in range(3):  # the following calls' draws too: the counter advances alike
        a.pb.act(p.data_ptr(), B, a.cmd.data_ptr(), seed=11, greedy=greedy, d_action_ptr=a.act.data_ptr())
        b.pb.act_masked(p.data_ptr(), B, (full if call != 1 else wide).data_ptr(), b.cmd.data_ptr(), seed=11, greedy=greedy,
                        d_action_ptr=b.act.data_ptr(), d_probs_out_ptr=b.out.data_ptr())
        ra, rb = a.results(), b.results()
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]), call
        assert np.array_equal(memory(a.pb, B).view(np.uint32), memory(b.pb, B).view(np.uint32)), call
    # a masked call advances the counter exactly as an unmasked one: the fourth call of either, unmasked, draws alike
    a.pb.act(p.data_ptr(), B, a.cmd.data_ptr(), seed=11, greedy=greedy, d_action_ptr=a.act.data_ptr())
    b.pb.act(p.data_ptr(), B, b.cmd.data_ptr(), seed=11, greedy=greedy, d_action_ptr=b.act.data_ptr())
    assert np.array_equal(a.results()[1], b.results()[1])


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_masks_against_the_float32_restatement(B):
    probs = some_probs(B, 200 + B)
    rng = np.random.RandomState(B)
    masks = rng.randint(0, 1 << 9, size=B).astype(np.uint32)
    masks[0::5] = np.uint32(1) << rng.randint(0, 9, size=len(masks[0::5])).astype(np.uint32)  # single-bit masks
    masks[1::9] = 0                                                                            # the word 0: a dead seat
    masks[2::13] |= np.uint32(0xFFFFFE00)                                                      # stray high bits
    p, m = dev(probs), dev(masks.view(np.int32))
    r = Run(B)
    for draw, greedy in enumerate([False, True, False, False]):
        r.pb.act_masked(p.data_ptr(), B, m.data_ptr(), r.cmd.data_ptr(), seed=99, greedy=greedy, d_action_ptr=r.act.data_ptr(),
                        d_probs_out_ptr=r.out.data_ptr())
        cmd, act, out = r.results()
        mem = memory(r.pb, B)
        for a in range(B):
            pick, dist = pick_ref(probs[a], int(masks[a]), 99, draw, greedy, a)
            assert act[a] == pick, (a, draw, greedy, hex(int(masks[a])))
            assert cmd[a] == ord(policy.ACTION_STRING[pick])
            assert np.array_equal(out[a].view(np.uint32), dist.view(np.uint32)), (a, out[a], dist)
            assert mem[a].tolist() == np.eye(9, dtype=np.float32)[pick].tolist()
            allowed = int(masks[a]) | 1
            assert allowed >> pick & 1  # a masked action is never drawn
            assert all((out[a, k] == 0) == (not allowed >> k & 1 or (k > 0 and probs[a, k] == 0)) for k in range(9))
            assert abs(float(out[a].astype(np.float64).sum()) - 1.0) <= 9 * 2.0 ** -24  # one rounding per entry
        assert (act[masks == 0] == 0).all() and (cmd[masks == 0] == ord("+")).all()


def test_action_and_probs_out_may_each_be_null():
    B = 65
    probs = some_probs(B, 5)
    masks = np.random.RandomState(5).randint(0, 1 << 9, size=B).astype(np.uint32)
    p, m = dev(probs), dev(masks.view(np.int32))
    want = [pick_ref(probs[a], int(masks[a]), 3, 0, False, a)[0] for a in range(B)]
    for with_act, with_out in ((False, True), (True, False), (False, False)):
        r = Run(B)
        r.pb.act_masked(p.data_ptr(), B, m.data_ptr(), r.cmd.data_ptr(), seed=3, d_action_ptr=r.act.data_ptr() if with_act else None,
                        d_probs_out_ptr=r.out.data_ptr() if with_out else None)
        cmd, act, out = r.results()
        assert bytes(cmd.tolist()) == "".join(policy.ACTION_STRING[k] for k in want).encode()
        assert (act == want).all() if with_act else (act == -7).all()
        assert (out != -7.0).all() if with_out else (out == -7.0).all()
    with pytest.raises(env.StrikeForceError):
        r.pb.act_masked(p.data_ptr(), B, None, r.cmd.data_ptr())
    with pytest.raises(env.StrikeForceError):
        r.pb.act_masked(p.data_ptr(), B, m.data_ptr(), r.cmd.data_ptr(), action_string="+x")


def test_closed_loop_never_draws_a_masked_command():
    """observe -> forward -> mask -> masked draw -> step for 40 ticks, all on the device: no drawn command has a clear bit in
    the mask it was drawn under.  17 agents: a 16-agent Battle arena and the first agent of a second one share the batch (the
    library commands at most 16 humans per arena)."""
    w = mc.CASES[mc.NAMES.index("battle16")][1](2)  # the case's world with two arenas (auto_reset on: games restart)
    g = env.ArenaBatch(w)
    B = 2 * 16
    pb = policy.PolicyBatch(policy.init_parameters(seed=21), B)
    try:
        tb, sr = w.seeds()
        g.reset(tb, sr)
        d_obs = torch.zeros((B, 32, 31, 31), dtype=torch.float32, device="cuda")
        d_probs = torch.zeros((B, 9), dtype=torch.float32, device="cuda")
        d_value = torch.zeros(B, dtype=torch.float32, device="cuda")
        d_cmd = torch.zeros(B, dtype=torch.uint8, device="cuda")
        d_act = torch.zeros(B, dtype=torch.int32, device="cuda")
        seen = set()
        for t in range(40):
            g.observe_device(d_obs.data_ptr())
            pb.forward(d_obs.data_ptr(), B, d_probs.data_ptr(), d_value.data_ptr())
            commands, actions = g.action_mask(policy.ACTION_STRING)
            g.synchronize()  # (two streams: the mask before the draw)
            pb.act_masked(d_probs.data_ptr(), B, actions.data_ptr(), d_cmd.data_ptr(), seed=8, d_action_ptr=d_act.data_ptr())
            pb.synchronize()
            cm, ac = commands.cpu().numpy().view(np.uint32).reshape(-1), actions.cpu().numpy().view(np.uint32).reshape(-1)
            act, cmd = d_act.cpu().numpy(), d_cmd.cpu().numpy()
            for a in range(17):
                assert (ac[a] | 1) >> act[a] & 1, (t, a, hex(int(ac[a])), act[a])
                if cm[a]:
                    assert cm[a] >> mc.COMMANDS.index(chr(cmd[a])) & 1, (t, a)
                else:
                    assert cmd[a] == ord("+")  # a dead seat
            seen |= set(act[:17].tolist())
            g.step_device(d_cmd.data_ptr(), 1)
            g.synchronize()
        assert len(seen) > 3
    finally:
        g.close()
