"""The continuing rollout buffer and sf_rollout_gae restated (include/strikeforce_policy.h; strikeforce_amd/rollout.py), no GPU.

(a) Bookkeeping: `RefRolloutCont` keeps rollout_ref.RefRollout's per-agent lists under the continuing rule — a full buffer
    drops the tick, otherwise the tick is appended with first = the restart flag; a flag never clears a list.
(b) `gae_numpy`: the header's recursion in uncontracted numpy f32, sequential in the slots, agents side by side; terms are
    selected, never multiplied by 0 or 1.  `fused=` puts a fused multiply-add (emulated in f64, where a product of two f32
    is exact) at one of the recursion's four products: what a compiler's contraction would compute.
(c) `gae_delta_f64`: textbook GAE(lambda) in float64 in the delta form A_t = delta_t + gamma lambda (1 - end_t) A_{t+1}, on
    the same f32 inputs; and `gae_error_bound`, half an ulp per rounded f32 operation of (b) propagated through the recursion
    in float64."""
import numpy as np

import rollout_ref as rr

FUSED_SITES = ("gamma", "scale", "mix_v", "mix_g")


class RefRolloutCont(rr.RefRollout):
    def __init__(self, agents, T, list_cap, **kw):
        super().__init__(agents, T, list_cap, **kw)
        self.image["first"] = np.full((T, agents), rr.SENTINEL_U8, dtype=np.uint8)

    def record(self, tick, probs, value, action, reward, reset=None, **kw):
        for a in range(len(value)):
            t = len(self.lists[a])
            if t < self.T:  # (a ready agent drops the tick: its flag is not stored anywhere)
                self.image["first"][t, a] = 1 if (reset is not None and reset[a]) else 0
        super().record(tick, probs, value, action, reward, reset=None, **kw)  # no list is ever cleared by a flag

    def first_of(self, a):
        return [int(self.image["first"][t, a]) for t in range(len(self.lists[a]))]


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def _ends(first, next_end, T, n):
    """end[t] = first[t + 1]; end[T - 1] = the next tick's flag."""
    end = np.zeros((T, n), dtype=bool)
    if first is not None:
        end[:-1] = np.asarray(first).reshape(T, n)[1:] != 0
    if next_end is not None:
        end[T - 1] = np.asarray(next_end).reshape(n) != 0
    return end


def gae_numpy(reward, value, first, gamma, lam, reward_scale=1.0, log_values=False, next_value=None, next_end=None, fused=None):
    """-> (returns, v, adv), [T][n] f32.  reward, value [T][n]; first [T][n] or None; next_value [n] or None; next_end [n]
    or None."""
    r, val = _f32(reward), _f32(value)
    T = r.shape[0]
    r, val = r.reshape(T, -1), val.reshape(T, -1)
    n = r.shape[1]
    g, lm, sc = np.float32(gamma), np.float32(lam), np.float32(reward_scale)
    oml = np.float32(1) - lm
    V = rr.log32(val) if log_values else val
    have = next_value is not None
    vn = (rr.log32(_f32(next_value)) if log_values else _f32(next_value)).reshape(n) if have else np.zeros(n, dtype=np.float32)
    end = _ends(first, next_end, T, n)
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    G = np.zeros(n, dtype=np.float32)
    out = np.empty((T, n), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T - 1, -1, -1):
            x = sc * r[t]
            if t == T - 1 or lm == 0:
                boot = vn
            elif lm == 1:
                boot = G
            else:
                pv, pg = oml * vn, lm * G
                if fused == "mix_v":
                    boot = (f64(oml) * f64(vn) + f64(pg)).astype(np.float32)
                elif fused == "mix_g":
                    boot = (f64(lm) * f64(G) + f64(pv)).astype(np.float32)
                else:
                    boot = pv + pg
            if fused == "gamma":
                s = (f64(g) * f64(boot) + f64(x)).astype(np.float32)
            elif fused == "scale":
                s = (f64(g * boot) + f64(sc) * f64(r[t])).astype(np.float32)
            else:
                s = g * boot + x
            cut = end[t] | (not have and t == T - 1)
            G = np.where(cut, x, s).astype(np.float32)
            out[t] = G
            vn = V[t]
        adv = out - V
    return out.reshape(np.shape(reward)), V.reshape(np.shape(reward)), adv.reshape(np.shape(reward))


def gae_delta_f64(reward, value, first, gamma, lam, reward_scale=1.0, next_value=None, next_end=None):
    """Textbook GAE(lambda), float64, finite inputs: delta_t = x_t + gamma (1 - end_t) V_{t+1} - V_t,
    A_t = delta_t + gamma lambda (1 - end_t) A_{t+1}; without a next value the last slot ends the sum.  gamma, lambda and
    reward_scale are the f32 numbers the device is given.  -> (A + V, V, A)."""
    r, V = np.asarray(_f32(reward), dtype=np.float64), np.asarray(_f32(value), dtype=np.float64)
    T = r.shape[0]
    r, V = r.reshape(T, -1), V.reshape(T, -1)
    n = r.shape[1]
    g, lm, sc = float(np.float32(gamma)), float(np.float32(lam)), float(np.float32(reward_scale))
    cont = 1.0 - _ends(first, next_end, T, n).astype(np.float64)
    if next_value is None:
        cont[T - 1] = 0.0
        vT = np.zeros(n)
    else:
        vT = np.asarray(_f32(next_value), dtype=np.float64).reshape(n)
    A = np.zeros((T + 1, n))
    Vx = np.concatenate([V, vT[None]], axis=0)
    for t in range(T - 1, -1, -1):
        delta = sc * r[t] + g * cont[t] * Vx[t + 1] - V[t]
        A[t] = delta + g * lm * cont[t] * A[t + 1]
    A = A[:T]
    return (A + V).reshape(np.shape(reward)), V.reshape(np.shape(reward)), A.reshape(np.shape(reward))


def gae_error_bound(reward, value, first, gamma, lam, reward_scale=1.0, next_value=None, next_end=None):
    """How far (b)'s f32 returns and advantages can lie from the exact recursion on the same inputs: every f32 operation of
    (b) rounds to nearest, so it adds at most u = 2^-24 times the magnitude of its own result (half an ulp); an operand's
    error passes through a product scaled by the other factor and through a sum unchanged.  (1 - lambda) is rounded too.
    Magnitudes are (b)'s own f32 results plus the error bound so far.  -> (bound on returns, bound on adv), [T][n] f64."""
    u = 2.0 ** -24
    r, V = np.asarray(_f32(reward), dtype=np.float64), np.asarray(_f32(value), dtype=np.float64)
    T = r.shape[0]
    r, V = r.reshape(T, -1), V.reshape(T, -1)
    n = r.shape[1]
    g, lm, sc = float(np.float32(gamma)), float(np.float32(lam)), float(np.float32(reward_scale))
    oml = float(np.float32(1) - np.float32(lam))
    e_oml = u * abs(oml) if lm not in (0.0, 1.0) else 0.0
    have = next_value is not None
    end = _ends(first, next_end, T, n)
    G32 = np.asarray(gae_numpy(reward, value, first, gamma, lam, reward_scale, False, next_value, next_end)[0], dtype=np.float64).reshape(T, n)
    vn = np.asarray(_f32(next_value), dtype=np.float64).reshape(n) if have else np.zeros(n)
    E = np.zeros(n)
    eg, ea = np.zeros((T, n)), np.zeros((T, n))
    for t in range(T - 1, -1, -1):
        x = sc * r[t]
        e_x = u * np.abs(x)
        if t == T - 1 or lm == 0.0:
            boot, e_boot = vn, np.zeros(n)
        elif lm == 1.0:
            boot, e_boot = G32[t + 1], E
        else:
            pv, pg = oml * vn, lm * G32[t + 1]
            e_pv = e_oml * np.abs(vn) + u * (np.abs(pv) + e_oml * np.abs(vn))
            e_pg = lm * E + u * (np.abs(pg) + lm * E)
            boot = pv + pg
            e_boot = e_pv + e_pg + u * (np.abs(boot) + e_pv + e_pg)
        y = g * boot
        e_y = g * e_boot + u * (np.abs(y) + g * e_boot)
        e_s = e_y + e_x + u * (np.abs(y + x) + e_y + e_x)
        cut = end[t] | (not have and t == T - 1)
        E = np.where(cut, e_x, e_s)
        eg[t] = E
        ea[t] = E + u * (np.abs(G32[t] - V[t]) + E)
        vn = V[t]
    return eg.reshape(np.shape(reward)), ea.reshape(np.shape(reward))


# ---- the GPU test's committed inputs ------------------------------------------------------------------------------------------
GAE_AGENTS = rr.RETURNS_AGENTS
GAE_T = rr.RETURNS_T
GAE_GAMMAS = (0.99, 0.5)
GAE_LAMBDAS = (1.0, 0.0, 0.95)
NOT_READY = (3, 64, 129)


def gae_case(T, agents=GAE_AGENTS):
    """rollout_ref.returns_case's rewards, values and actions with game ends by agent % 8: 0 none; 1 first[1]; 2 first[T / 2];
    3 first[T - 1]; 4 the next tick's flag; 5 first[T / 2] and first[T / 2 + 1] (adjacent, where T has the room); 6 random,
    one in five; 7 first[0] (which belongs to the block before: it cuts nothing) and random.  Agents 2 and 10 have a game end
    at first[T / 2]: agent 2 also a reward of -inf at slot T / 2 (returns_case puts agent 1's there, beside first[1]), agent
    10 a value of 0 at slot T / 2 (agent 2's is moved to it).  -> rewards, values, actions, first [T][agents] u8, next flags
    [agents] u8, next values [agents] in (0, 1)."""
    rewards, values, actions = rr.returns_case(T, agents=agents)
    rng = np.random.default_rng(4242 + T)
    values[T // 2, 2] = rng.uniform(1e-3, 1.0)
    rewards[T // 2, 2] = -np.inf
    values[T // 2, 10] = 0.0
    first = np.zeros((T, agents), dtype=np.uint8)
    nxt = np.zeros(agents, dtype=np.uint8)
    rnd = (rng.random((T, agents)) < 0.2).astype(np.uint8)
    for a in range(agents):
        k = a % 8
        if k == 1:
            first[1, a] = 1
        elif k == 2:
            first[T // 2, a] = 1
        elif k == 3:
            first[T - 1, a] = 1
        elif k == 4:
            nxt[a] = 1
        elif k == 5:
            first[T // 2, a] = 1
            if T // 2 + 1 < T:
                first[T // 2 + 1, a] = 1
        elif k == 6:
            first[:, a] = rnd[:, a]
        elif k == 7:
            first[:, a] = rnd[:, a]
            first[0, a] = 1
    next_values = rng.uniform(1e-3, 1.0, size=agents).astype(np.float32)
    return rewards, values, actions, first, nxt, next_values
