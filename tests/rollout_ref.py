"""The rollout buffer restated (include/strikeforce_policy.h, sf_rollout_*; strikeforce_amd/rollout.py), no GPU.

Bookkeeping: `RefRollout` keeps, per agent, the Python list the reference's Agent keeps as five std::vectors
(bots/bot-1/Agent.hpp:200-204,227,233-234,301-302) — push_back per tick, clear() on release — under the header's three rules
(a full buffer drops the tick; a restarted game starts a new list; the tick is appended).  Beside the lists it keeps an
image of the caller's device buffers as the kernel may leave them: what was never written holds the sentinel, what a later
list overwrote holds the later value.
Arithmetic: computeReturns() (:333-339) with torch CPU ops in the reference's order — the ATen arithmetic the reference
runs — and the same as uncontracted numpy f32, plus the two forms a compiler's fused multiply-add would give (emulated in
f64), which the committed seeds tell apart; train_log()'s four numbers (:342-350) as sequential f32."""
import numpy as np
import torch

ACTIONS, HIDDEN = 9, 160
MARKER = 0xFFFFFFFF
SENTINEL = 0x7FC0DEAD  # a quiet NaN nobody computes (tests/test_gpu_reward.py's pattern)
SENTINEL_U8 = 0xAD


def log32(x):
    """The f32 log of an f32, rounded once; log32(0) = -inf."""
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(x, dtype=np.float32).astype(np.float64)).astype(np.float32)


class RefRollout:
    def __init__(self, agents, T, list_cap, store_states=True, store_disc=True, store_imitate=True):
        self.agents, self.T, self.list_cap, self.store_states = agents, T, list_cap, store_states
        self.lists = [[] for _ in range(agents)]  # per agent: one dict per slot
        self.dropped = self.missing_states = 0
        s32 = lambda *shape: np.full((T, agents) + shape, SENTINEL, dtype=np.uint32)
        self.image = {"action": s32(), "probs": s32(ACTIONS), "value": s32(), "reward": s32()}
        if store_states:
            self.image.update(keys=s32(list_cap), vals=s32(list_cap), counts=s32(), pov=s32(HIDDEN))
        if store_disc:
            self.image["disc"] = s32()
        if store_imitate:
            self.image["imitate"] = np.full((T, agents), SENTINEL_U8, dtype=np.uint8)
        self.written = np.zeros((T, agents), dtype=bool)  # slots some tick was ever written to

    @staticmethod
    def _bits(x):
        x = np.ascontiguousarray(x)
        return x.view(np.uint32) if x.dtype.itemsize == 4 else x

    def record(self, tick, probs, value, action, reward, keys=None, vals=None, counts=None, pov=None, cap=0, disc=None, imitate=None,
               reset=None):
        """One tick of agents [0, len(value)).  reset: one flag per agent, or None."""
        im = self.image
        for a in range(len(value)):
            rows = self.lists[a]
            if len(rows) == self.T:  # ready: `if (is_training ...) return;`  Agent.hpp:219
                self.dropped += 1
                continue
            if reset is not None and reset[a]:  # a new Agent per game
                rows.clear()
            t = len(rows)
            row = dict(tick=tick, action=int(action[a]))
            if self.store_states:
                cnt = int(np.uint32(counts[a]))
                n = min(cnt, self.list_cap, cap)
                im["keys"][t, a, :n] = self._bits(keys[a, :n])
                im["vals"][t, a, :n] = self._bits(vals[a, :n])
                im["counts"][t, a] = cnt
                im["pov"][t, a] = self._bits(pov[a])
                if cnt > self.list_cap:
                    self.missing_states += 1
                row["count"] = cnt
            im["action"][t, a] = self._bits(np.asarray(action, dtype=np.int32)[a:a + 1])[0]
            im["probs"][t, a] = self._bits(np.asarray(probs[a], dtype=np.float32))
            im["value"][t, a] = self._bits(np.asarray(value, dtype=np.float32)[a:a + 1])[0]
            im["reward"][t, a] = self._bits(np.asarray(reward, dtype=np.float32)[a:a + 1])[0]
            if "disc" in im:
                im["disc"][t, a] = self._bits(np.asarray(disc, dtype=np.float32)[a:a + 1])[0]
            if "imitate" in im:
                im["imitate"][t, a] = imitate[a]
            self.written[t, a] = True
            rows.append(row)

    def fill(self):
        return np.array([len(r) for r in self.lists], dtype=np.int32)

    def ready(self):
        return self.fill() == self.T

    def release(self, mask=None):
        """clear(): the ready agents, or the agents a mask names (ready or not)."""
        for a, rows in enumerate(self.lists):
            if (mask[a] if mask is not None else len(rows) == self.T):
                rows.clear()

    def tick_of(self, a, t):
        return self.lists[a][t]["tick"]


# ---- computeReturns(), Agent.hpp:333-339 ------------------------------------------------------------------------------------
def returns_torch(rewards, gamma):
    """rewards [T] or [T][n] f32 -> returns of the same shape: torch CPU ops in the reference's order.  `gamma` is the
    reference's `float gamma`: (1 - gamma) is an f32 subtraction, a tensor times it is an f32 product."""
    g = np.float32(gamma)
    om = np.float32(1) - g
    r = torch.from_numpy(np.ascontiguousarray(rewards, dtype=np.float32))
    T = r.shape[0]
    out = [None] * T
    out[T - 1] = float(om) * r[T - 1]
    for i in range(T - 2, -1, -1):
        out[i] = float(g) * out[i + 1] + float(om) * r[i]
    return torch.stack(out).numpy()


def returns_numpy(rewards, gamma, fused=None):
    """The same in numpy f32, every product rounded before the add.  fused="carry": gamma * returns[i+1] kept exact inside
    the add, as fma(gamma, returns[i+1], (1-gamma)*r) gives it; fused="reward": fma(1-gamma, r, gamma*returns[i+1]).  The
    fused forms are emulated in f64 (a product of two f32 is exact there)."""
    g = np.float32(gamma)
    om = np.float32(1) - g
    r = np.ascontiguousarray(rewards, dtype=np.float32)
    T = r.shape[0]
    out = np.empty_like(r)
    with np.errstate(invalid="ignore", over="ignore"):
        out[T - 1] = om * r[T - 1]
        for i in range(T - 2, -1, -1):
            if fused == "carry":
                out[i] = (np.float64(g) * out[i + 1].astype(np.float64) + (om * r[i]).astype(np.float64)).astype(np.float32)
            elif fused == "reward":
                out[i] = ((g * out[i + 1]).astype(np.float64) + np.float64(om) * r[i].astype(np.float64)).astype(np.float32)
            else:
                out[i] = g * out[i + 1] + om * r[i]
    return out


def stats_ref(rewards, actions):
    """train_log()'s r_avg0, r_avg1, n_avg0, n_avg1 (Agent.hpp:342-350) per agent, [n][4]: sequential f32 sums over each
    half of the buffer; the reward sums are divided by T, the action-0 counts by T / 2."""
    r = np.ascontiguousarray(rewards, dtype=np.float32)
    T = r.shape[0]
    r = r.reshape(T, -1)
    act = np.asarray(actions).reshape(T, -1)
    s = np.zeros((2, r.shape[1]), dtype=np.float32)
    nothing = np.zeros((2, r.shape[1]), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(T):
            h = i // (T // 2)
            s[h] = s[h] + r[i]
            nothing[h] = nothing[h] + (act[i] == 0).astype(np.float32)
        return np.stack([s[0] / np.float32(T), s[1] / np.float32(T), nothing[0] / np.float32(T // 2), nothing[1] / np.float32(T // 2)], axis=1)


# ---- the GPU test's committed inputs ------------------------------------------------------------------------------------------
RETURNS_AGENTS = 130
RETURNS_T = (2, 4, 16, 1024)
RETURNS_GAMMAS = (0.99, 0.5)
RETURNS_SEED = 20260


def returns_case(T, agents=RETURNS_AGENTS, seed=RETURNS_SEED):
    """rewards = log D of a random D, values in (0, 1), actions in [0, 9) ([T][agents] each); agent 1 has one reward of -inf
    (D == 0) and agent 2 one value of 0, both at slot T // 2."""
    rng = np.random.default_rng(seed + T)
    disc = rng.uniform(1e-3, 1.0, size=(T, agents)).astype(np.float32)
    rewards = log32(disc)
    values = rng.uniform(1e-3, 1.0, size=(T, agents)).astype(np.float32)
    actions = rng.integers(0, ACTIONS, size=(T, agents)).astype(np.int32)
    rewards[T // 2, 1] = -np.inf
    values[T // 2, 2] = 0.0
    return rewards, values, actions
