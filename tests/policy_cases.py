"""Shared cases of the bot-network tests: parameter sets, observation makers, hand-built observation lists, the gate and
the reference trajectories.  Plain builders, no GPU: tests/test_policy_ref64.py (CPU) checks on every case that the f32
restatement stays within half of the gate around the f64 one, tests/test_gpu_policy_edges.py holds the HIP kernels to the
f64 one on the same cases.  A trajectory never depends on what a device computes (the action fed back is the f64
reference's own arg-max), so each is computed once per process and shared by every path that runs it."""
import functools
import os
import sys

import numpy as np
import torch

from strikeforce_amd import policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import policy_ref  # noqa: E402

# |hip - reference| <= ATOL + RTOL * |reference| on probabilities and value, 10 * ATOL + RTOL * |reference| on the
# recurrent state: the project's gate for the HIP path (tests/test_gpu_policy.py imports these)
RTOL, ATOL = 5e-5, 1e-6

HIDDEN, ACTIONS, CHANNELS, GRID = 160, 9, 32, 31
OBS_FLOATS = CHANNELS * GRID * GRID
POV_CELLS = ((14, 15), (15, 14), (15, 15), (15, 16), (16, 15))  # (row, column): Modules.hpp:114-121


def gate(ref, state=False):
    """The largest |device - ref| the project accepts, element by element."""
    return (10 * ATOL if state else ATOL) + RTOL * np.abs(np.asarray(ref, dtype=np.float64))


def gate_fraction(got, ref, state=False):
    """max |got - ref| / gate(ref): <= 1 passes the gate, <= 0.5 is the condition on the f32 reference."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref) / gate(ref, state)))


# torch's default initialisers (gain 1); every weight x3 (saturating gates, probabilities from 3e-7 to 0.98: what a
# trained checkpoint looks like; the largest gain at which the f32 restatement leaves half of the gate free); x0.3
PARAM_SETS = {"gain-1": dict(seed=41, gain=1.0), "gain-3": dict(seed=43, gain=3.0), "gain-0.3": dict(seed=47, gain=0.3)}


@functools.lru_cache(maxsize=None)
def parameters(name):
    return policy.init_parameters(**PARAM_SETS[name])


# ---- observation makers: (rng, B) -> [B, 32, 31, 31] f32 -------------------------------------------------------------
def obs_dense30(rng, B):
    """30 % non-zero, a fifth of them negative (tests/test_gpu_policy.py's `_obs`)."""
    x = rng.uniform(0.0, 2.0, size=(B, CHANNELS, GRID, GRID)).astype(np.float32)
    x *= rng.uniform(size=x.shape) < 0.3
    x *= np.where(rng.uniform(size=x.shape) < 0.2, -1.0, 1.0).astype(np.float32)
    return x


def obs_sparse1(rng, B):
    """1 % non-zero: what an observation of the simulator is."""
    x = rng.uniform(-2.0, 2.0, size=(B, CHANNELS, GRID, GRID)).astype(np.float32)
    x *= rng.uniform(size=x.shape) < 0.01
    return x


def obs_with_count(rng, n):
    """One image with exactly n non-zeros at random places."""
    x = np.zeros(OBS_FLOATS, dtype=np.float32)
    where = rng.choice(OBS_FLOATS, size=n, replace=False)
    x[where] = rng.uniform(0.25, 2.0, size=n) * rng.choice(np.array([-1.0, 1.0]), size=n)
    return x.reshape(CHANNELS, GRID, GRID)


EDGE_NAMES = ("all-zero", "one-corner", "centre-cells-only", "outside-the-centre-only", "one-channel-pair-full",
              "one-entry-per-channel", "one-entry-per-channel-pair", "magnitudes-2^-20..2^20-by-row")


@functools.lru_cache(maxsize=None)
def edge_images(seed=5):
    """[8, 32, 31, 31], in EDGE_NAMES' order: the all-zero image (feature row 0: the 1e-8 of the normalisation decides,
    pov is the action one-hot alone); one non-zero in a corner; non-zeros in the five centre cells only (all of them in
    pov); only outside them (pov = the one-hot alone); one pair of channels completely full (1 922 non-zeros, one
    partial sum); one entry in each of the 32 channels (a new pair at every second entry); one entry in every second
    channel (a new pair at every entry); 2 % non-zero with magnitudes from 2^-20 to 2^20 spread over the rows."""
    rng = np.random.default_rng(seed)
    x = np.zeros((len(EDGE_NAMES), CHANNELS, GRID, GRID), dtype=np.float32)
    x[1, 31, 30, 30] = -1.5
    for (r, c) in POV_CELLS:
        x[2, :, r, c] = rng.uniform(-2.0, 2.0, size=CHANNELS) * (rng.uniform(size=CHANNELS) < 0.5)
    x[2, 7, 15, 15] = 1.25  # (never empty)
    x[3] = obs_sparse1(rng, 1)[0]
    for (r, c) in POV_CELLS:
        x[3, :, r, c] = 0
    x[4, 12:14] = rng.uniform(0.5, 2.0, size=(2, GRID, GRID)) * rng.choice(np.array([-1.0, 1.0]), size=(2, GRID, GRID))
    for ch in range(CHANNELS):
        x[5, ch, rng.integers(0, GRID), rng.integers(0, GRID)] = rng.uniform(0.5, 2.0)
    for ch in range(0, CHANNELS, 2):
        x[6, ch, rng.integers(0, GRID), rng.integers(0, GRID)] = -rng.uniform(0.5, 2.0)
    m = rng.uniform(-2.0, 2.0, size=(CHANNELS, GRID, GRID)) * (rng.uniform(size=(CHANNELS, GRID, GRID)) < 0.02)
    x[7] = m * np.exp2(np.round(np.linspace(-20, 20, GRID)))[None, :, None]
    assert np.count_nonzero(x[4]) == 2 * GRID * GRID and np.count_nonzero(x[5]) == CHANNELS
    return x


# ---- the observation as lists ------------------------------------------------------------------------------------------
def lists_from_dense(obs, cap):
    """The lists sf_observe_sparse_device writes for these dense observations (include/strikeforce.h): per agent the
    non-zero floats in the dense buffer's own order (channel, then row, then column), key = channel * 9 | row << 9 |
    column << 14, count = the true number of non-zeros (above `cap`: the list was cut, only the first cap entries are
    there), pov = the 5 x 32 floats around the centre, channel fastest.  (The 0xffffffff marker of a crowded window is
    the simulator's own decision; a test that wants it overwrites the count.)
    -> keys uint32 [B, cap], vals float32 [B, cap], counts uint32 [B], pov float32 [B, 160]"""
    obs = np.ascontiguousarray(obs, dtype=np.float32).reshape(-1, CHANNELS, GRID, GRID)
    B = obs.shape[0]
    keys = np.zeros((B, cap), dtype=np.uint32)
    vals = np.zeros((B, cap), dtype=np.float32)
    counts = np.zeros(B, dtype=np.uint32)
    flat = obs.reshape(B, -1)
    for b in range(B):
        nz = np.flatnonzero(flat[b])
        counts[b] = len(nz)
        nz = nz[:cap]
        ch, r = np.divmod(nz, GRID * GRID)
        y, x = np.divmod(r, GRID)
        keys[b, :len(nz)] = (ch * 9) | (y << 9) | (x << 14)
        vals[b, :len(nz)] = flat[b][nz]
    pov = np.stack([obs[:, :, r, c] for r, c in POV_CELLS], axis=1).reshape(B, 5 * CHANNELS)
    return keys, vals, counts, np.ascontiguousarray(pov)


def dense_from_lists(keys, vals, counts):
    """The inverse, for lists that fit: the dense observations [B, 32, 31, 31]."""
    B = len(counts)
    obs = np.zeros((B, CHANNELS, GRID, GRID), dtype=np.float32)
    for b in range(B):
        k = keys[b, :counts[b]].astype(np.int64)
        obs[b, (k & 511) // 9, (k >> 9) & 31, (k >> 14) & 31] = vals[b, :counts[b]]
    return obs


def features64(params, obs):
    """GameCNN::forward in float64 and the same chain on |x| with |W| (what an f32 evaluation's roundings are
    proportional to): [B, 160] each."""
    import torch.nn.functional as F
    want = torch.from_numpy(np.ascontiguousarray(obs)).double()
    mag = want.abs()
    for i in range(4):
        w = torch.from_numpy(params["backbone.cnn.conv%d.weight" % i]).double()
        want, mag = F.conv2d(want, w, stride=2), F.conv2d(mag, w.abs(), stride=2)
    return want.reshape(-1, HIDDEN).numpy(), mag.reshape(-1, HIDDEN).numpy()


# ---- trajectories ------------------------------------------------------------------------------------------------------
def random_memory(rng, B):
    """A state as a running agent has it: h in (-1, 1), any of the nine actions as the last one."""
    h = rng.uniform(-1.0, 1.0, size=(2, B, HIDDEN)).astype(np.float32)
    a = np.eye(ACTIONS, dtype=np.float32)[rng.integers(0, ACTIONS, size=B)]
    return h, a


def fresh_memory(B):
    return np.zeros((2, B, HIDDEN), dtype=np.float32), np.eye(ACTIONS, dtype=np.float32)[[0] * B]


@functools.lru_cache(maxsize=None)
def _made(maker, B, steps, seed):
    rng = np.random.default_rng(seed)
    make = {"dense30": obs_dense30, "sparse1": obs_sparse1}[maker]
    return [make(rng, B) for _ in range(steps)]


class Case:
    """A recurrent run: the observations, the memory it starts from, and resets {step: agents} applied in front of that
    step's forward (Backbone::reset_memory, Modules.hpp:95-100)."""

    def __init__(self, params, B, steps, maker, seed, start="fresh", resets=None):
        self.params, self.B, self.steps, self.maker, self.seed = params, B, steps, maker, seed
        self.start, self.resets = start, resets or {}

    def observations(self):
        """steps x [B, 32, 31, 31] (the same arrays on every call)"""
        if self.maker == "edges":  # every image twice: from a new agent's memory, then from another image's state
            e = edge_images()
            return [e, np.ascontiguousarray(e[::-1])][:self.steps]
        if self.steps * self.B > 2000:  # (a long run: 16 MB a step, made again where it is needed)
            return _made.__wrapped__(self.maker, self.B, self.steps, self.seed)
        return _made(self.maker, self.B, self.steps, self.seed)

    def memory(self):
        if self.start == "fresh":
            return fresh_memory(self.B)
        return random_memory(np.random.default_rng(self.seed + 1000), self.B)


class Run:
    """What a reference computed: per step probs [B, 9], value [B], the state behind it [2, B, 160], and the action whose
    one-hot went into the next step."""

    def __init__(self):
        self.probs, self.value, self.h, self.action = [], [], [], []


def run_reference(case, dtype, actions=None):
    """The restatement over `case`.  actions: per step the action to feed back (the f32 run is given the f64 run's, so
    that the two stay one trajectory); None: the arg-max of this run's own probabilities."""
    params = parameters(case.params)
    h, a = case.memory()
    out = Run()
    for t, obs in enumerate(case.observations()):
        if t in case.resets:
            h = np.array(h)
            for b in case.resets[t]:
                h[:, b] = 0
                a[b] = np.eye(ACTIONS, dtype=np.float32)[0]
        probs, value, h = policy_ref.forward_batched(params, obs, h, a, dtype=dtype)
        act = probs.argmax(axis=1) if actions is None else actions[t]
        a = np.eye(ACTIONS, dtype=np.float32)[act]
        out.probs.append(probs), out.value.append(value), out.h.append(h), out.action.append(np.asarray(act))
    return out


@functools.lru_cache(maxsize=None)
def reference64(key):
    """The f64 trajectory of CASES[key], computed once per process."""
    return run_reference(CASES[key], torch.float64)


PATH_BATCHES = (1, 17, 100, 300)  # one-, two- and four-wave GEMM blocks, ragged tiles, B % 16 != 0
LONG_STEPS, LONG_B, LONG_RESET_AT, LONG_RESET = 120, 33, 60, (0, 16, 32)
PARTIAL_MAX, PARTIAL_AGENTS = 64, (1, 15, 16, 17, 33, 63)
# the restart flags of the partial-batch test's predict call: agents [0, 64), three in ten set
PARTIAL_RESET = tuple(int(b) for b in np.flatnonzero(np.random.default_rng(99).uniform(size=PARTIAL_MAX) < 0.3))

CASES = {}
for _p in PARAM_SETS:
    for _B in PATH_BATCHES:  # test_every_path
        CASES["paths/%s/B%d" % (_p, _B)] = Case(_p, _B, 4, "dense30", seed=100 + _B)
for _p in ("gain-1", "gain-3"):
    CASES["long/%s" % _p] = Case(_p, LONG_B, LONG_STEPS, "sparse1", seed=7, resets={LONG_RESET_AT: LONG_RESET})
    CASES["edges/%s" % _p] = Case(_p, len(EDGE_NAMES), 2, "edges", seed=0)
# one step of 64 agents out of a running agent's memory (the partial-batch test evaluates the first `agents` of them),
# and the same with some of them restarted first
CASES["partial/gain-1"] = Case("gain-1", PARTIAL_MAX, 1, "sparse1", seed=21, start="random")
CASES["partial-restarted/gain-1"] = Case("gain-1", PARTIAL_MAX, 1, "sparse1", seed=21, start="random", resets={0: PARTIAL_RESET})
