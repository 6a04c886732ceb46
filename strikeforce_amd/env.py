"""Host-side mirror of the reference's environment surface over the C-ABI (include/strikeforce.h).

``ArenaBatch`` is plumbing only: it loads libstrikeforce_amd.so (hand-written gfx950 kernels) and moves
pointers.  There is no CPU path — if the library is missing or no MI355X is visible it raises.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# SF_LIBRARY_PATH: load another build of the same library (A/B timing of two builds inside one gpurun call)
LIB_PATH = os.environ.get("SF_LIBRARY_PATH") or os.path.join(_HERE, "libstrikeforce_amd.so")
_LIB = None


class StrikeForceError(RuntimeError):
    pass


def load_library():
    """Load the HIP library and declare its signatures.  Raises if it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise StrikeForceError(
                "libstrikeforce_amd.so is missing: run `python -m strikeforce_amd.build` (hipcc, gfx950). "
                "strikeforce_amd has no CPU path.")
        # PyTorch wheels bundle their own libamdhip64 / libhsa-runtime64.  If this library's copies (from /opt/rocm)
        # were mapped first, a later `import torch` would bring a second HSA runtime into the process and
        # torch.cuda would find no GPU.  Importing torch first makes the loader resolve our DT_NEEDED entries to
        # the runtime that is already mapped (same sonames), so there is exactly one runtime either way.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        L.sf_create.argtypes = [C.POINTER(abi.Config), C.POINTER(vp)]
        L.sf_create.restype = C.c_int
        abi.bind(L, "sf_")
        L.sf_destroy.restype = C.c_int
        L.sf_step_device.argtypes = [vp, vp, C.c_int32]
        L.sf_observe_device.argtypes = [vp, vp]
        L.sf_observe_device_delta.argtypes = [vp, vp]
        L.sf_observe_sparse_device.argtypes = [vp, vp, vp, vp, vp, C.c_int32]
        L.sf_observe_overflow_device.argtypes = [vp, vp, C.c_int32, vp, vp]
        L.sf_observe_overflow_device.restype = C.c_int
        L.sf_results_device.argtypes = [vp, vp]
        L.sf_done_device.argtypes = [vp, vp]
        if hasattr(L, "sf_done_view_device"):  # (A/B runs against older builds of the library, tools/ab.sh)
            L.sf_done_view_device.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
            L.sf_done_view_device.restype = C.c_int
        if hasattr(L, "sf_episode_log"):  # (the episode log; an older build loaded through SF_LIBRARY_PATH lacks it)
            L.sf_episode_log.argtypes = [vp, C.c_int32]
            L.sf_episodes.argtypes = [vp, vp, C.c_int32, vp]
            L.sf_episodes_device.argtypes = [vp, vp, C.c_int32, vp]
            L.sf_episode_ring.argtypes = [vp, vp]
            L.sf_episodes_allgather.argtypes = [vp, vp]
            for n in ("sf_episode_log", "sf_episodes", "sf_episodes_device", "sf_episode_ring", "sf_episodes_allgather"):
                getattr(L, n).restype = C.c_int
        if hasattr(L, "sf_replay_load"):  # (replay of logged games; an older build loaded through SF_LIBRARY_PATH lacks it)
            L.sf_replay_load.argtypes = [vp, vp, vp]
            L.sf_replay_step.argtypes = [vp]
            L.sf_replay_status.argtypes = [vp, vp]
            L.sf_replay_status_device.argtypes = [vp, vp]
            L.sf_replay_commands_device.argtypes = [vp, vp]
            for n in REPLAY_EXPORTS:
                getattr(L, n).restype = C.c_int
        if hasattr(L, "sf_reset_arenas"):  # (restart of chosen arenas; an older build loaded through SF_LIBRARY_PATH lacks it)
            L.sf_reset_arenas.argtypes = [vp, C.POINTER(abi.ResetSel)]
            L.sf_reset_arenas.restype = C.c_int
        if hasattr(L, "sf_snapshot_create"):  # (arena snapshots; an older build loaded through SF_LIBRARY_PATH lacks them)
            abi.bind_snapshot(L, "sf_")
        if hasattr(L, "sf_signals_create"):  # (per-step signals; an older build loaded through SF_LIBRARY_PATH lacks them)
            abi.bind_signals(L, "sf_")
        if hasattr(L, "sf_state_device"):  # (state records on the device; an older build loaded through SF_LIBRARY_PATH lacks them)
            abi.bind_state(L, "sf_")
        if hasattr(L, "sf_state_put_device"):  # (arenas written from records; an older build loaded through SF_LIBRARY_PATH lacks it)
            abi.bind_state_put(L, "sf_")
        if hasattr(L, "sf_record_create"):  # (recording of games; an older build loaded through SF_LIBRARY_PATH lacks it)
            abi.bind_record(L, "sf_")
        if hasattr(L, "sf_action_mask_device"):  # (action masks; an older build loaded through SF_LIBRARY_PATH lacks them)
            abi.bind_action_mask(L, "sf_")
        L.sf_set_stream.argtypes = [vp, vp]
        L.sf_synchronize.argtypes = [vp]
        L.sf_kernel_time.argtypes = [vp, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
        if hasattr(L, "sf_step_kernel"):  # (an older build loaded through SF_LIBRARY_PATH lacks it)
            L.sf_step_kernel.argtypes = [vp, C.POINTER(C.c_int32)]
            L.sf_step_kernel.restype = C.c_int
        L.sf_comm_unique_id.argtypes = [C.c_char_p]
        L.sf_comm_init.argtypes = [vp, C.c_char_p, C.c_int32, C.c_int32]
        L.sf_results_allgather.argtypes = [vp, vp]
        L.sf_comm_wait.argtypes = [vp, C.c_int32]
        L.sf_comm_ranks.argtypes = [vp, C.POINTER(C.c_int32)]
        L.sf_step_end_device.argtypes = [vp, vp]
        L.sf_agent_alive_device.argtypes = [vp, vp]
        for n in ("sf_comm_unique_id", "sf_comm_init", "sf_results_allgather", "sf_comm_wait", "sf_comm_ranks",
                  "sf_step_end_device", "sf_agent_alive_device"):
            getattr(L, n).restype = C.c_int
        L.sf_config_defaults.argtypes = [C.POINTER(abi.Config)]
        L.sf_config_defaults.restype = None
        for n in ("sf_step_device", "sf_observe_device", "sf_observe_device_delta", "sf_observe_sparse_device", "sf_results_device", "sf_done_device", "sf_set_stream", "sf_synchronize",
                  "sf_kernel_time", "sf_abi_version"):
            getattr(L, n).restype = C.c_int
        L.sf_last_error.restype = C.c_char_p
        _LIB = L
    return _LIB


REPLAY_EXPORTS = ("sf_replay_load", "sf_replay_step", "sf_replay_status", "sf_replay_status_device",
                  "sf_replay_commands_device")

# every symbol include/strikeforce.h declares
EXPORTS = ["sf_create", "sf_destroy", "sf_config_defaults", "sf_reset", "sf_step", "sf_step_device", "sf_observe",
           "sf_observe_device", "sf_observe_device_delta", "sf_observe_sparse_device", "sf_observe_overflow_device", "sf_results", "sf_results_device", "sf_done", "sf_done_device", "sf_done_view_device", "sf_state_digest", "sf_dump_arena",
           "sf_set_stream", "sf_synchronize", "sf_kernel_time", "sf_step_kernel", "sf_last_error", "sf_abi_version",
           "sf_comm_unique_id", "sf_comm_init", "sf_results_allgather", "sf_comm_wait", "sf_comm_ranks",
           "sf_step_begin", "sf_step_end", "sf_step_end_device", "sf_agent_alive", "sf_agent_alive_device", "sf_phase_draws",
           "sf_episode_log", "sf_episodes", "sf_episodes_device", "sf_episode_ring", "sf_episodes_allgather",
           "sf_replay_load", "sf_replay_step", "sf_replay_status", "sf_replay_status_device", "sf_replay_commands_device",
           "sf_reset_arenas"] + ["sf_" + n for n in abi.SNAPSHOT_EXPORTS + abi.SIGNALS_EXPORTS + abi.STATE_EXPORTS +
                                     abi.RECORD_EXPORTS + abi.ACTION_MASK_EXPORTS + abi.STATE_PUT_EXPORTS]

EPISODE_HDR_WORDS = 8  # SF_EPISODE_HDR_WORDS


def episode_record_words(n_agents):
    """int32 words of one episode-log record: the header, then eight result words per agent."""
    return EPISODE_HDR_WORDS + 8 * n_agents


def decode_episodes(records, n_agents):
    """Named arrays of episode-log records (sf_episodes / sf_episode_ring / sf_episodes_allgather output, any leading
    shape, flattened to n records): arena, episode, tb (uint64), serial (uint64), steps, outcome (int32 [n]) and
    results (int32 [n][n_agents][8], the words sf_results holds).  Empty ring slots come out with episode == -1."""
    r = np.ascontiguousarray(records, dtype=np.int32).reshape(-1, episode_record_words(n_agents))
    u = r.view(np.uint32).astype(np.uint64)
    return {
        "arena": r[:, 0].copy(), "episode": r[:, 1].copy(),
        "tb": u[:, 2] | (u[:, 3] << np.uint64(32)), "serial": u[:, 4] | (u[:, 5] << np.uint64(32)),
        "steps": r[:, 6].copy(), "outcome": r[:, 7].copy(),
        "results": r[:, EPISODE_HDR_WORDS:].reshape(-1, n_agents, 8).copy(),
    }


class Snapshot:
    """`slots` saved arena states in device memory (strikeforce.h sf_snapshot_*): save(slot_of_arena) copies arena a into
    slot slot_of_arena[a], load(slot_of_arena) copies slot slot_of_arena[a] into arena a; -1 leaves the arena out, and many
    arenas may load one slot — the fork.  Both are one stream-ordered launch.  slot_of_arena: a device address (int) of
    int32 [arenas], a torch int32 tensor on the environment's device, or a host array, which is uploaded first (and, for
    save, refused if two arenas name one slot).  A load keeps the destination's episode count, result latch and episode
    log; what else it carries and leaves is in the header.  export / import_ move one slot through a host blob that only
    an environment of the same configuration (any arena count) accepts.  close() before the environment's."""

    def __init__(self, batch, slots):
        if not hasattr(batch.L, "sf_snapshot_create"):
            raise StrikeForceError("this build of libstrikeforce_amd.so has no sf_snapshot_* entry points")
        self.batch, self.L, self.slots = batch, batch.L, int(slots)
        self.h = C.c_void_p()
        self._held = None  # the uploaded index array of the last call: alive until the next one replaces it
        rc = self.L.sf_snapshot_create(batch.h, self.slots, C.byref(self.h))
        if rc != 0:
            self.h = None
            raise StrikeForceError("sf_snapshot_create failed (%d): %s" % (rc, self.L.sf_last_error().decode()))
        self.blob_bytes = batch.snapshot_slot_bytes()[1]

    def close(self):
        if getattr(self, "h", None):
            self.L.sf_snapshot_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _index(self, slot_of_arena, saving):
        if isinstance(slot_of_arena, int):
            return slot_of_arena
        if hasattr(slot_of_arena, "data_ptr"):  # a torch tensor
            t = slot_of_arena
            if str(t.dtype) != "torch.int32" or not t.is_cuda or not t.is_contiguous() or t.numel() != self.batch.cfg.arenas:
                raise ValueError("slot_of_arena must be a contiguous int32 tensor of `arenas` entries on the device")
            return t.data_ptr()
        host = np.ascontiguousarray(slot_of_arena, dtype=np.int32).reshape(-1)
        if host.size != self.batch.cfg.arenas:
            raise ValueError("slot_of_arena must hold one entry per arena")
        named = host[(host >= 0) & (host < self.slots)]  # (anything else is skipped by the kernel)
        if saving and len(np.unique(named)) != len(named):
            raise ValueError("two arenas save into one slot")
        import torch
        # (a copy from pageable host memory has arrived when .to() returns, whatever stream the environment runs on)
        self._held = torch.from_numpy(host).to("cuda:%d" % self.batch.cfg.device)
        return self._held.data_ptr()

    def save(self, slot_of_arena):
        rc = self.L.sf_snapshot_save(self.batch.h, self.h, C.c_void_p(self._index(slot_of_arena, True)))
        self.batch._ck(rc, "sf_snapshot_save")

    def load(self, slot_of_arena):
        rc = self.L.sf_snapshot_load(self.batch.h, self.h, C.c_void_p(self._index(slot_of_arena, False)))
        self.batch._ck(rc, "sf_snapshot_load")

    def status(self):
        """(arenas skipped for an empty slot, arenas skipped for an index out of range) since the last call; synchronises."""
        out = (C.c_int32 * abi.SNAPSHOT_STATUS_WORDS)()
        self.batch._ck(self.L.sf_snapshot_status(self.h, C.byref(out)), "sf_snapshot_status")
        return int(out[0]), int(out[1])

    def export(self, slot):
        buf = C.create_string_buffer(self.blob_bytes)
        self.batch._ck(self.L.sf_snapshot_export(self.h, int(slot), C.cast(buf, C.c_void_p), self.blob_bytes), "sf_snapshot_export")
        return buf.raw

    def import_(self, slot, blob):
        blob = bytes(blob)
        self.batch._ck(self.L.sf_snapshot_import(self.h, int(slot), C.cast(C.c_char_p(blob), C.c_void_p), len(blob)), "sf_snapshot_import")


SIG_PRESENT, SIG_DIED, SIG_ENDED = abi.SIG_PRESENT, abi.SIG_DIED, abi.SIG_ENDED
SIG_REBASED, SIG_UNRESOLVED, SIG_IDLE = abi.SIG_REBASED, abi.SIG_UNRESOLVED, abi.SIG_IDLE


def reward_weights(per_step=0.0, kills=0.0, teams_kills=0.0, loot=0.0, damage=0.0, effect=0.0, hp=0.0, died=0.0, outcome=None):
    """An abi.RewardWeights; outcome: {SF_* outcome code: weight} or a sequence of up to eight weights by code."""
    w = abi.RewardWeights()
    w.per_step, w.died = per_step, died
    for j, x in enumerate((kills, teams_kills, loot, damage, effect, hp)):
        w.w[j] = x
    for code, x in (outcome.items() if isinstance(outcome, dict) else enumerate(outcome or ())):
        w.outcome[code] = x
    return w


def decode_signals(vitals=None, delta=None):
    """Host copies of sf_signals_step's outputs by field name: vitals int32 [..., 16] and / or delta int32 [..., 8] ->
    {name: int32 [...]} (abi.VITALS_FIELDS, abi.DELTA_FIELDS; the delta's flag word under "flags" where only a delta is
    given, else the vitals' — they are the same word), plus one bool array per flag bit: present, died, ended, rebased,
    unresolved, idle."""
    out = {}
    if delta is not None:
        d = np.asarray(delta, dtype=np.int32)
        assert d.shape[-1] == abi.DELTA_WORDS
        out.update({n: d[..., j] for j, n in enumerate(abi.DELTA_FIELDS)})
    if vitals is not None:
        v = np.asarray(vitals, dtype=np.int32)
        assert v.shape[-1] == abi.VITALS_WORDS
        out.update({n: v[..., j] for j, n in enumerate(abi.VITALS_FIELDS)})
    if "flags" in out:
        for bit, n in ((SIG_PRESENT, "present"), (SIG_DIED, "died"), (SIG_ENDED, "ended"), (SIG_REBASED, "rebased"),
                       (SIG_UNRESOLVED, "unresolved"), (SIG_IDLE, "idle")):
            out[n] = (out["flags"] & bit) != 0
    return out


COMMANDS = abi.ALL_COMMANDS  # SF_COMMANDS: bit k of an action-mask word stands for COMMANDS[k]


def decode_action_mask(words):
    """Action-mask command words (host copies, uint32 [...]) as a bool array [..., 30]: [..., k] = COMMANDS[k] would do
    something."""
    w = np.asarray(words).astype(np.uint32)
    return ((w[..., None] >> np.arange(abi.N_COMMANDS, dtype=np.uint32)) & np.uint32(1)).astype(bool)


def decode_state(hdr=None, humans=None, zombies=None, bullets=None, portals=None, counts=None):
    """Named views of sf_state_device's record outputs, torch tensors or numpy arrays alike, nothing copied: each table
    int32 [..., words of its record] -> {field: int32 [...]} (cons / throw_cnt keep a last axis of 4) under "humans",
    "zombies", "bullets", "portals"; hdr int32 [rows][40] -> "hdr": the ten 64-bit fields as int64 [rows], rng int32
    [rows][18], done, outcome; counts int32 [rows][8] -> "counts": abi.STATE_COUNT_FIELDS.  -> {table: {field: view}}"""
    out = {}
    for name, t, struct in (("humans", humans, abi.HumanRec), ("zombies", zombies, abi.ZombieRec),
                            ("bullets", bullets, abi.BulletRec), ("portals", portals, abi.PortalRec)):
        if t is not None:
            assert t.shape[-1] == C.sizeof(struct) // 4
            out[name] = {n: (t[..., w] if k == 1 else t[..., w:w + k]) for n, w, k in abi.record_fields(struct)}
    if hdr is not None:
        assert hdr.shape[-1] == C.sizeof(abi.ArenaHdr) // 4
        i64 = hdr[..., :20].view(np.int64 if isinstance(hdr, np.ndarray) else __import__("torch").int64)
        h = {n: i64[..., j] for j, (n, _) in enumerate(abi.ArenaHdr._fields_[:10])}
        h.update(rng=hdr[..., 20:38], done=hdr[..., 38], outcome=hdr[..., 39])
        out["hdr"] = h
    if counts is not None:
        assert counts.shape[-1] == abi.STATE_COUNT_WORDS
        out["counts"] = {n: counts[..., j] for j, n in enumerate(abi.STATE_COUNT_FIELDS)}
    return out


def encode_state(hdr=None, humans=None, zombies=None, bullets=None, portals=None):
    """The inverse of decode_state(): field dictionaries -> record arrays.  Each table {field: [...]} (cons / throw_cnt with a
    last axis of 4) -> int32 [..., words of its record]; hdr {the ten 64-bit fields, rng [rows][18], done, outcome} -> int32
    [rows][40].  Numpy arrays give numpy arrays, torch tensors give torch tensors on the fields' device.  -> {name: array}
    for the parts given, what ArenaBatch.put_state takes as its raw records."""
    out = {}

    def new(shape, proto):
        if isinstance(proto, np.ndarray) or not hasattr(proto, "device"):
            return np.zeros(shape, dtype=np.int32)
        import torch
        return torch.zeros(shape, dtype=torch.int32, device=proto.device)

    for name, d, struct in (("humans", humans, abi.HumanRec), ("zombies", zombies, abi.ZombieRec),
                            ("bullets", bullets, abi.BulletRec), ("portals", portals, abi.PortalRec)):
        if d is None:
            continue
        fields = abi.record_fields(struct)
        first = d[fields[0][0]]
        first = first if hasattr(first, "shape") else np.asarray(first)
        t = new(tuple(first.shape) + (C.sizeof(struct) // 4,), first)
        for n, w, k in fields:
            v = d[n] if hasattr(d[n], "shape") else np.asarray(d[n])
            if k == 1:
                t[..., w] = v
            else:
                t[..., w:w + k] = v
        out[name] = t
    if hdr is not None:
        names = [n for n, _ in abi.ArenaHdr._fields_[:10]]
        first = hdr[names[0]] if hasattr(hdr[names[0]], "shape") else np.asarray(hdr[names[0]])
        t = new(tuple(first.shape) + (C.sizeof(abi.ArenaHdr) // 4,), first)
        i64 = t[..., :20].view(np.int64 if isinstance(t, np.ndarray) else __import__("torch").int64)
        for j, n in enumerate(names):
            i64[..., j] = hdr[n] if hasattr(hdr[n], "shape") else np.asarray(hdr[n])
        t[..., 20:38] = hdr["rng"] if hasattr(hdr["rng"], "shape") else np.asarray(hdr["rng"])
        t[..., 38], t[..., 39] = hdr["done"], hdr["outcome"]
        out["hdr"] = t
    return out


class Signals:
    """Per-step game signals of every (arena, agent) on the device (strikeforce.h sf_signals_*): step() is one
    stream-ordered launch behind any step that writes, wherever a device address is given, the vitals (int32 [arenas]
    [n_agents][16]), the delta since this object's previous step() (int32 [arenas][n_agents][8]) and the shaped reward
    (float32 [arenas * n_agents], what the rollout buffer's d_reward takes; weights: an abi.RewardWeights, see
    reward_weights()).  rebase_ptr: device uint8 [arenas][n_agents], non-zero where the caller restarted or loaded the
    arena since the previous step() — reset_arenas(selected_ptr=)'s output as it is.  Pointers are device addresses (int)
    or torch tensors.  close() before the environment's."""

    def __init__(self, batch):
        if not hasattr(batch.L, "sf_signals_create"):
            raise StrikeForceError("this build of libstrikeforce_amd.so has no sf_signals_* entry points")
        self.batch, self.L = batch, batch.L
        self.h = C.c_void_p()
        rc = self.L.sf_signals_create(batch.h, C.byref(self.h))
        if rc != 0:
            self.h = None
            raise StrikeForceError("sf_signals_create failed (%d): %s" % (rc, self.L.sf_last_error().decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.sf_signals_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _ptr(x):
        return x.data_ptr() if hasattr(x, "data_ptr") else x

    def step(self, vitals_ptr=None, delta_ptr=None, reward_ptr=None, rebase_ptr=None, weights=None):
        io = abi.SignalsIO(self._ptr(vitals_ptr), self._ptr(delta_ptr), self._ptr(reward_ptr), self._ptr(rebase_ptr),
                           weights if weights is not None else abi.RewardWeights())
        self.batch._ck(self.L.sf_signals_step(self.batch.h, self.h, C.byref(io)), "sf_signals_step")

    def status(self):
        """(delta records that carried UNRESOLVED, records rebased by the detection alone) since the last call;
        synchronises and clears."""
        out = (C.c_int64 * abi.SIGNALS_STATUS_WORDS)()
        self.batch._ck(self.L.sf_signals_status(self.h, C.byref(out)), "sf_signals_status")
        return int(out[0]), int(out[1])


def decode_games(games):
    """Named arrays of the game records sf_record_collect* delivers (int32 [n][12]): arena, episode, tb (uint64), serial
    (uint64), lines, iterations, end (abi.RECORD_*), outcome (int32 [n]) and offset (int64 [n], the stream's first byte in
    the collected bytes)."""
    r = np.ascontiguousarray(games, dtype=np.int32).reshape(-1, abi.RECORD_GAME_WORDS)
    u = r.view(np.uint32).astype(np.uint64)
    return {
        "arena": r[:, 0].copy(), "episode": r[:, 1].copy(),
        "tb": u[:, 2] | (u[:, 3] << np.uint64(32)), "serial": u[:, 4] | (u[:, 5] << np.uint64(32)),
        "lines": r[:, 6].copy(), "iterations": r[:, 7].copy(), "end": r[:, 8].copy(), "outcome": r[:, 9].copy(),
        "offset": (u[:, 10] | (u[:, 11] << np.uint64(32))).astype(np.int64),
    }


class Recorder:
    """Games written out on the device as the command streams of `.sf_sample` files (strikeforce.h sf_record_*): step(d_cmd)
    plays one iteration of every arena exactly as step_device(d_cmd, 1) does and appends the lines the reference's logger
    would write; flush() closes every open game as cut; collect() hands out the closed games (int32 [n][12], see
    decode_games) and their streams back to back (uint8), with the six counts by name; collect_device() does the same into
    device buffers without a host synchronisation.  replay.samples_from_recording turns a collection into Samples.
    Pointers are device addresses (int) or torch tensors.  close() before the environment's."""

    def __init__(self, batch, bytes_per_arena, games_per_arena):
        if not hasattr(batch.L, "sf_record_create"):
            raise StrikeForceError("this build of libstrikeforce_amd.so has no sf_record_* entry points")
        self.batch, self.L = batch, batch.L
        self.bytes_per_arena, self.games_per_arena = int(bytes_per_arena), int(games_per_arena)
        self.h = C.c_void_p()
        rc = self.L.sf_record_create(batch.h, self.bytes_per_arena, self.games_per_arena, C.byref(self.h))
        if rc != 0:
            self.h = None
            raise StrikeForceError("sf_record_create failed (%d): %s" % (rc, self.L.sf_last_error().decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.sf_record_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _ptr(x):
        return x.data_ptr() if hasattr(x, "data_ptr") else x

    def step(self, d_cmd_ptr):
        self.batch._ck(self.L.sf_record_step(self.batch.h, self.h, self._ptr(d_cmd_ptr)), "sf_record_step")

    def flush(self):
        self.batch._ck(self.L.sf_record_flush(self.batch.h, self.h), "sf_record_flush")

    def collect_device(self, d_bytes_ptr, max_bytes, d_games_ptr, max_games, d_counts_ptr):
        self.batch._ck(self.L.sf_record_collect_device(self.h, self._ptr(d_bytes_ptr), int(max_bytes), self._ptr(d_games_ptr),
                                                       int(max_games), self._ptr(d_counts_ptr)), "sf_record_collect_device")

    def collect(self, max_bytes=None, max_games=None):
        """(games int32 [n][12], bytes uint8 [m], counts dict) of the closed games that fit; synchronises.  The defaults
        hold everything a recorder can hold."""
        A = self.batch.cfg.arenas
        max_bytes = int(max_bytes) if max_bytes is not None else A * self.bytes_per_arena
        max_games = int(max_games) if max_games is not None else A * self.games_per_arena
        data = np.zeros(max(max_bytes, 1), dtype=np.uint8)
        games = np.zeros((max(max_games, 1), abi.RECORD_GAME_WORDS), dtype=np.int32)
        counts = np.zeros(abi.RECORD_COUNT_WORDS, dtype=np.int64)
        self.batch._ck(self.L.sf_record_collect(self.h, data.ctypes.data, max_bytes, games.ctypes.data, max_games,
                                                counts.ctypes.data), "sf_record_collect")
        named = dict(zip(abi.RECORD_COUNT_FIELDS, (int(x) for x in counts)))
        return games[:named["games"]].copy(), data[:named["bytes"]].copy(), named


class ArenaBatch:
    """A batch of independent arenas on one GPU.

    Mirrors the reference loop (gameplay.hpp:1428-1505): ``reset`` = setup()+load_data() and the first
    loop top; ``step`` = one iteration of play()'s while(true) for every arena, commands are the
    reference's command chars; ``observe`` = gameplay::bot()'s 32x31x31 encoding
    (bots/bot-0.5/Custom.hpp:137-159); ``done`` = check_end().
    """

    def __init__(self, workload):
        self.w = workload
        self.cfg = workload.cfg
        self.L = load_library()
        self.h = C.c_void_p()
        rc = self.L.sf_create(C.byref(self.cfg), C.byref(self.h))
        if rc != 0:
            self.h = None
            raise StrikeForceError("sf_create failed (%d): %s" % (rc, self.L.sf_last_error().decode()))

    def _ck(self, rc, what):
        if rc != 0:
            raise StrikeForceError("%s failed (%d): %s" % (what, rc, self.L.sf_last_error().decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.sf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream):
        self._ck(self.L.sf_set_stream(self.h, C.c_void_p(hip_stream)), "sf_set_stream")

    def synchronize(self):
        self._ck(self.L.sf_synchronize(self.h), "sf_synchronize")

    def reset(self, tb, serial):
        self._ck(self.L.sf_reset(self.h, tb, serial), "sf_reset")

    def reset_arenas(self, mask_ptr=None, mask_stride=1, done=False, max_steps=0, tb_ptr=None, serial_ptr=None,
                     selected_ptr=None):
        """Restart the chosen arenas on the device, in stream order, every other arena untouched (sf_reset_arenas): those
        whose byte at mask_ptr[a * mask_stride] is set, with done=True those whose game has ended, with max_steps > 0
        those whose running game has played that many steps.  tb_ptr / serial_ptr: device uint64 [arenas], read for the
        chosen arenas only; both None: tb + reseed_stride, the serial kept.  selected_ptr: device uint8
        [arenas][n_agents], 1 for every agent of a restarted arena — what PolicyBatch.reset_memory and the rollout
        buffer's restart mask take.  All pointers are device addresses."""
        if not hasattr(self.L, "sf_reset_arenas"):
            raise StrikeForceError("this build of libstrikeforce_amd.so has no sf_reset_arenas")
        sel = abi.ResetSel(mask_ptr, int(mask_stride), 1 if done else 0, int(max_steps), tb_ptr, serial_ptr, selected_ptr)
        self._ck(self.L.sf_reset_arenas(self.h, C.byref(sel)), "sf_reset_arenas")

    def snapshot(self, slots):
        """Device memory for `slots` arena states of this configuration (sf_snapshot_create): see Snapshot."""
        return Snapshot(self, slots)

    def signals(self):
        """Per-step vitals, deltas and a shaped reward on the device (sf_signals_create): see Signals."""
        return Signals(self)

    def action_mask_device(self, commands_ptr=None, action_string=None, actions_ptr=None):
        """sf_action_mask_device on the caller's buffers: one stream-ordered launch, nothing else.  commands_ptr / actions_ptr:
        device uint32 [arenas][n_agents]; actions_ptr needs action_string (1..32 characters of COMMANDS), and the reverse."""
        if not hasattr(self.L, "sf_action_mask_device"):
            raise StrikeForceError("this build of libstrikeforce_amd.so has no sf_action_mask_device")
        io = abi.ActionMaskIO(commands_ptr, None if action_string is None else action_string.encode(), actions_ptr)
        self._ck(self.L.sf_action_mask_device(self.h, C.byref(io)), "sf_action_mask_device")

    def action_mask(self, action_string=None):
        """Which commands would do anything right now, for every (arena, agent), on the device (sf_action_mask_device): bit k
        of a word is set when obey(COMMANDS[k]) would change the stored state ('+' always, for a present agent; an absent
        agent's word is 0).  -> an int32 tensor [arenas][n_agents] holding the bits of the unsigned words; with action_string
        (a bot's action set, e.g. "+xzqeawsd") a pair: the command words and the action words, bit j = action_string[j] —
        what PolicyBatch.act_masked takes.  The tensors are the batch's own, allocated once and rewritten by every call;
        nothing is read on the host.  The mask is of the state as stored now: the zombies, the bullets and the humans
        earlier in the sweep still move before this human's command is obeyed."""
        import torch
        own = self.__dict__.setdefault("_action_mask", {})
        for key in ("commands", "actions"):
            if key not in own and (key == "commands" or action_string is not None):
                own[key] = torch.zeros((self.cfg.arenas, self.cfg.n_agents), dtype=torch.int32, device="cuda:%d" % self.cfg.device)
        if action_string is None:
            self.action_mask_device(own["commands"].data_ptr())
            return own["commands"]
        self.action_mask_device(own["commands"].data_ptr(), action_string, own["actions"].data_ptr())
        return own["commands"], own["actions"]

    def action_mask_host(self):
        """The command words through the host (sf_action_mask): uint32 [arenas][n_agents]; synchronises."""
        out = np.zeros((self.cfg.arenas, self.cfg.n_agents), dtype=np.uint32)
        self._ck(self.L.sf_action_mask(self.h, out.ctypes.data_as(C.c_void_p)), "sf_action_mask")
        return out

    def recorder(self, bytes_per_arena, games_per_arena):
        """Games recorded on the device as `.sf_sample` command streams (sf_record_create): see Recorder."""
        return Recorder(self, bytes_per_arena, games_per_arena)

    def state_device(self, io):
        """sf_state_device with a ready abi.StateIO: one or two stream-ordered launches, nothing else."""
        if not hasattr(self.L, "sf_state_device"):
            raise StrikeForceError("this build of libstrikeforce_amd.so has no sf_state_device")
        self._ck(self.L.sf_state_device(self.h, C.byref(io)), "sf_state_device")

    def state_bytes(self, io):
        """The bytes each of the ten outputs of `io` must hold, in abi.STATE_OUTPUTS' order (sf_state_bytes)."""
        out = (C.c_int64 * 10)()
        self._ck(self.L.sf_state_bytes(self.h, C.byref(io), C.byref(out)), "sf_state_bytes")
        return [int(x) for x in out]

    def state_io(self, arena_ids=None, humans=None, zombies=None, bullets=None, portals=None, cells=False, hdr=True,
                 counts=True, digest=False):
        """The request of state_records() without the launch: (abi.StateIO, the dict state_records() returns).  Tensors,
        struct and named views are built once per shape of request and kept; a later call of the same shape returns the
        same objects (with its own arena_ids), so a loop pays for them once."""
        import torch
        cfg = self.cfg
        dev = "cuda:%d" % cfg.device
        ids = None
        if arena_ids is not None:
            ids = arena_ids if hasattr(arena_ids, "data_ptr") else torch.from_numpy(
                np.ascontiguousarray(arena_ids, dtype=np.int32).reshape(-1)).to(dev)
            if str(ids.dtype) != "torch.int32" or not ids.is_cuda or not ids.is_contiguous() or ids.dim() != 1:
                raise ValueError("arena_ids must be a contiguous one-dimensional int32 tensor on the device")
        rows = cfg.arenas if ids is None else int(ids.numel())
        cut = tuple(cap if n is None else int(n) for n, cap in ((humans, cfg.cap_humans), (zombies, cfg.cap_zombies),
                                                                (bullets, cfg.cap_bullets), (portals, cfg.cap_portals)))
        key = (rows, ids is not None, cut, bool(cells), bool(hdr), bool(counts), bool(digest))
        cache = self.__dict__.setdefault("_state_requests", {})
        if key not in cache:
            ncell = cfg.floors * cfg.rows * cfg.cols
            new = lambda shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype, device=dev)
            raw = {}
            if hdr:
                raw["hdr"] = new((rows, 40))
            for name, n, words in (("humans", cut[0], 28), ("zombies", cut[1], 7), ("bullets", cut[2], 11), ("portals", cut[3], 4)):
                if n:
                    raw[name] = new((rows, n, words))
            if cells:
                raw["cell_flags"] = new((rows, ncell), torch.uint8)
                raw["cell_dmg"], raw["cell_portal"] = new((rows, ncell)), new((rows, ncell))
            if counts:
                raw["counts"] = new((rows, abi.STATE_COUNT_WORDS))
            if digest:
                raw["digest"] = new((rows,), torch.int64)
            io = abi.StateIO()
            io.humans, io.zombies, io.bullets, io.portals = cut
            for n in abi.STATE_OUTPUTS:
                if n[2:] in raw:
                    setattr(io, n, raw[n[2:]].data_ptr())
            out = decode_state(*[raw.get(n) for n in ("hdr", "humans", "zombies", "bullets", "portals", "counts")])
            out["raw"] = raw
            cache[key] = (io, out)
        io, out = cache[key]
        if ids is not None:
            io.d_arena_ids, io.rows = ids.data_ptr(), rows
            out["arena_ids"] = ids  # (alive as long as the request: the launch may still be queued)
        return io, out

    def state_records(self, arena_ids=None, humans=None, zombies=None, bullets=None, portals=None, cells=False, hdr=True,
                      counts=True, digest=False):
        """Every arena's canonical records on the device (sf_state_device), as torch tensors that are allocated once per
        shape of request and rewritten by every later call of the same shape.  arena_ids: None (row i = arena i), a torch
        int32 tensor on the device, or a host sequence (uploaded on every call).  humans / zombies / bullets / portals:
        slots per row, None = the configuration's cap, 0 = leave the table out.  -> a dict: the raw tensors under "raw"
        (hdr int32 [rows][40], humans [rows][n][28], zombies [rows][n][7], bullets [rows][n][11], portals [rows][n][4],
        cell_flags uint8 / cell_dmg / cell_portal int32 [rows][cells], counts int32 [rows][8], digest int64 [rows]: the
        bits of the unsigned value) and the named views of decode_state().  Nothing is read on the host."""
        io, out = self.state_io(arena_ids, humans, zombies, bullets, portals, cells, hdr, counts, digest)
        self.state_device(io)
        return out

    def digest_device(self):
        """sf_state_digest's values computed on the device, in stream order: an int64 tensor [arenas] holding the bits of
        the unsigned digests (`.cpu().numpy().view(numpy.uint64)` equals digest()).  The same tensor is rewritten by every call."""
        return self.state_records(humans=0, zombies=0, bullets=0, portals=0, hdr=False, counts=False, digest=True)["raw"]["digest"]

    def state_put_device(self, io):
        """sf_state_put_device with a ready abi.StatePutIO: three stream-ordered launches, nothing else."""
        if not hasattr(self.L, "sf_state_put_device"):
            raise StrikeForceError("this build of libstrikeforce_amd.so has no sf_state_put_device")
        self._ck(self.L.sf_state_put_device(self.h, C.byref(io)), "sf_state_put_device")

    def state_put_io(self, records, row_of_arena=None, status=True, selected=False):
        """The request of put_state() without the launch: (abi.StatePutIO, the tensors it points at).  records: what
        state_records() returned or its "raw" dict — torch tensors on the device under any of hdr [rows][40], humans
        [rows][n][28], zombies [rows][n][7], bullets [rows][n][11], portals [rows][n][4] (int32; n = the table's cut) and
        cell_flags (uint8) / cell_dmg / cell_portal (int32) [rows][cells], all three or none.  row_of_arena: device int32
        [arenas], None = arena a takes row a (rows == arenas)."""
        import torch
        cfg = self.cfg
        dev = "cuda:%d" % cfg.device
        raw = dict(records.get("raw", records))
        keep = {}
        io = abi.StatePutIO()
        rows = None
        for name, words in (("hdr", 40), ("humans", 28), ("zombies", 7), ("bullets", 11), ("portals", 4),
                            ("cell_flags", None), ("cell_dmg", None), ("cell_portal", None)):
            t = raw.get(name)
            if t is None:
                continue
            want = torch.uint8 if name == "cell_flags" else torch.int32
            if t.dtype != want or not t.is_cuda or not t.is_contiguous():
                raise ValueError("%s must be a contiguous %s tensor on the device" % (name, want))
            if words is not None and t.shape[-1] != words:
                raise ValueError("%s must have %d words per record" % (name, words))
            if rows is not None and t.shape[0] != rows:
                raise ValueError("every part must have the same number of rows")
            rows = int(t.shape[0])
            if name in ("humans", "zombies", "bullets", "portals"):
                setattr(io, name, int(t.shape[1]))
            keep[name] = t
            ptr = t.data_ptr()
            if t.numel() == 0:  # a table of 0 slots is still given (its whole pool becomes empty): any valid address
                if getattr(self, "_put_nothing", None) is None:
                    self._put_nothing = torch.zeros(4, dtype=torch.int32, device=dev)
                ptr = self._put_nothing.data_ptr()
            setattr(io, "d_" + name, ptr)
        if rows is None:
            raise ValueError("no part given")
        if row_of_arena is None:
            if rows != cfg.arenas:
                raise ValueError("without row_of_arena the parts must have one row per arena")
            own = self.__dict__.setdefault("_put_identity", None)
            if own is None:
                own = self._put_identity = torch.arange(cfg.arenas, dtype=torch.int32, device=dev)
            row_of_arena = own
        elif not hasattr(row_of_arena, "data_ptr"):
            row_of_arena = torch.from_numpy(np.ascontiguousarray(row_of_arena, dtype=np.int32).reshape(-1)).to(dev)
        if row_of_arena.dtype != torch.int32 or not row_of_arena.is_cuda or row_of_arena.numel() != cfg.arenas:
            raise ValueError("row_of_arena must be an int32 tensor [arenas] on the device")
        keep["row_of_arena"] = row_of_arena
        io.d_row_of_arena, io.rows = row_of_arena.data_ptr(), rows
        own = self.__dict__.setdefault("_put_outputs", {})
        if status:
            if "status" not in own:
                own["status"] = torch.zeros((cfg.arenas,), dtype=torch.int32, device=dev)
            keep["status"], io.d_status = own["status"], own["status"].data_ptr()
        if selected:
            if "selected" not in own:
                own["selected"] = torch.zeros((cfg.arenas, cfg.n_agents), dtype=torch.uint8, device=dev)
            keep["selected"], io.d_selected = own["selected"], own["selected"].data_ptr()
        return io, keep

    def put_state(self, records, row_of_arena=None, selected=False):
        """Write arenas from canonical records on the device (sf_state_put_device), the inverse of state_records(): arena a
        takes row row_of_arena[a] of the given parts (-1: untouched; None: row a).  -> the status tensor, int32 [arenas]:
        -1 not named, 0 written, > 0 refused (abi.PUT_BAD_* bits); with selected=True a pair with the uint8
        [arenas][n_agents] mask of the agents whose arena was written (what Signals.step's rebase_ptr, the policy's
        reset_memory and the rollout buffer take).  Both tensors are the batch's own and rewritten by every call; nothing
        is read on the host."""
        io, keep = self.state_put_io(records, row_of_arena, True, selected)
        self._put_last = keep  # (alive while the launches may still be queued)
        self.state_put_device(io)
        return (keep["status"], keep["selected"]) if selected else keep["status"]

    def put_status(self):
        """Arenas written, refused and naming a row out of range since the last call (sf_state_put_status); synchronises."""
        out = (C.c_int64 * 4)()
        self._ck(self.L.sf_state_put_status(self.h, C.byref(out)), "sf_state_put_status")
        return dict(zip(abi.STATE_PUT_STATUS_FIELDS, (int(x) for x in out)))

    def load_arena(self, arena, hdr=None, humans=None, zombies=None, bullets=None, portals=None, cell_flags=None,
                   cell_dmg=None, cell_portal=None):
        """The host mirror of dump_raw(): one arena from whole pools in host memory (sf_load_arena), any part None.  hdr: an
        abi.ArenaHdr; the tables: ctypes arrays of the records or int32 numpy arrays [cap][words]; the cell tables: numpy
        uint8 / int32 [cells].  Synchronises; a refused state raises with the reason."""
        caps = {"humans": (self.cfg.cap_humans, 28), "zombies": (self.cfg.cap_zombies, 7), "bullets": (self.cfg.cap_bullets, 11),
                "portals": (self.cfg.cap_portals, 4)}
        cells = self.cfg.floors * self.cfg.rows * self.cfg.cols
        hold, args = [], []
        for name, x in (("hdr", hdr), ("humans", humans), ("zombies", zombies), ("bullets", bullets), ("portals", portals),
                        ("cell_flags", cell_flags), ("cell_dmg", cell_dmg), ("cell_portal", cell_portal)):
            if x is None:
                args.append(None)
                continue
            if isinstance(x, np.ndarray) or name.startswith("cell"):
                x = np.ascontiguousarray(x, dtype=np.uint8 if name == "cell_flags" else np.int32)
                n = 40 if name == "hdr" else cells if name.startswith("cell") else caps[name][0] * caps[name][1]
                if x.size != n:
                    raise ValueError("%s must hold the whole pool (%d values)" % (name, n))
                hold.append(x)
                args.append(x.ctypes.data)
            else:
                if name in caps and len(x) != caps[name][0]:
                    raise ValueError("%s must hold the whole pool (%d records)" % (name, caps[name][0]))
                hold.append(x)
                args.append(C.addressof(x))
        self._ck(self.L.sf_load_arena(self.h, int(arena), *args), "sf_load_arena")

    def snapshot_slot_bytes(self):
        """(device bytes, blob bytes) one snapshot slot of this configuration takes: to budget before snapshot()."""
        if not hasattr(self.L, "sf_snapshot_create"):
            raise StrikeForceError("this build of libstrikeforce_amd.so has no sf_snapshot_* entry points")
        d, b = C.c_int64(0), C.c_int64(0)
        self._ck(self.L.sf_snapshot_slot_bytes(self.h, C.byref(d), C.byref(b)), "sf_snapshot_slot_bytes")
        return int(d.value), int(b.value)

    def step(self, cmd):
        cmd = np.ascontiguousarray(cmd, dtype=np.uint8)
        if cmd.size != self.cfg.arenas * self.cfg.n_agents:
            raise ValueError("cmd must hold arenas * n_agents command chars")
        self._ck(self.L.sf_step(self.h, cmd.ctypes.data_as(C.c_char_p)), "sf_step")

    def step_begin(self):
        """The first half of one iteration (gameplay.hpp:1455-1463): up to where the reference asks the agents of humans
        other than `ind` for their command."""
        self._ck(self.L.sf_step_begin(self.h), "sf_step_begin")

    def step_end(self, cmd):
        """The second half (gameplay.hpp:1464-1471) and the next loop top; cmd as for step()."""
        cmd = np.ascontiguousarray(cmd, dtype=np.uint8)
        if cmd.size != self.cfg.arenas * self.cfg.n_agents:
            raise ValueError("cmd must hold arenas * n_agents command chars")
        self._ck(self.L.sf_step_end(self.h, cmd.ctypes.data_as(C.c_char_p)), "sf_step_end")

    def step_end_device(self, d_cmd_ptr):
        self._ck(self.L.sf_step_end_device(self.h, C.c_void_p(d_cmd_ptr)), "sf_step_end_device")

    def agent_alive(self):
        """[arenas][n_agents] uint8: 1 while the commanded human is alive and still has its Agent (Human::active_agent)."""
        out = np.zeros((self.cfg.arenas, self.cfg.n_agents), dtype=np.uint8)
        self._ck(self.L.sf_agent_alive(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8))), "sf_agent_alive")
        return out

    def phase_draws(self, arena=None):
        """Generator draws of the last step by phase [zombie_action, update_bull, human_action, update_bull, spawns, rest]:
        of one arena (a list of six ints) or of all ([arenas][6] int32)."""
        out = np.zeros((self.cfg.arenas, 6), dtype=np.int32)
        self._ck(self.L.sf_phase_draws(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))), "sf_phase_draws")
        return out if arena is None else [int(x) for x in out[arena]]

    def agent_alive_device(self, d_out_ptr):
        self._ck(self.L.sf_agent_alive_device(self.h, C.c_void_p(d_out_ptr)), "sf_agent_alive_device")

    def comm_ranks(self):
        n = C.c_int32(0)
        self._ck(self.L.sf_comm_ranks(self.h, C.byref(n)), "sf_comm_ranks")
        return int(n.value)

    def step_device(self, d_cmd_ptr, k):
        """k loop iterations in one launch; d_cmd_ptr: device address of uint8 [k][arenas][n_agents]."""
        self._ck(self.L.sf_step_device(self.h, C.c_void_p(d_cmd_ptr), k), "sf_step_device")

    def observe(self):
        out = np.empty((self.cfg.arenas, self.cfg.n_agents, abi.OBS_CHANNELS, abi.OBS_WINDOW, abi.OBS_WINDOW),
                       dtype=np.float32)
        self._ck(self.L.sf_observe(self.h, out.ctypes.data_as(C.POINTER(C.c_float))), "sf_observe")
        return out

    def observe_device_delta(self, d_out_ptr):
        """observe_device for ONE persistent, caller-untouched buffer per env: only what changed is written."""
        self._ck(self.L.sf_observe_device_delta(self.h, C.c_void_p(d_out_ptr)), "sf_observe_device_delta")

    def observe_sparse_device(self, d_keys_ptr, d_vals_ptr, d_counts_ptr, d_pov_ptr, cap):
        """The observation as the list of its non-zero floats ([agents][cap] keys and values, [agents] counts,
        [agents][160] centre values): what PolicyBatch.forward_sparse consumes."""
        self._ck(self.L.sf_observe_sparse_device(self.h, C.c_void_p(d_keys_ptr), C.c_void_p(d_vals_ptr), C.c_void_p(d_counts_ptr),
                                                 C.c_void_p(d_pov_ptr), int(cap)), "sf_observe_sparse_device")

    def observe_overflow_device(self, d_counts_ptr, cap, d_dense_ptr, d_pov_ptr):
        """Right behind observe_sparse_device, same counts / cap: the dense observation of exactly the agents whose list
        did not fit, into their rows of d_dense ([agents][32][31][31]); their d_pov rows are rewritten from it."""
        self._ck(self.L.sf_observe_overflow_device(self.h, C.c_void_p(d_counts_ptr), int(cap), C.c_void_p(d_dense_ptr),
                                                   C.c_void_p(d_pov_ptr)), "sf_observe_overflow_device")

    def observe_device(self, d_out_ptr):
        self._ck(self.L.sf_observe_device(self.h, C.c_void_p(d_out_ptr)), "sf_observe_device")

    def results(self):
        out = np.zeros((self.cfg.arenas, self.cfg.n_agents, 8), dtype=np.int32)
        self._ck(self.L.sf_results(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))), "sf_results")
        return out

    def results_device(self, d_out_ptr):
        self._ck(self.L.sf_results_device(self.h, C.c_void_p(d_out_ptr)), "sf_results_device")

    @staticmethod
    def comm_unique_id():
        """128 opaque bytes from rank 0 (ncclGetUniqueId through the library's own RCCL): hand them to every rank."""
        L = load_library()
        buf = C.create_string_buffer(128)
        rc = L.sf_comm_unique_id(buf)
        if rc != 0:
            raise StrikeForceError("sf_comm_unique_id failed (%d): %s" % (rc, L.sf_last_error().decode()))
        return buf.raw

    def comm_init(self, uid, rank, world):
        self._ck(self.L.sf_comm_init(self.h, uid, rank, world), "sf_comm_init")

    def results_allgather(self, d_out_ptr):
        """RCCL all-gather of every rank's result records into [world][arenas][agents][8] int32, on a side stream."""
        self._ck(self.L.sf_results_allgather(self.h, C.c_void_p(d_out_ptr)), "sf_results_allgather")

    def comm_wait(self, host_too=False):
        self._ck(self.L.sf_comm_wait(self.h, 1 if host_too else 0), "sf_comm_wait")

    # ---- episode log (strikeforce.h sf_episode_log) ----
    @property
    def episode_record_words(self):
        return episode_record_words(self.cfg.n_agents)

    def _need_log(self):
        if not hasattr(self.L, "sf_episode_log"):
            raise StrikeForceError("this build of libstrikeforce_amd.so has no episode log")

    def enable_episode_log(self, depth):
        """Keep the last `depth` (a power of two in [1, 64]) finished episodes of every arena in a device ring; 0 turns
        the log off.  Only episodes that end from now on are offered."""
        self._need_log()
        self._ck(self.L.sf_episode_log(self.h, int(depth)), "sf_episode_log")
        self.episode_depth = int(depth)

    def episodes(self, max_records=None):
        """The finished episodes not delivered yet: (records int32 [n][record words], (written, lost, pending)).
        max_records=None: as many as the rings can hold."""
        self._need_log()
        if max_records is None:
            max_records = self.cfg.arenas * getattr(self, "episode_depth", 64)
        out = np.zeros((max(int(max_records), 0), self.episode_record_words), dtype=np.int32)
        counts = np.zeros(3, dtype=np.int32)
        self._ck(self.L.sf_episodes(self.h, C.c_void_p(out.ctypes.data), int(max_records), C.c_void_p(counts.ctypes.data)),
                 "sf_episodes")
        return out[:counts[0]], (int(counts[0]), int(counts[1]), int(counts[2]))

    def episodes_device(self, d_out_ptr, max_records, d_counts_ptr):
        """The same on the device, no host synchronisation: d_out int32 [max_records][record words], d_counts int32 [3]."""
        self._need_log()
        self._ck(self.L.sf_episodes_device(self.h, C.c_void_p(d_out_ptr), int(max_records), C.c_void_p(d_counts_ptr)),
                 "sf_episodes_device")

    def episode_ring(self):
        """The raw rings, int32 [arenas][depth][record words]; empty slots have episode == -1."""
        self._need_log()
        out = np.zeros((self.cfg.arenas, getattr(self, "episode_depth", 0), self.episode_record_words), dtype=np.int32)
        self._ck(self.L.sf_episode_ring(self.h, C.c_void_p(out.ctypes.data)), "sf_episode_ring")
        return out

    def episodes_allgather(self, d_out_ptr):
        """RCCL all-gather of every rank's raw rings into [world][arenas][depth][record words] int32, on a side stream."""
        self._need_log()
        self._ck(self.L.sf_episodes_allgather(self.h, C.c_void_p(d_out_ptr)), "sf_episodes_allgather")

    # ---- replay of logged games (strikeforce.h sf_replay_load) ----
    def _need_replay(self):
        if not hasattr(self.L, "sf_replay_load"):
            raise StrikeForceError("this build of libstrikeforce_amd.so has no sf_replay_* entry points")

    def replay_load(self, streams):
        """One command stream per arena — str / bytes of reference command chars in file order, or objects with a
        `.commands` attribute (replay.Sample) — uploaded to the device, every cursor at its stream's start.  None frees
        them.  Needs auto_reset == 0; the seeds are reset()'s."""
        self._need_replay()
        if streams is None:
            self._ck(self.L.sf_replay_load(self.h, None, None), "sf_replay_load")
            return
        rows = [getattr(s, "commands", s) for s in streams]
        rows = [r.encode("ascii") if isinstance(r, str) else bytes(r) for r in rows]
        if len(rows) != self.cfg.arenas:
            raise ValueError("replay_load takes one command stream per arena")
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(r) for r in rows])
        flat = np.frombuffer(b"".join(rows) or b"\0", dtype=np.uint8)
        self._ck(self.L.sf_replay_load(self.h, C.c_void_p(flat.ctypes.data), C.c_void_p(off.ctypes.data)), "sf_replay_load")

    def replay_step(self):
        """One iteration of every arena, the commands fetched from the loaded streams on the device (no host round trip)."""
        self._need_replay()
        self._ck(self.L.sf_replay_step(self.h), "sf_replay_step")

    def replay_status(self):
        """int32 [arenas][4]: state (abi.REPLAY_*), cursor (lines taken), iterations played, 0."""
        self._need_replay()
        out = np.zeros((self.cfg.arenas, 4), dtype=np.int32)
        self._ck(self.L.sf_replay_status(self.h, C.c_void_p(out.ctypes.data)), "sf_replay_status")
        return out

    def replay_status_device(self, d_out_ptr):
        self._need_replay()
        self._ck(self.L.sf_replay_status_device(self.h, C.c_void_p(d_out_ptr)), "sf_replay_status_device")

    def replay_commands_device(self, d_out_ptr):
        """uint8 [arenas][n_agents] on the device: the line each commanded human took in the last iteration, 0 where none."""
        self._need_replay()
        self._ck(self.L.sf_replay_commands_device(self.h, C.c_void_p(d_out_ptr)), "sf_replay_commands_device")

    def done_device(self, d_out_ptr):
        """check_end()'s verdict on the device, one byte per (arena, agent): what PolicyBatch.reset_memory takes."""
        self._ck(self.L.sf_done_device(self.h, C.c_void_p(d_out_ptr)), "sf_done_device")

    def done_view_device(self):
        """The same flags where the library keeps them: (device pointer, int32 stride, agents per arena) — what
        PolicyBatch.predict_sparse reads in place (reset_words=)."""
        ptr, stride, group = C.c_void_p(), C.c_int32(), C.c_int32()
        self._ck(self.L.sf_done_view_device(self.h, C.byref(ptr), C.byref(stride), C.byref(group)), "sf_done_view_device")
        return ptr.value, stride.value, group.value

    def done(self):
        out = np.zeros(self.cfg.arenas, dtype=np.uint8)
        self._ck(self.L.sf_done(self.h, out.ctypes.data_as(C.POINTER(C.c_uint8))), "sf_done")
        return out

    def digest(self):
        out = np.zeros(self.cfg.arenas, dtype=np.uint64)
        self._ck(self.L.sf_state_digest(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64))), "sf_state_digest")
        return out

    def dump_raw(self, arena):
        cfg = self.cfg
        cells = cfg.floors * cfg.rows * cfg.cols
        hdr = abi.ArenaHdr()
        hs = (abi.HumanRec * cfg.cap_humans)()
        zs = (abi.ZombieRec * cfg.cap_zombies)()
        bs = (abi.BulletRec * cfg.cap_bullets)()
        ps = (abi.PortalRec * cfg.cap_portals)()
        flags = np.zeros(cells, dtype=np.uint8)
        dmg = np.zeros(cells, dtype=np.int32)
        pidx = np.zeros(cells, dtype=np.int32)
        self._ck(self.L.sf_dump_arena(self.h, arena, C.byref(hdr), hs, zs, bs, ps,
                                      flags.ctypes.data_as(C.POINTER(C.c_uint8)),
                                      dmg.ctypes.data_as(C.POINTER(C.c_int32)),
                                      pidx.ctypes.data_as(C.POINTER(C.c_int32))), "sf_dump_arena")
        return hdr, list(hs), list(zs), list(bs), list(ps), flags, dmg, pidx

    def dump(self, arena):
        """dump_raw() as an object with named fields (hdr, humans, zombies, bullets, portals, flags, dmg, pidx)."""
        import types
        hdr, hs, zs, bs, ps, flags, dmg, pidx = self.dump_raw(arena)
        return types.SimpleNamespace(hdr=hdr, humans=hs, zombies=zs, bullets=bs, portals=ps, flags=flags, dmg=dmg,
                                     pidx=pidx)

    def step_kernel(self):
        """Index of the fixed-shape kernel the last step launch ran (csrc/sf_types.hpp FixedShapes), -1: a generic instance."""
        i = C.c_int32(-2)
        self._ck(self.L.sf_step_kernel(self.h, C.byref(i)), "sf_step_kernel")
        return i.value

    def kernel_time(self, enable=True):
        """(ms, launches) of the step kernels since the last call, from HIP events on the launch stream."""
        ms, n = C.c_float(0), C.c_int32(0)
        self._ck(self.L.sf_kernel_time(self.h, 1 if enable else 0, C.byref(ms), C.byref(n)), "sf_kernel_time")
        return ms.value, n.value
