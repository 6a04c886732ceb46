"""The device rollout buffer (include/strikeforce_policy.h, sf_rollout_*): bot-1's T-step record, returns and advantages.

One reference `Agent` keeps `states, log_probs, values, rewards, actions` per game (bots/bot-1/Agent.hpp:200-204,227,
233-234,301-302), fills them for T ticks and then runs computeReturns() (:333-339) and train_log() (:341-351) over them.
``RolloutBatch`` does that for every agent of a batch behind ``PolicyBatch.predict_sparse`` and
``RewardBatch.reward_sparse``: it allocates the storage as torch tensors (slot-major, ``[T][agents]...``, exposed as
attributes), records one tick per call, and hands the learner returns, log V, advantages and the statistics of the agents
whose buffer is full.  The learners themselves (gradients, AdamW, backups) are the caller's.  No CPU path.

That is the reference's rule, one buffer per game: a restart rewinds the agent to slot 0.  ``RolloutBatch(...,
continuing=True)`` is the buffer of a learner that trains on fixed blocks instead (sf_rollout_continue): every tick is kept,
a restart is stored in ``first`` and never moves the cursor, and ``gae()`` (sf_rollout_gae) computes GAE(lambda) returns,
values and advantages over a full block, bootstrapped from the value of the state behind it, game ends cutting the recursion.
"""
import ctypes as C

from . import env, policy

HIDDEN, ACTIONS = policy.HIDDEN, policy.ACTIONS

# every sf_rollout_* symbol include/strikeforce_policy.h declares (sf_policy_update_actions is in policy.EXPORTS)
EXPORTS = ["sf_rollout_create", "sf_rollout_destroy", "sf_rollout_set_stream", "sf_rollout_synchronize", "sf_rollout_record",
           "sf_rollout_fill_device", "sf_rollout_ready_device", "sf_rollout_status", "sf_rollout_returns", "sf_rollout_release",
           "sf_rollout_state", "sf_rollout_continue", "sf_rollout_gae", "sf_rollout_dense"]

# sf_rollout_dense: element types, layouts, the row cap and a row's elements (include/strikeforce_policy.h)
DENSE_F32, DENSE_BF16, DENSE_F16 = 0, 1, 2
DENSE_NCHW, DENSE_NHWC = 0, 1
DENSE_ROWS_MAX = 16384
DENSE_ROW = 32 * 31 * 31


class Buffers(C.Structure):
    """sf_rollout_buffers."""
    _fields_ = [("keys", C.c_void_p), ("vals", C.c_void_p), ("counts", C.c_void_p), ("pov", C.c_void_p), ("action", C.c_void_p),
                ("logp", C.c_void_p), ("value", C.c_void_p), ("reward", C.c_void_p), ("disc", C.c_void_p), ("imitate", C.c_void_p)]


class Step(C.Structure):
    """sf_rollout_step."""
    _fields_ = [("d_keys", C.c_void_p), ("d_vals", C.c_void_p), ("d_counts", C.c_void_p), ("d_pov", C.c_void_p), ("cap", C.c_int32),
                ("agents", C.c_int32), ("d_probs", C.c_void_p), ("d_value", C.c_void_p), ("d_action", C.c_void_p),
                ("d_reward", C.c_void_p), ("d_disc", C.c_void_p), ("d_imitate", C.c_void_p), ("d_reset_mask", C.c_void_p),
                ("d_reset_words", C.c_void_p), ("reset_stride", C.c_int32), ("reset_group", C.c_int32)]


class GaeIO(C.Structure):
    """sf_rollout_gae_io."""
    _fields_ = [("gamma", C.c_float), ("lam", C.c_float), ("reward_scale", C.c_float), ("log_values", C.c_int32),
                ("d_next_value", C.c_void_p), ("d_next_mask", C.c_void_p), ("d_next_words", C.c_void_p), ("next_stride", C.c_int32),
                ("next_group", C.c_int32), ("d_returns", C.c_void_p), ("d_v", C.c_void_p), ("d_adv", C.c_void_p)]


class DenseIO(C.Structure):
    """sf_rollout_dense_io."""
    _fields_ = [("d_cells", C.c_void_p), ("slot", C.c_int32), ("agent0", C.c_int32), ("rows", C.c_int32), ("dtype", C.c_int32),
                ("layout", C.c_int32), ("d_dense", C.c_void_p), ("d_valid", C.c_void_p)]


def _bind(L):
    if getattr(L, "_sf_rollout_bound", False):
        return
    vp, pp = C.c_void_p, C.POINTER(C.c_void_p)
    L.sf_rollout_create.argtypes = [C.POINTER(Buffers), C.c_int32, C.c_int32, C.c_int32, C.c_int32, pp]
    L.sf_rollout_destroy.argtypes = [vp]
    L.sf_rollout_destroy.restype = None
    L.sf_rollout_set_stream.argtypes = [vp, vp]
    L.sf_rollout_synchronize.argtypes = [vp]
    L.sf_rollout_record.argtypes = [vp, C.POINTER(Step)]
    L.sf_rollout_fill_device.argtypes = [vp, pp]
    L.sf_rollout_ready_device.argtypes = [vp, vp]
    L.sf_rollout_status.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.sf_rollout_returns.argtypes = [vp, C.c_float, vp, vp, vp, vp]
    L.sf_rollout_release.argtypes = [vp, vp]
    L.sf_rollout_state.argtypes = [vp, C.c_int32, pp, pp, pp, pp, C.POINTER(C.c_int32)]
    if hasattr(L, "sf_rollout_gae"):  # (an older build loaded through SF_LIBRARY_PATH lacks them)
        L.sf_rollout_continue.argtypes = [vp, vp]
        L.sf_rollout_gae.argtypes = [vp, C.POINTER(GaeIO)]
    if hasattr(L, "sf_rollout_dense"):
        L.sf_rollout_dense.argtypes = [vp, C.POINTER(DenseIO)]
    for n in EXPORTS:
        if n != "sf_rollout_destroy" and hasattr(L, n):
            getattr(L, n).restype = C.c_int
    L._sf_rollout_bound = True


class RolloutBatch:
    """The five vectors of `agents` reference Agents, T slots each.  Tensors (device, slot-major): keys, vals
    [T][agents][list_cap], counts [T][agents], pov [T][agents][160] (None with store_states=False), action [T][agents]
    int32, logp [T][agents][9], value, reward [T][agents], disc [T][agents] and imitate [T][agents] uint8 (None unless
    asked for).  continuing=True: the buffer spans game ends (sf_rollout_continue) — a restart flag never rewinds an agent,
    it is stored in `first` [T][agents] uint8, and every T ticks all agents that recorded every tick are ready."""

    def __init__(self, agents, T, list_cap, store_states=True, store_disc=False, store_imitate=False, device=0, continuing=False):
        import torch
        self.L = env.load_library()
        if not hasattr(self.L, "sf_rollout_create"):
            raise env.StrikeForceError("libstrikeforce_amd.so has no rollout buffer: rebuild it (python -m strikeforce_amd.build)")
        _bind(self.L)
        self.agents, self.T, self.list_cap = int(agents), int(T), int(list_cap)
        self.h = None
        if torch.cuda.is_available() and self.agents >= 1 and self.T >= 1 and self.list_cap >= 1:
            dev = torch.device("cuda", int(device))
            new = lambda shape, dtype: torch.zeros((self.T, self.agents) + shape, dtype=dtype, device=dev)
            f32, i32 = torch.float32, torch.int32
            self.keys = new((self.list_cap,), i32) if store_states else None
            self.vals = new((self.list_cap,), f32) if store_states else None
            self.counts = new((), i32) if store_states else None
            self.pov = new((HIDDEN,), f32) if store_states else None
            self.action, self.logp, self.value, self.reward = new((), i32), new((ACTIONS,), f32), new((), f32), new((), f32)
            self.disc = new((), f32) if store_disc else None
            self.imitate = new((), torch.uint8) if store_imitate else None
            self.first = new((), torch.uint8) if continuing else None
            ptr = lambda t: t.data_ptr() if t is not None else None
        else:  # (no device, or sizes no tensor can have: the library says which — SF_ERR_DEVICE / SF_ERR_ARG)
            self.keys = self.vals = self.counts = self.pov = self.disc = self.imitate = None
            self.action = self.logp = self.value = self.reward = self.first = None
            ptr, dev = (lambda t: None), None
        b = Buffers(ptr(self.keys), ptr(self.vals), ptr(self.counts), ptr(self.pov), ptr(self.action), ptr(self.logp), ptr(self.value),
                    ptr(self.reward), ptr(self.disc), ptr(self.imitate))
        h = C.c_void_p()
        rc = self.L.sf_rollout_create(C.byref(b), self.agents, self.T, self.list_cap, int(device), C.byref(h))
        if rc != 0:
            raise env.StrikeForceError("sf_rollout_create failed (%d): %s" % (rc, self.L.sf_last_error().decode()))
        self.h = h
        self._torch, self._dev = torch, dev
        if continuing:
            if not hasattr(self.L, "sf_rollout_continue"):
                raise env.StrikeForceError("this build of libstrikeforce_amd.so has no sf_rollout_continue")
            self._ck(self.L.sf_rollout_continue(self.h, C.c_void_p(self.first.data_ptr())), "sf_rollout_continue")

    def _ck(self, rc, what):
        if rc != 0:
            raise env.StrikeForceError("%s failed (%d): %s" % (what, rc, self.L.sf_last_error().decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.sf_rollout_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream):
        self._ck(self.L.sf_rollout_set_stream(self.h, C.c_void_p(hip_stream)), "sf_rollout_set_stream")

    def synchronize(self):
        self._ck(self.L.sf_rollout_synchronize(self.h), "sf_rollout_synchronize")

    def record(self, d_probs_ptr, d_value_ptr, d_action_ptr, d_reward_ptr, d_keys_ptr=None, d_vals_ptr=None, d_counts_ptr=None,
               d_pov_ptr=None, cap=0, agents=None, d_disc_ptr=None, d_imitate_ptr=None, d_reset_mask_ptr=None, reset_words=None):
        """One tick: PolicyBatch.predict_sparse's probabilities, value and action, RewardBatch.reward_sparse's reward (and D),
        the observation lists both read, and the restart flags both were given.  One launch on this object's stream."""
        io = Step()
        io.d_keys, io.d_vals, io.d_counts, io.d_pov, io.cap = d_keys_ptr, d_vals_ptr, d_counts_ptr, d_pov_ptr, int(cap)
        io.agents = self.agents if agents is None else int(agents)
        io.d_probs, io.d_value, io.d_action, io.d_reward = d_probs_ptr, d_value_ptr, d_action_ptr, d_reward_ptr
        io.d_disc, io.d_imitate, io.d_reset_mask = d_disc_ptr, d_imitate_ptr, d_reset_mask_ptr
        if reset_words is not None:
            io.d_reset_words, io.reset_stride, io.reset_group = reset_words
        self._ck(self.L.sf_rollout_record(self.h, C.byref(io)), "sf_rollout_record")

    def fill(self):
        """The cursors as a device tensor view (int32 per agent, the library's memory: read it, do not write it)."""
        p = C.c_void_p()
        self._ck(self.L.sf_rollout_fill_device(self.h, C.byref(p)), "sf_rollout_fill_device")
        if not hasattr(self, "_fill"):
            iface = {"shape": (self.agents,), "typestr": "<i4", "data": (p.value, False), "version": 2}
            holder = type("FillView", (), {"__cuda_array_interface__": iface})()
            self._fill = self._torch.as_tensor(holder, device=self._dev)
        return self._fill

    def ready_mask(self, out=None):
        """uint8 per agent, 1 = its buffer is full: what reset_memory and release take."""
        if out is None:
            out = self._torch.empty(self.agents, dtype=self._torch.uint8, device=self._dev)
        self._ck(self.L.sf_rollout_ready_device(self.h, C.c_void_p(out.data_ptr())), "sf_rollout_ready_device")
        return out

    def status(self):
        """(ready agents now, ticks dropped on ready agents, states stored with a list that did not fit); synchronises."""
        r, d, m = C.c_int32(), C.c_int64(), C.c_int64()
        self._ck(self.L.sf_rollout_status(self.h, C.byref(r), C.byref(d), C.byref(m)), "sf_rollout_status")
        return r.value, d.value, m.value

    def returns(self, gamma=0.99, out=None):
        """computeReturns(), log V, the advantage and train_log()'s four numbers for the ready agents: (returns, logv, adv
        [T][agents], stats [agents][4]).  Rows of agents that are not ready are not written (new tensors hold NaN there)."""
        t = self._torch
        if out is None:
            nan = lambda shape: t.full(shape, float("nan"), dtype=t.float32, device=self._dev)
            out = (nan((self.T, self.agents)), nan((self.T, self.agents)), nan((self.T, self.agents)), nan((self.agents, 4)))
        self._ck(self.L.sf_rollout_returns(self.h, C.c_float(gamma), *[C.c_void_p(x.data_ptr()) if x is not None else None for x in out]),
                 "sf_rollout_returns")
        return out

    def gae(self, gamma, lam, reward_scale=1.0, log_values=False, next_value=None, next_mask=None, next_words=None, out=None):
        """GAE(lambda) over the ready agents' buffers (sf_rollout_gae): (returns, v, adv), [T][agents] each; game ends inside
        the buffer (`first`) cut the recursion.  next_value: device float32 per agent (a tensor or its address), the value
        head's output for the state behind slot T - 1, None: no bootstrap; next_mask (uint8 per agent) or next_words
        (ArenaBatch.done_view_device()'s triple): that tick's restart flags.  log_values: V is the f32 log of the stored
        value, as the reference's head has it.  out: three tensors, each may be None.  Rows of agents that are not ready
        are not written (new tensors hold NaN there)."""
        t = self._torch
        if out is None:
            nan = lambda: t.full((self.T, self.agents), float("nan"), dtype=t.float32, device=self._dev)
            out = (nan(), nan(), nan())
        ptr = lambda x: None if x is None else C.c_void_p(x if isinstance(x, int) else x.data_ptr())
        io = GaeIO()
        io.gamma, io.lam, io.reward_scale, io.log_values = gamma, lam, reward_scale, 1 if log_values else 0
        io.d_next_value, io.d_next_mask = ptr(next_value), ptr(next_mask)
        if next_words is not None:
            io.d_next_words, io.next_stride, io.next_group = next_words
        io.d_returns, io.d_v, io.d_adv = (ptr(x) for x in out)
        self._ck(self.L.sf_rollout_gae(self.h, C.byref(io)), "sf_rollout_gae")
        return out

    def dense(self, t=None, cells=None, agent0=0, rows=None, dtype=None, channels_last=False, out=None, valid=None):
        """Stored observation lists as the dense rows a torch module reads (sf_rollout_dense): (dense, valid).  Rows: the
        cells in `cells` (an int32 device tensor of t * agents + agent, any order), or agents agent0 .. agent0 + rows - 1 of
        slot t (rows None: all behind agent0).  dense: [rows, 32, 31, 31] of dtype (torch.float32, the default, bfloat16 or
        float16); with channels_last the memory is [rows, 31, 31, 32] and the tensor returned is its NCHW view, torch's
        channels_last format.  valid: uint8 per row, 0 where the stored list did not fit (or the cell is outside the buffer)
        and the row is all zero.  out / valid: tensors to write into (out: contiguous in the layout asked for, 16-byte
        aligned, at least rows * 30752 elements).  At most DENSE_ROWS_MAX rows per call: walk a larger batch in chunks.
        One launch on this object's stream."""
        tc = self._torch
        if not hasattr(self.L, "sf_rollout_dense"):
            raise env.StrikeForceError("this build of libstrikeforce_amd.so has no sf_rollout_dense")
        dtype = tc.float32 if dtype is None else dtype
        codes = {tc.float32: DENSE_F32, tc.bfloat16: DENSE_BF16, tc.float16: DENSE_F16}
        if dtype not in codes:
            raise ValueError("dense: dtype must be torch.float32, torch.bfloat16 or torch.float16")
        if (cells is None) == (t is None):
            raise ValueError("dense: give a slot t or a tensor of cells, not both")
        if cells is not None:
            if cells.dtype != tc.int32 or not cells.is_cuda or not cells.is_contiguous():
                raise ValueError("dense: cells must be a contiguous int32 device tensor")
            rows = cells.numel() if rows is None else int(rows)
            if rows > cells.numel():
                raise ValueError("dense: more rows than cells")
        elif rows is None:
            rows = self.agents - int(agent0)
        rows = int(rows)
        if rows > DENSE_ROWS_MAX:
            raise ValueError("dense: %d rows, at most %d per call (walk them in chunks)" % (rows, DENSE_ROWS_MAX))
        if out is None and rows >= 1:
            shape = (rows, 31, 31, 32) if channels_last else (rows, 32, 31, 31)
            out = tc.empty(shape, dtype=dtype, device=self._dev)
        if out is not None:
            if out.dtype != dtype or out.numel() < rows * DENSE_ROW:
                raise ValueError("dense: out must hold rows * 30752 elements of the dtype asked for")
            if not (out.permute(0, 2, 3, 1) if channels_last and out.dim() == 4 and out.shape[1] == 32 else out).is_contiguous():
                raise ValueError("dense: out is not contiguous in the layout asked for")
        if valid is None and rows >= 1:
            valid = tc.empty(rows, dtype=tc.uint8, device=self._dev)
        elif valid is not None and (valid.dtype != tc.uint8 or valid.numel() < rows or not valid.is_contiguous()):
            raise ValueError("dense: valid must be a contiguous uint8 tensor of at least `rows` elements")
        io = DenseIO()
        io.d_cells = None if cells is None else cells.data_ptr()
        io.slot, io.agent0, io.rows = (0 if t is None else int(t)), int(agent0), rows
        io.dtype, io.layout = codes[dtype], DENSE_NHWC if channels_last else DENSE_NCHW
        io.d_dense = None if out is None else out.data_ptr()
        io.d_valid = None if valid is None else valid.data_ptr()
        self._ck(self.L.sf_rollout_dense(self.h, C.byref(io)), "sf_rollout_dense")
        if channels_last and out.dim() == 4 and out.shape[-1] == 32 and out.shape[1] != 32:
            out = out.permute(0, 3, 1, 2)  # the NCHW view of [rows, 31, 31, 32]
        return out, valid

    def release(self, mask=None):
        """clear(): every ready agent starts at slot 0 again; with a mask (device uint8 per agent, or its address), the agents
        it names, ready or not."""
        m = None if mask is None else C.c_void_p(mask if isinstance(mask, int) else mask.data_ptr())
        self._ck(self.L.sf_rollout_release(self.h, m), "sf_rollout_release")

    def state(self, t):
        """(d_keys, d_vals, d_counts, d_pov, cap) of slot t: the leading arguments of forward_sparse / reward_sparse."""
        k, v, c, p, cap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32()
        self._ck(self.L.sf_rollout_state(self.h, int(t), C.byref(k), C.byref(v), C.byref(c), C.byref(p), C.byref(cap)), "sf_rollout_state")
        return k.value, v.value, c.value, p.value, cap.value
