"""ctypes plumbing for the on-device policy network (include/strikeforce_policy.h).

``PolicyBatch`` evaluates the reference's bot network (bots/bot-0.5/Modules.hpp:54-179) for every agent of an
arena batch on the GPU, straight from the observation buffer ``ArenaBatch.observe_device`` wrote.  Parameters are
passed as a dict of float32 numpy arrays keyed by the reference's parameter names (``named_parameters()`` of
``AgentModel``); ``init_parameters`` makes a random set with torch's default initialisers for the same shapes.
``RewardBatch`` does the same for the second network bot-1 runs every tick, the GAIL discriminator RewardModel
(bots/bot-1/RewardNet.hpp:138-167): D and log D, the per-step reward, from the observation and the action just drawn.
There is no CPU path: without the HIP library / a GPU this raises.
"""
import ctypes as C

import numpy as np

from . import env

HIDDEN, ACTIONS, CONVS, RES_LAYERS = 160, 9, 4, 3
OBS_CHANNELS, OBS_WINDOW = 32, 31
ACTION_STRING = "+xzqeawsd"  # gameplay::prepare, bots/bot-0.5/Custom.hpp:162
POLICY_ABI_VERSION = 1

_FP = C.POINTER(C.c_float)


class Weights(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("conv_w", _FP * CONVS),
        ("gru_w_ih", _FP * 2), ("gru_w_hh", _FP * 2), ("gru_b_ih", _FP * 2), ("gru_b_hh", _FP * 2),
        ("comb_w", _FP), ("comb_b", _FP),
        ("value_res_w", _FP * RES_LAYERS), ("value_res_b", _FP * RES_LAYERS), ("value_w", _FP), ("value_b", _FP),
        ("policy_res_w", _FP * RES_LAYERS), ("policy_res_b", _FP * RES_LAYERS), ("policy_w", _FP), ("policy_b", _FP),
    ]


def parameter_shapes():
    """name -> shape, the names and shapes of AgentModel's parameters (Modules.hpp:37,62,87-91,147-152)."""
    s = {}
    for i in range(CONVS):
        s["backbone.cnn.conv%d.weight" % i] = (HIDDEN, OBS_CHANNELS if i == 0 else HIDDEN, 3, 3)
    for g in range(2):
        s["backbone.gru%d.weight_ih_l0" % g] = (3 * HIDDEN, HIDDEN)
        s["backbone.gru%d.weight_hh_l0" % g] = (3 * HIDDEN, HIDDEN)
        s["backbone.gru%d.bias_ih_l0" % g] = (3 * HIDDEN,)
        s["backbone.gru%d.bias_hh_l0" % g] = (3 * HIDDEN,)
    s["backbone.combined_processor.0.weight"] = (HIDDEN, 2 * HIDDEN + ACTIONS)
    s["backbone.combined_processor.0.bias"] = (HIDDEN,)
    for head, n_out in (("value", 1), ("policy", ACTIONS)):
        for i in range(RES_LAYERS):
            s["%s.0.lin%d.weight" % (head, i)] = (HIDDEN, HIDDEN)
            s["%s.0.lin%d.bias" % (head, i)] = (HIDDEN,)
        s["%s.1.weight" % head] = (n_out, HIDDEN)
        s["%s.1.bias" % head] = (n_out,)
    return s


def reward_parameter_shapes():
    """name -> shape of bot-1's RewardModel (bots/bot-1/RewardNet.hpp:138-151): AgentModel's backbone.* and value.*
    under the same names (value.0.lin{i}.*, value.1.*); it has no policy head."""
    return {k: v for k, v in parameter_shapes().items() if not k.startswith("policy.")}


def init_parameters(seed=0, gain=1.0):
    """Random parameters of the reference's shapes: U(-1/sqrt(fan_in), 1/sqrt(fan_in)) like torch's defaults for
    Conv2d / Linear, U(-1/sqrt(hidden), 1/sqrt(hidden)) for GRU.  (There is no network to fetch checkpoints.)"""
    rng = np.random.default_rng(seed)
    out = {}
    for name, shape in parameter_shapes().items():
        if ".gru" in name:
            bound = 1.0 / np.sqrt(HIDDEN)
        elif name.endswith(".bias"):
            w = parameter_shapes()[name[:-5] + ".weight"]
            bound = 1.0 / np.sqrt(np.prod(w[1:]))
        else:
            bound = 1.0 / np.sqrt(np.prod(shape[1:]))
        out[name] = (rng.uniform(-bound, bound, size=shape) * gain).astype(np.float32)
    return out


def load_checkpoint(path):
    """Parameters of a trained bot from the reference's checkpoint file: `torch::save(model, dir + "/model.pt")`
    (bots/bot-0.5/Agent.hpp:77-110,124,159-161) writes a TorchScript module archive whose named_parameters() carry the
    names AgentModel registered (Modules.hpp:37,62,87-91,147-152) — the names `parameter_shapes()` lists.  Also reads a
    plain state_dict saved from Python.  Returns {name: float32 numpy array}, every name and shape checked; nothing
    is filled in silently.  A RewardModel archive (bots/bot-1/RewardNet.hpp:239: no policy.* parameter in it) is held to
    `reward_parameter_shapes()` instead and goes to `RewardBatch`."""
    import torch
    named = None
    try:
        m = torch.jit.load(path, map_location="cpu")
        named = {k: v for k, v in m.named_parameters()}
    except Exception:  # noqa: BLE001  (not a TorchScript archive)
        obj = torch.load(path, map_location="cpu", weights_only=True)
        if hasattr(obj, "state_dict"):
            obj = obj.state_dict()
        if not isinstance(obj, dict):
            raise ValueError("%s holds neither a TorchScript module nor a state_dict" % path)
        named = obj
    out = {}
    shapes = parameter_shapes() if any(k.startswith("policy.") for k in named) else reward_parameter_shapes()
    for name, shape in shapes.items():
        if name not in named:
            raise ValueError("checkpoint %s lacks parameter %s" % (path, name))
        a = named[name].detach().to(torch.float32).contiguous().numpy()
        if a.shape != tuple(shape):
            raise ValueError("checkpoint parameter %s has shape %s, expected %s" % (name, a.shape, shape))
        out[name] = a.copy()
    extra = sorted(k for k in named if k not in out and not k.endswith("num_batches_tracked"))
    if extra:
        raise ValueError("checkpoint %s holds parameters this network does not have: %s" % (path, extra[:5]))
    return out


def _fill_weights(ptr, shapes):
    """A Weights whose fields are ptr(name) for the parameter names of `shapes` (a reward model's table has no policy.*
    names: those fields stay NULL)."""
    w = Weights()
    w.abi_version = POLICY_ABI_VERSION
    for i in range(CONVS):
        w.conv_w[i] = ptr("backbone.cnn.conv%d.weight" % i)
    for g in range(2):
        w.gru_w_ih[g] = ptr("backbone.gru%d.weight_ih_l0" % g)
        w.gru_w_hh[g] = ptr("backbone.gru%d.weight_hh_l0" % g)
        w.gru_b_ih[g] = ptr("backbone.gru%d.bias_ih_l0" % g)
        w.gru_b_hh[g] = ptr("backbone.gru%d.bias_hh_l0" % g)
    w.comb_w, w.comb_b = ptr("backbone.combined_processor.0.weight"), ptr("backbone.combined_processor.0.bias")
    for i in range(RES_LAYERS):
        w.value_res_w[i], w.value_res_b[i] = ptr("value.0.lin%d.weight" % i), ptr("value.0.lin%d.bias" % i)
    w.value_w, w.value_b = ptr("value.1.weight"), ptr("value.1.bias")
    if "policy.1.weight" in shapes:
        for i in range(RES_LAYERS):
            w.policy_res_w[i], w.policy_res_b[i] = ptr("policy.0.lin%d.weight" % i), ptr("policy.0.lin%d.bias" % i)
        w.policy_w, w.policy_b = ptr("policy.1.weight"), ptr("policy.1.bias")
    return w


def device_weights(tensors, shapes):
    """The `Weights` of sf_policy_load_weights for parameters that live on the device: `tensors` is a dict of torch tensors
    keyed by the reference's parameter names, `shapes` the kind's table (`parameter_shapes()` / `reward_parameter_shapes()`;
    names outside it are ignored).  Every tensor named there must be a contiguous float32 tensor of that shape on one and
    the same GPU — views into one flat tensor are fine, any 4-byte offset will do — or this raises ValueError naming the
    parameter; nothing is converted or copied.  Returns (weights, keep): `keep` holds the tensors the pointers point into
    and must outlive every load issued with `weights`, until the stream has passed it."""
    import torch
    keep, device = {}, None
    for name, shape in shapes.items():
        if name not in tensors:
            raise ValueError("missing parameter %s" % name)
        t = tensors[name]
        if not isinstance(t, torch.Tensor):
            raise ValueError("parameter %s is a %s, not a torch tensor" % (name, type(t).__name__))
        if tuple(t.shape) != tuple(shape):
            raise ValueError("parameter %s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
        if t.dtype != torch.float32:
            raise ValueError("parameter %s has dtype %s, expected torch.float32" % (name, t.dtype))
        if not t.is_contiguous():
            raise ValueError("parameter %s is not contiguous" % name)
        if t.device.type != "cuda":
            raise ValueError("parameter %s is on %s, not on a GPU" % (name, t.device))
        if device is None:
            device = t.device
        elif t.device != device:
            raise ValueError("parameter %s is on %s, the parameters before it on %s" % (name, t.device, device))
        keep[name] = t
    return _fill_weights(lambda n: C.cast(C.c_void_p(keep[n].data_ptr()), _FP), shapes), keep


class PredictIO(C.Structure):
    """sf_policy_predict_io (include/strikeforce_policy.h)."""
    _fields_ = [("d_keys", C.c_void_p), ("d_vals", C.c_void_p), ("d_counts", C.c_void_p), ("d_pov", C.c_void_p), ("cap", C.c_int32),
                ("d_dense", C.c_void_p), ("d_reset_mask", C.c_void_p), ("d_reset_words", C.c_void_p),
                ("reset_stride", C.c_int32), ("reset_group", C.c_int32), ("action_string", C.c_char_p), ("seed", C.c_uint64),
                ("greedy", C.c_int32), ("d_probs", C.c_void_p), ("d_value", C.c_void_p), ("d_cmd", C.c_void_p), ("d_action", C.c_void_p)]


class RewardIO(C.Structure):
    """sf_reward_io (include/strikeforce_policy.h)."""
    _fields_ = [("d_keys", C.c_void_p), ("d_vals", C.c_void_p), ("d_counts", C.c_void_p), ("d_pov", C.c_void_p), ("cap", C.c_int32),
                ("d_dense", C.c_void_p), ("d_reset_mask", C.c_void_p), ("d_reset_words", C.c_void_p),
                ("reset_stride", C.c_int32), ("reset_group", C.c_int32), ("d_action", C.c_void_p), ("d_disc", C.c_void_p),
                ("d_reward", C.c_void_p)]


def _bind(L):
    if getattr(L, "_sf_policy_bound", False):
        return
    vp = C.c_void_p
    L.sf_reward_create.argtypes = [C.POINTER(Weights), C.c_int32, C.c_int32, C.POINTER(vp)]
    L.sf_reward_forward.argtypes = [vp, vp, vp, C.c_int32, vp, vp]
    L.sf_reward_sparse.argtypes = [vp, C.POINTER(RewardIO), C.c_int32]
    L.sf_policy_predict_sparse.argtypes = [vp, C.POINTER(PredictIO), C.c_int32]
    L.sf_policy_create.argtypes = [C.POINTER(Weights), C.c_int32, C.c_int32, C.POINTER(vp)]
    L.sf_policy_destroy.argtypes = [vp]
    L.sf_policy_destroy.restype = None
    L.sf_policy_reset_memory.argtypes = [vp, vp]
    L.sf_policy_reset_memory_n.argtypes = [vp, vp, C.c_int32]
    L.sf_policy_reset_memory_n.restype = C.c_int
    L.sf_policy_forward.argtypes = [vp, vp, C.c_int32, vp, vp]
    L.sf_policy_forward_sparse.argtypes = [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, vp, vp]
    L.sf_policy_forward_sparse_or_dense.argtypes = [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, vp, vp, vp]
    L.sf_policy_kernel_time_by_kernel.argtypes = [vp, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.sf_policy_sparse_overflows.argtypes = [vp, C.POINTER(C.c_int32)]
    L.sf_policy_act.argtypes = [vp, vp, C.c_int32, C.c_char_p, C.c_uint64, C.c_int32, vp, vp]
    if hasattr(L, "sf_policy_act_masked"):  # (an older build loaded through SF_LIBRARY_PATH lacks it)
        L.sf_policy_act_masked.argtypes = [vp, vp, C.c_int32, C.c_char_p, C.c_uint64, C.c_int32, vp, vp, vp, vp]
    L.sf_policy_get_memory.argtypes = [vp, C.c_int32, _FP, _FP]
    L.sf_policy_set_memory.argtypes = [vp, C.c_int32, _FP, _FP]
    L.sf_policy_set_stream.argtypes = [vp, vp]
    L.sf_policy_synchronize.argtypes = [vp]
    L.sf_policy_gemm.argtypes = [vp, vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.sf_policy_gemm_split.argtypes = L.sf_policy_gemm.argtypes
    L.sf_policy_features.argtypes = [vp, vp, C.c_int32, vp]
    L.sf_policy_kernel_time.argtypes = [vp, C.c_int32, _FP, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.sf_policy_kernel_time_ex.argtypes = L.sf_policy_kernel_time.argtypes
    if hasattr(L, "sf_policy_update_actions"):  # (the rollout buffer's replay entry: strikeforce_amd/rollout.py)
        L.sf_policy_update_actions.argtypes = [vp, vp, C.c_int32]
    if hasattr(L, "sf_policy_load_weights"):  # (parameters in, from the device: _NetBatch.load_weights)
        L.sf_policy_load_weights.argtypes = [vp, C.POINTER(Weights)]
        L.sf_policy_weights_digest.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
    if hasattr(L, "sf_policy_memory_rows"):  # (an older build loaded through SF_LIBRARY_PATH lacks it)
        L.sf_policy_memory_rows.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32]
    for n in EXPORTS + REWARD_EXPORTS:
        if n != "sf_policy_destroy" and hasattr(L, n):
            getattr(L, n).restype = C.c_int
    L._sf_policy_bound = True


# every symbol include/strikeforce_policy.h declares
EXPORTS = ["sf_policy_create", "sf_policy_destroy", "sf_policy_reset_memory", "sf_policy_reset_memory_n", "sf_policy_forward", "sf_policy_forward_sparse",
           "sf_policy_forward_sparse_or_dense",
           "sf_policy_sparse_overflows", "sf_policy_act", "sf_policy_act_masked", "sf_policy_predict_sparse",
           "sf_policy_get_memory", "sf_policy_set_memory", "sf_policy_set_stream", "sf_policy_synchronize",
           "sf_policy_kernel_time", "sf_policy_kernel_time_ex", "sf_policy_kernel_time_by_kernel", "sf_policy_gemm", "sf_policy_gemm_split", "sf_policy_features", "sf_policy_abi_version",
           "sf_policy_update_actions", "sf_policy_load_weights", "sf_policy_weights_digest", "sf_policy_memory_rows"]


# the reward network's entries (sf_reward_*: the same header)
REWARD_EXPORTS = ["sf_reward_create", "sf_reward_forward", "sf_reward_sparse"]


class _NetBatch:
    """What a policy and a reward model share: one sf_policy handle, per-agent memory, stream, timers."""

    def __init__(self, params, max_agents, device, shapes, create):
        self.L = env.load_library()
        _bind(self.L)
        self.max_agents, self.device, self.shapes = int(max_agents), int(device), shapes
        keep = {}
        for name, shape in shapes.items():
            if name not in params:
                raise ValueError("missing parameter %s" % name)
            a = np.ascontiguousarray(params[name], dtype=np.float32)
            if a.shape != tuple(shape):
                raise ValueError("parameter %s has shape %s, expected %s" % (name, a.shape, shape))
            keep[name] = a
        w = _fill_weights(lambda n: keep[n].ctypes.data_as(_FP), shapes)
        self.h = C.c_void_p()
        rc = getattr(self.L, create)(C.byref(w), self.max_agents, int(device), C.byref(self.h))
        if rc != 0:
            self.h = None
            raise env.StrikeForceError("%s failed (%d): %s" % (create, rc, self.L.sf_last_error().decode()))

    def _ck(self, rc, what):
        if rc != 0:
            raise env.StrikeForceError("%s failed (%d): %s" % (what, rc, self.L.sf_last_error().decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.sf_policy_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream):
        self._ck(self.L.sf_policy_set_stream(self.h, C.c_void_p(hip_stream)), "sf_policy_set_stream")

    def synchronize(self):
        self._ck(self.L.sf_policy_synchronize(self.h), "sf_policy_synchronize")

    def reset_memory(self, d_mask_ptr=None, agents=None):
        """d_mask: device bytes, one per agent; with `agents` only agents [0, agents) are looked at (a mask of that
        many bytes), otherwise the mask must hold max_agents bytes."""
        m = C.c_void_p(d_mask_ptr) if d_mask_ptr else None
        if agents is None:
            self._ck(self.L.sf_policy_reset_memory(self.h, m), "sf_policy_reset_memory")
        else:
            self._ck(self.L.sf_policy_reset_memory_n(self.h, m, int(agents)), "sf_policy_reset_memory_n")

    def update_actions(self, d_action_ptr, agents):
        """AgentModel::update_actions(one_hot(action)) for agents [0, agents) (device int32 per agent; outside [0, 9): 0):
        what a replay of a stored rollout calls behind every forward (RolloutBatch)."""
        self._ck(self.L.sf_policy_update_actions(self.h, C.c_void_p(d_action_ptr), int(agents)), "sf_policy_update_actions")

    def load_weights(self, tensors):
        """optimizer->step() seen from the device (sf_policy_load_weights): the parameters every later forward on this
        object's stream uses are `tensors` — torch tensors on this object's GPU, checked by `device_weights` against the
        kind's shape table.  Stream-ordered, no synchronisation; per-agent memory, stream and timers stay as they are.
        The tensors are read when the stream gets there: they are kept alive here until the next load, and work that
        changes them has to be ordered behind this call (issued later on the same stream, or after a synchronise)."""
        w, keep = device_weights(tensors, self.shapes)
        for name, t in keep.items():
            if t.device.index != self.device:
                raise ValueError("parameter %s is on %s, this object on device %d" % (name, t.device, self.device))
        self._ck(self.L.sf_policy_load_weights(self.h, C.byref(w)), "sf_policy_load_weights")
        self._loaded = keep

    def weights_digest(self):
        """One 64-bit digest per device image the object derives from its parameters, in the header's order (test hook;
        synchronises)."""
        out, n = (C.c_uint64 * 64)(), C.c_int32(64)
        self._ck(self.L.sf_policy_weights_digest(self.h, out, C.byref(n)), "sf_policy_weights_digest")
        return [int(out[i]) for i in range(n.value)]

    def sparse_overflows(self):
        """Agents evaluated on an empty observation since the last call because their list did not fit (synchronises)."""
        n = C.c_int32()
        self._ck(self.L.sf_policy_sparse_overflows(self.h, C.byref(n)), "sf_policy_sparse_overflows")
        return n.value

    def get_memory(self, agent):
        h = np.zeros((2, HIDDEN), dtype=np.float32)
        a = np.zeros(ACTIONS, dtype=np.float32)
        self._ck(self.L.sf_policy_get_memory(self.h, int(agent), h.ctypes.data_as(_FP), a.ctypes.data_as(_FP)),
                 "sf_policy_get_memory")
        return h, a

    def set_memory(self, agent, h, action_input):
        h = np.ascontiguousarray(h, dtype=np.float32).reshape(2, HIDDEN)
        a = np.ascontiguousarray(action_input, dtype=np.float32).reshape(ACTIONS)
        self._ck(self.L.sf_policy_set_memory(self.h, int(agent), h.ctypes.data_as(_FP), a.ctypes.data_as(_FP)),
                 "sf_policy_set_memory")

    def memory_rows(self, to_rows, d_h_ptr, d_action_ptr, d_row_of_agent_ptr, rows, agents=None):
        """The memory of agents [0, agents) to (to_rows=True) or from rows of the caller's device buffers, one stream-ordered
        launch (sf_policy_memory_rows): d_h float32 [rows][2][160], d_action float32 [rows][9], d_row_of_agent int32
        [agents] with -1 (or anything outside [0, rows)) for an agent that takes no part.  Many agents may read one row:
        the network memory of a forked arena (env.Snapshot.load)."""
        if not hasattr(self.L, "sf_policy_memory_rows"):
            raise env.StrikeForceError("this build of libstrikeforce_amd.so has no sf_policy_memory_rows")
        n = self.max_agents if agents is None else int(agents)
        self._ck(self.L.sf_policy_memory_rows(self.h, 1 if to_rows else 0, C.c_void_p(d_h_ptr), C.c_void_p(d_action_ptr),
                                              C.c_void_p(d_row_of_agent_ptr), int(rows), n), "sf_policy_memory_rows")

    def kernel_time_by_pipe(self, enable=True):
        """[(ms, flop, launches) of the f32-MFMA launches, (...) of the bf16-split launches] since the last call."""
        ms, fl, n = (C.c_float * 2)(), (C.c_double * 2)(), (C.c_int32 * 2)()
        self._ck(self.L.sf_policy_kernel_time_ex(self.h, 1 if enable else 0, ms, fl, n), "sf_policy_kernel_time_ex")
        return [(ms[k], fl[k], n[k]) for k in range(2)]

    def kernel_time_by_kernel(self, enable=True):
        """[(ms, algorithmic flop, launches)] for k_gemm (f32 MFMA), k_gemm_b3 (bf16 split), conv0 on the non-zeros, k_tail."""
        ms, fl, n = (C.c_float * 4)(), (C.c_double * 4)(), (C.c_int32 * 4)()
        self._ck(self.L.sf_policy_kernel_time_by_kernel(self.h, 1 if enable else 0, ms, fl, n), "sf_policy_kernel_time_by_kernel")
        return [(float(ms[k]), float(fl[k]), int(n[k])) for k in range(4)]

    def kernel_time(self, enable=True):
        """(ms, flop, launches) of the MFMA GEMM launches since the last call; arms / disarms the timers."""
        ms, fl, n = C.c_float(), C.c_double(), C.c_int32()
        self._ck(self.L.sf_policy_kernel_time(self.h, 1 if enable else 0, C.byref(ms), C.byref(fl), C.byref(n)),
                 "sf_policy_kernel_time")
        return ms.value, fl.value, n.value


class PolicyBatch(_NetBatch):
    """`max_agents` independent copies of the reference's AgentModel state over one shared parameter set."""

    def __init__(self, params, max_agents, device=0):
        super().__init__(params, max_agents, device, parameter_shapes(), "sf_policy_create")

    def forward(self, d_obs_ptr, agents, d_probs_ptr, d_value_ptr):
        self._ck(self.L.sf_policy_forward(self.h, C.c_void_p(d_obs_ptr), int(agents), C.c_void_p(d_probs_ptr),
                                          C.c_void_p(d_value_ptr)), "sf_policy_forward")

    def forward_sparse(self, d_keys_ptr, d_vals_ptr, d_counts_ptr, d_pov_ptr, cap, agents, d_probs_ptr, d_value_ptr,
                       d_dense_ptr=None):
        """forward() on ArenaBatch.observe_sparse_device's lists: same results, no dense observation in between.
        d_dense_ptr: the buffer ArenaBatch.observe_overflow_device filled for the agents whose list did not fit; they are
        then evaluated from it (never on a blank window).  Without it such agents are evaluated as empty and counted
        (sparse_overflows)."""
        if d_dense_ptr is not None:
            self._ck(self.L.sf_policy_forward_sparse_or_dense(
                self.h, C.c_void_p(d_keys_ptr), C.c_void_p(d_vals_ptr), C.c_void_p(d_counts_ptr), C.c_void_p(d_pov_ptr),
                int(cap), int(agents), C.c_void_p(d_dense_ptr), C.c_void_p(d_probs_ptr), C.c_void_p(d_value_ptr)),
                "sf_policy_forward_sparse_or_dense")
            return
        self._ck(self.L.sf_policy_forward_sparse(self.h, C.c_void_p(d_keys_ptr), C.c_void_p(d_vals_ptr), C.c_void_p(d_counts_ptr),
                                                 C.c_void_p(d_pov_ptr), int(cap), int(agents), C.c_void_p(d_probs_ptr),
                                                 C.c_void_p(d_value_ptr)), "sf_policy_forward_sparse")

    def predict_sparse(self, d_keys_ptr, d_vals_ptr, d_counts_ptr, d_pov_ptr, cap, agents, d_probs_ptr, d_value_ptr, d_cmd_ptr,
                       seed=0, greedy=False, d_action_ptr=None, action_string=ACTION_STRING, d_dense_ptr=None, d_reset_mask_ptr=None,
                       reset_words=None):
        """reset_memory(mask) + forward_sparse + act as the forward's two launches (Agent::predict + update are one call in
        the reference too): same results bit for bit.  reset_words: ArenaBatch.done_view_device()'s triple, read in place."""
        io = PredictIO()
        io.d_keys, io.d_vals, io.d_counts, io.d_pov, io.cap = d_keys_ptr, d_vals_ptr, d_counts_ptr, d_pov_ptr, int(cap)
        io.d_dense, io.d_reset_mask = d_dense_ptr, d_reset_mask_ptr
        if reset_words is not None:
            io.d_reset_words, io.reset_stride, io.reset_group = reset_words
        io.action_string, io.seed, io.greedy = action_string.encode(), seed, 1 if greedy else 0
        io.d_probs, io.d_value, io.d_cmd, io.d_action = d_probs_ptr, d_value_ptr, d_cmd_ptr, d_action_ptr
        self._ck(self.L.sf_policy_predict_sparse(self.h, C.byref(io), int(agents)), "sf_policy_predict_sparse")

    def act(self, d_probs_ptr, agents, d_cmd_ptr, seed=0, greedy=False, d_action_ptr=None,
            action_string=ACTION_STRING):
        self._ck(self.L.sf_policy_act(self.h, C.c_void_p(d_probs_ptr), int(agents), action_string.encode(),
                                      C.c_uint64(seed), 1 if greedy else 0, C.c_void_p(d_cmd_ptr),
                                      C.c_void_p(d_action_ptr) if d_action_ptr else None), "sf_policy_act")

    def act_masked(self, d_probs_ptr, agents, d_action_mask_ptr, d_cmd_ptr, seed=0, greedy=False, d_action_ptr=None,
                   d_probs_out_ptr=None, action_string=ACTION_STRING):
        """act() under an action mask (sf_policy_act_masked): d_action_mask_ptr is ArenaBatch.action_mask(action_string)'s
        second tensor, uint32 per agent, bit j = action_string[j] would do something.  A masked action is never drawn; a
        word of 0 (a dead seat) yields action 0.  d_probs_out_ptr: float32 [agents][9], the distribution the action was drawn
        from (masked entries exactly 0: their log is -inf) — what the rollout buffer takes as d_probs.  With every bit set
        this is act() bit for bit."""
        if not hasattr(self.L, "sf_policy_act_masked"):
            raise env.StrikeForceError("this build of libstrikeforce_amd.so has no sf_policy_act_masked")
        opt = lambda x: C.c_void_p(x) if x else None
        self._ck(self.L.sf_policy_act_masked(self.h, C.c_void_p(d_probs_ptr), int(agents), action_string.encode(),
                                             C.c_uint64(seed), 1 if greedy else 0, C.c_void_p(d_action_mask_ptr),
                                             C.c_void_p(d_cmd_ptr), opt(d_action_ptr), opt(d_probs_out_ptr)),
                 "sf_policy_act_masked")

    def gemm(self, d_a_ptr, lda, d_w_ptr, d_bias_ptr, d_c_ptr, ldc, m, n, k):
        """The MFMA matrix kernel on its own: C = A W^T + bias on device buffers."""
        self._ck(self.L.sf_policy_gemm(self.h, C.c_void_p(d_a_ptr), lda, C.c_void_p(d_w_ptr),
                                       C.c_void_p(d_bias_ptr) if d_bias_ptr else None, C.c_void_p(d_c_ptr), ldc, m, n, k),
                 "sf_policy_gemm")

    def features(self, d_obs_ptr, agents, d_feat_ptr):
        """GameCNN::forward alone: [agents][160] features behind the four convolutions (test hook)."""
        self._ck(self.L.sf_policy_features(self.h, C.c_void_p(d_obs_ptr), agents, C.c_void_p(d_feat_ptr)), "sf_policy_features")

    def gemm_split(self, d_a_ptr, lda, d_w_ptr, d_bias_ptr, d_c_ptr, ldc, m, n, k):
        """The same product through the bf16-split kernel of conv1 / conv2 (six bf16 MFMAs per block, f32-level error)."""
        self._ck(self.L.sf_policy_gemm_split(self.h, C.c_void_p(d_a_ptr), lda, C.c_void_p(d_w_ptr),
                                             C.c_void_p(d_bias_ptr) if d_bias_ptr else None, C.c_void_p(d_c_ptr), ldc, m, n, k),
                 "sf_policy_gemm_split")


class RewardBatch(_NetBatch):
    """`max_agents` independent copies of bot-1's RewardModel state (bots/bot-1/RewardNet.hpp:138-167, one per Agent:
    Agent.hpp:95) over one shared parameter set (`reward_parameter_shapes()`; policy.* entries of `params` are ignored).
    D = the discriminator's output, reward = log D: what RewardNet::get_reward returns (RewardNet.hpp:244-259)."""

    def __init__(self, params, max_agents, device=0):
        super().__init__(params, max_agents, device, reward_parameter_shapes(), "sf_reward_create")

    def forward(self, d_obs_ptr, d_action_ptr, agents, d_disc_ptr=None, d_reward_ptr=None):
        """RewardModel::forward(one_hot(action), obs) on the dense observation: D and / or log D per agent; the one-hot
        stays in the agent's memory (update_actions)."""
        self._ck(self.L.sf_reward_forward(self.h, C.c_void_p(d_obs_ptr), C.c_void_p(d_action_ptr), int(agents), C.c_void_p(d_disc_ptr),
                                          C.c_void_p(d_reward_ptr)), "sf_reward_forward")

    def reward_sparse(self, d_keys_ptr, d_vals_ptr, d_counts_ptr, d_pov_ptr, cap, agents, d_action_ptr, d_disc_ptr=None, d_reward_ptr=None,
                      d_dense_ptr=None, d_reset_mask_ptr=None, reset_words=None):
        """The same on ArenaBatch.observe_sparse_device's lists with the restart flags folded in (PolicyBatch.predict_sparse's
        arguments): issue it right behind predict_sparse on the same stream with that call's d_action."""
        io = RewardIO()
        io.d_keys, io.d_vals, io.d_counts, io.d_pov, io.cap = d_keys_ptr, d_vals_ptr, d_counts_ptr, d_pov_ptr, int(cap)
        io.d_dense, io.d_reset_mask = d_dense_ptr, d_reset_mask_ptr
        if reset_words is not None:
            io.d_reset_words, io.reset_stride, io.reset_group = reset_words
        io.d_action, io.d_disc, io.d_reward = d_action_ptr, d_disc_ptr, d_reward_ptr
        self._ck(self.L.sf_reward_sparse(self.h, C.byref(io), int(agents)), "sf_reward_sparse")


# ---- several networks in one match (include/strikeforce_policy.h, sf_route_*) -------------------------------------------------
ROUTE_MAX_NETS = 8
ROUTE_EXPORTS = ["sf_route_create", "sf_route_destroy", "sf_route_set_stream", "sf_route_synchronize", "sf_route_count",
                 "sf_route_agents_device", "sf_route_gather", "sf_route_scatter"]
ROUTE_ROW_FIELDS = ("cmd", "action", "probs", "value", "reward", "disc")


class RouteSrc(C.Structure):
    """sf_route_src."""
    _fields_ = [("d_keys", C.c_void_p), ("d_vals", C.c_void_p), ("d_counts", C.c_void_p), ("d_pov", C.c_void_p), ("cap", C.c_int32),
                ("d_dense", C.c_void_p), ("d_reset_mask", C.c_void_p), ("d_reset_words", C.c_void_p),
                ("reset_stride", C.c_int32), ("reset_group", C.c_int32)]


class RouteDst(C.Structure):
    """sf_route_dst."""
    _fields_ = [("d_keys", C.c_void_p), ("d_vals", C.c_void_p), ("d_counts", C.c_void_p), ("d_pov", C.c_void_p), ("cap", C.c_int32),
                ("d_dense", C.c_void_p), ("d_reset_mask", C.c_void_p)]


class RouteRows(C.Structure):
    """sf_route_rows."""
    _fields_ = [("d_cmd", C.c_void_p), ("d_action", C.c_void_p), ("d_probs", C.c_void_p), ("d_value", C.c_void_p),
                ("d_reward", C.c_void_p), ("d_disc", C.c_void_p)]


def _bind_route(L):
    if getattr(L, "_sf_route_bound", False):
        return
    if not hasattr(L, "sf_route_create"):  # (an older build loaded through SF_LIBRARY_PATH lacks it)
        raise env.StrikeForceError("libstrikeforce_amd.so has no sf_route_* entry points: rebuild it (python -m strikeforce_amd.build)")
    vp, pp = C.c_void_p, C.POINTER(C.c_void_p)
    L.sf_route_create.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32, pp]
    L.sf_route_destroy.argtypes = [vp]
    L.sf_route_destroy.restype = None
    L.sf_route_set_stream.argtypes = [vp, vp]
    L.sf_route_synchronize.argtypes = [vp]
    L.sf_route_count.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32)]
    L.sf_route_agents_device.argtypes = [vp, C.c_int32, pp]
    L.sf_route_gather.argtypes = [vp, C.POINTER(RouteSrc), C.POINTER(RouteDst)]
    L.sf_route_scatter.argtypes = [vp, C.POINTER(RouteRows), C.POINTER(RouteRows)]
    for n in ROUTE_EXPORTS:
        if n != "sf_route_destroy":
            getattr(L, n).restype = C.c_int
    L._sf_route_bound = True


def route_slots(assign, nets):
    """The slot rule of sf_route_create on the host: (slot per agent, -1 for nobody's; per network the agents by slot)."""
    assign = np.asarray(assign, dtype=np.int64).reshape(-1)
    slot = np.full(len(assign), -1, dtype=np.int32)
    agents_of = []
    for k in range(int(nets)):
        mine = np.flatnonzero(assign == k)
        slot[mine] = np.arange(len(mine), dtype=np.int32)
        agents_of.append(mine.astype(np.int32))
    return slot, agents_of


class Router:
    """Agents of one environment batch routed to `nets` networks (`PolicyBatch` / `RewardBatch` / `RolloutBatch` objects of
    count(k) agents each): assign[a] in [0, nets), or -1 for an agent no network plays.  Every commanded human of the
    reference owns its network (bots/bot-0.5/Custom.hpp:161-165, bots/bot-1/Agent.hpp:84-101); this is that, for a batch.

    Allocates, per network, the rows gather() fills — keys, vals [n][cap], counts [n], pov [n][160], reset [n] uint8 and,
    with dense=True, dense [n][32][31][31] — and the compact rows the network answers into: cmd [n] uint8, action [n] int32,
    probs [n][9], value, reward, disc [n] (attributes of `net[k]`).  One tick:

        router.gather((keys, vals, counts, pov, cap), d_dense_ptr=..., reset_words=sim.done_view_device())
        for k in range(nets): nets_[k].predict_sparse(**router.inputs(k), **router.outputs(k), seed=seed[k])
        router.scatter({"cmd": d_cmd})

    The draw of slot s is keyed by (seed, s, i): give every network its own seed."""

    def __init__(self, assign, nets, cap=2048, dense=False, device=0):
        import torch
        import types
        self.L = env.load_library()
        _bind_route(self.L)
        self.assign = np.ascontiguousarray(assign, dtype=np.int32).reshape(-1)
        self.agents, self.nets, self.cap, self.device = len(self.assign), int(nets), int(cap), int(device)
        self.h = None
        h = C.c_void_p()
        rc = self.L.sf_route_create(self.assign.ctypes.data_as(C.POINTER(C.c_int32)), self.agents, self.nets, self.device, C.byref(h))
        if rc != 0:
            raise env.StrikeForceError("sf_route_create failed (%d): %s" % (rc, self.L.sf_last_error().decode()))
        self.h = h
        dev = torch.device("cuda", self.device)
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        self.net = []
        for k in range(self.nets):
            n = self.count(k)
            new = lambda shape, dtype: torch.zeros((n,) + shape, dtype=dtype, device=dev)
            self.net.append(types.SimpleNamespace(
                keys=new((self.cap,), i32), vals=new((self.cap,), f32), counts=new((), i32), pov=new((HIDDEN,), f32),
                dense=new((OBS_CHANNELS, OBS_WINDOW, OBS_WINDOW), f32) if dense else None, reset=new((), u8),
                cmd=new((), u8), action=new((), i32), probs=new((ACTIONS,), f32), value=new((), f32), reward=new((), f32),
                disc=new((), f32)))
        self._torch, self._dev = torch, dev
        ptr = lambda t: (t.data_ptr() or None) if t is not None else None
        self._dst = (RouteDst * self.nets)(*[RouteDst(ptr(g.keys), ptr(g.vals), ptr(g.counts), ptr(g.pov), self.cap, ptr(g.dense),
                                                      ptr(g.reset)) for g in self.net])
        self._rows = (RouteRows * self.nets)(*[RouteRows(*[ptr(getattr(g, f)) for f in ROUTE_ROW_FIELDS]) for g in self.net])

    def _ck(self, rc, what):
        if rc != 0:
            raise env.StrikeForceError("%s failed (%d): %s" % (what, rc, self.L.sf_last_error().decode()))

    def close(self):
        if getattr(self, "h", None):
            self.L.sf_route_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream):
        self._ck(self.L.sf_route_set_stream(self.h, C.c_void_p(hip_stream)), "sf_route_set_stream")

    def synchronize(self):
        self._ck(self.L.sf_route_synchronize(self.h), "sf_route_synchronize")

    def count(self, k):
        n = C.c_int32()
        self._ck(self.L.sf_route_count(self.h, int(k), C.byref(n)), "sf_route_count")
        return n.value

    def agents_of(self, k):
        """Network k's agents by slot, as a device tensor view (int32 [count(k)], the library's memory: read it only)."""
        p = C.c_void_p()
        self._ck(self.L.sf_route_agents_device(self.h, int(k), C.byref(p)), "sf_route_agents_device")
        n = self.count(k)
        if n == 0:
            return self._torch.zeros(0, dtype=self._torch.int32, device=self._dev)
        iface = {"shape": (n,), "typestr": "<i4", "data": (p.value, False), "version": 2}
        return self._torch.as_tensor(type("AgentsView", (), {"__cuda_array_interface__": iface})(), device=self._dev)

    def gather(self, lists, d_dense_ptr=None, d_reset_mask_ptr=None, reset_words=None):
        """lists: (d_keys_ptr, d_vals_ptr, d_counts_ptr, d_pov_ptr, cap) of ArenaBatch.observe_sparse_device, environment
        order; cap must be this router's.  The other arguments as PolicyBatch.predict_sparse takes them.  One launch."""
        s = RouteSrc()
        s.d_keys, s.d_vals, s.d_counts, s.d_pov, s.cap = lists[0], lists[1], lists[2], lists[3], int(lists[4])
        s.d_dense, s.d_reset_mask = d_dense_ptr, d_reset_mask_ptr
        if reset_words is not None:
            s.d_reset_words, s.reset_stride, s.reset_group = reset_words
        self._ck(self.L.sf_route_gather(self.h, C.byref(s), self._dst), "sf_route_gather")

    def inputs(self, k, record=False):
        """Keyword arguments for network k: what PolicyBatch.predict_sparse and RewardBatch.reward_sparse take — or, with
        record=True, RolloutBatch.record (which takes no dense rows)."""
        g = self.net[k]
        kw = dict(d_keys_ptr=g.keys.data_ptr(), d_vals_ptr=g.vals.data_ptr(), d_counts_ptr=g.counts.data_ptr(),
                  d_pov_ptr=g.pov.data_ptr(), cap=self.cap, agents=self.count(k), d_reset_mask_ptr=g.reset.data_ptr())
        if g.dense is not None and not record:
            kw["d_dense_ptr"] = g.dense.data_ptr()
        return kw

    def outputs(self, k):
        """Keyword arguments for PolicyBatch.predict_sparse's outputs of network k: its compact rows."""
        g = self.net[k]
        return dict(d_probs_ptr=g.probs.data_ptr(), d_value_ptr=g.value.data_ptr(), d_cmd_ptr=g.cmd.data_ptr(),
                    d_action_ptr=g.action.data_ptr())

    def scatter(self, env_rows):
        """env_rows: {"cmd" | "action" | "probs" | "value" | "reward" | "disc": environment-order tensor or device address}; the
        fields it names are copied from every network's compact rows to row a.  Rows of unassigned agents stay.  One launch."""
        unknown = sorted(set(env_rows) - set(ROUTE_ROW_FIELDS))
        if unknown:
            raise ValueError("scatter: no such rows: %s" % unknown)
        at = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        e = RouteRows(*[at(env_rows.get(f)) for f in ROUTE_ROW_FIELDS])
        self._ck(self.L.sf_route_scatter(self.h, self._rows, C.byref(e)), "sf_route_scatter")
