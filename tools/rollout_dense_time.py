"""What sf_rollout_dense costs against the fill it cannot avoid ("Stored lists to dense rows"), one process:

    python tools/rollout_dense_time.py [out.json]

4096 rows: slot 0 of a rollout of BASELINE configs[1], 4096 agents, list_cap = 512, recorded after 20 ticks of play.  For
NCHW / float32 and for NHWC / bfloat16: two series of the call and two of its yardstick, hipMemsetAsync of the same
destination bytes on the same stream (not code of this library), the four alternating and the order rotating by one every
round; device events around each call; medians of 21 after 10 warm-up rounds.  The yardstick's spread is the difference of
its two medians.  The call is given the yardstick's time, plus that spread, plus the share of bytes it moves beyond the
fill: the lists it reads (8 bytes per entry, the count and the row's cell) and the values it stores a second time (one
element per entry), computed here from the stored counts.  As information only: the same rows by torch (zero_, index
arithmetic in int64, scatter_ into rows one element longer, where the entries behind the count land).
Prints one JSON object."""
import ctypes as C
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from strikeforce_amd import config, env, policy, rollout

REPS, WARM, CAP, ROWS, T, LIST_CAP, PLAY = 21, 10, 2048, 4096, 2, 512, 20
out = {"reps": REPS, "warm": WARM, "unit": "ms, device events", "rows": ROWS, "list_cap": LIST_CAP}

lib = sorted(glob.glob(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so*")))
H = C.CDLL(lib[0] if lib else "libamdhip64.so")
H.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]


def span(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def med(pairs):
    torch.cuda.synchronize()
    t = np.array([a.elapsed_time(b) for a, b in pairs])
    return {"median": float(np.median(t)), "min": float(t.min()), "max": float(t.max())}


def alternate(calls):
    """calls: name -> function.  WARM rounds untimed, then REPS rounds with every call timed, the order rotating."""
    names = list(calls)
    spans = {n: [] for n in names}
    for i in range(WARM + REPS):
        for k in range(len(names)):
            n = names[(i + k) % len(names)]
            if i < WARM:
                calls[n]()
            else:
                spans[n].append(span(calls[n]))
    return {n: med(v) for n, v in spans.items()}


# ---- the rows: a rollout of configs[1] -----------------------------------------------------------------------------------
w = config.baseline_workload("C2", arenas=ROWS)
assert w.cfg.n_agents == 1
sim = env.ArenaBatch(w)
sim.reset(*w.seeds())
net = policy.PolicyBatch(policy.init_parameters(seed=0), ROWS)
rb = rollout.RolloutBatch(ROWS, T, LIST_CAP)
i32 = dict(dtype=torch.int32, device="cuda")
d_keys, d_counts, d_act = torch.zeros((ROWS, CAP), **i32), torch.zeros(ROWS, **i32), torch.zeros(ROWS, **i32)
d_vals, d_pov = torch.zeros((ROWS, CAP), device="cuda"), torch.zeros((ROWS, 160), device="cuda")
d_probs, d_value, d_rew = torch.zeros((ROWS, 9), device="cuda"), torch.zeros(ROWS, device="cuda"), torch.zeros(ROWS, device="cuda")
d_cmd = torch.zeros(ROWS, dtype=torch.uint8, device="cuda")
lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
for tick in range(PLAY + T):
    sim.observe_sparse_device(*lists)
    net.predict_sparse(*lists, ROWS, d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr(), seed=7, d_action_ptr=d_act.data_ptr())
    sim.synchronize(), net.synchronize()
    if tick >= PLAY:
        rb.record(d_probs.data_ptr(), d_value.data_ptr(), d_act.data_ptr(), d_rew.data_ptr(), *lists)
        rb.synchronize()
    sim.step_device(d_cmd.data_ptr(), 1)
    sim.synchronize()
counts = rb.counts[0].cpu().numpy().view(np.uint32).astype(np.int64)
fits = counts <= LIST_CAP
entries = int(counts[fits].sum())
out.update(mean_list_entries=float(counts[fits].mean()), rows_that_fit=int(fits.sum()))


def torch_form(dtype, nhwc, dst):
    """The same rows by torch.  dst: [ROWS][30752 + 1]; the entries behind the count go to the last column."""
    k = rb.keys[0].long()
    n = rb.counts[0].long()
    ch, y, x = (k & 511) // 9, (k >> 9) & 31, (k >> 14) & 31
    pos = (y * 31 + x) * 32 + ch if nhwc else (ch * 31 + y) * 31 + x
    live = (torch.arange(LIST_CAP, device="cuda")[None, :] < n[:, None]) & (n[:, None] <= LIST_CAP)
    pos = torch.where(live, pos, rollout.DENSE_ROW)
    dst.zero_()
    dst.scatter_(1, pos, rb.vals[0].to(dtype))


for name, dtype, nhwc in (("nchw_f32", torch.float32, False), ("nhwc_bf16", torch.bfloat16, True)):
    esize = 4 if dtype == torch.float32 else 2
    dense = torch.empty((ROWS, rollout.DENSE_ROW), dtype=dtype, device="cuda")
    valid = torch.empty(ROWS, dtype=torch.uint8, device="cuda")
    wide = torch.empty((ROWS, rollout.DENSE_ROW + 1), dtype=dtype, device="cuda")
    nbytes = ROWS * rollout.DENSE_ROW * esize
    call = lambda: rb.dense(0, dtype=dtype, channels_last=nhwc, out=dense, valid=valid)
    fill = lambda: H.hipMemsetAsync(C.c_void_p(dense.data_ptr()), 0, nbytes, None)
    row = alternate({"memset_a": fill, "dense_a": call, "memset_b": fill, "dense_b": call})
    row.update(alternate({"torch": lambda: torch_form(dtype, nhwc, wide)}))
    call()
    rb.synchronize()
    torch_form(dtype, nhwc, wide)
    row["same_bits_as_torch"] = bool(torch.equal(dense.view(torch.int16), wide[:, :-1].contiguous().view(torch.int16)))
    row["valid_rows"] = int(valid.sum().item())
    # bytes: the fill; beyond it the lists (key + value per entry, the count per row) and the values stored a second time
    extra = entries * 8 + ROWS * 4 + entries * esize
    spread = abs(row["memset_a"]["median"] - row["memset_b"]["median"])
    row.update(bytes_fill=nbytes, bytes_beyond_fill=extra, share_beyond_fill=extra / nbytes, yardstick_spread_ms=spread)
    row["allowed_ms"] = row["memset_a"]["median"] * (1 + extra / nbytes) + spread
    row["dense_over_memset"] = row["dense_a"]["median"] / row["memset_a"]["median"]
    row["within_bound"] = bool(row["dense_a"]["median"] <= row["allowed_ms"])
    row["fill_GBps_dense"] = nbytes / row["dense_a"]["median"] / 1e6
    row["fill_GBps_memset"] = nbytes / row["memset_a"]["median"] / 1e6
    out[name] = row
    del dense, wide
for x in (rb, net, sim):
    x.close()
print(json.dumps(out))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
