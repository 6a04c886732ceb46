"""What new parameters cost a live policy: sf_policy_load_weights against the only way there was before it.

    python tools/policy_load_time.py            # writes profiles/policy_load_time.json

One process, 4096 agents, the folded form and then the layered one (SF_POLICY_LAYERED=1).  Per form, medians of 21 after 5
warm-ups of
  load      PolicyBatch.load_weights(device tensors): host time of the call, device time (events around it, to completion),
            wall time from the call to the stream synchronised
  recreate  what a caller had to do without it: .cpu() of every tensor, close(), a new PolicyBatch — the same three figures
The recreate path runs every kernel the load runs, plus the host staging, ~60 allocations and synchronous copies, the
97 MB of f64 temporaries and the per-agent buffers: the load's wall time has to be below it (asserted; no ratio is fixed).
To be read next to one T = 1024 rollout of the closed loop, about 0.2 s at 0.2 ms per tick."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from strikeforce_amd import policy

AGENTS, WARM, RUNS = 4096, 5, 21
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "policy_load_time.json")


def timed(call):
    """(host ms of call(), device ms between events around it, wall ms until the device is idle)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    call()
    t1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, e0.elapsed_time(e1), (t2 - t0) * 1e3


def medians(call):
    rows = [timed(call) for _ in range(WARM + RUNS)][WARM:]
    return dict(zip(("host_ms", "device_ms", "wall_ms"), (round(statistics.median(c), 4) for c in zip(*rows))))


def measure(form):
    if form == "layered":
        os.environ["SF_POLICY_LAYERED"] = "1"
    else:
        os.environ.pop("SF_POLICY_LAYERED", None)
    params = {k: torch.from_numpy(v).cuda() for k, v in policy.init_parameters(seed=0).items()}
    held = {"net": policy.PolicyBatch(policy.init_parameters(seed=1), AGENTS)}

    def load():
        held["net"].load_weights(params)

    def recreate():
        host = {k: v.cpu().numpy() for k, v in params.items()}
        held["net"].close()
        held["net"] = policy.PolicyBatch(host, AGENTS)

    want = None
    res = {"load": medians(load)}
    got = held["net"].weights_digest()
    res["recreate"] = medians(recreate)
    want = held["net"].weights_digest()
    held["net"].close()
    res["digests_equal"] = got == want
    return res


def main():
    result = {"agents": AGENTS, "warmups": WARM, "runs": RUNS, "device": torch.cuda.get_device_name(0), "forms": {}}
    ok = True
    for form in ("folded", "layered"):
        r = measure(form)
        result["forms"][form] = r
        ok = ok and r["digests_equal"] and r["load"]["wall_ms"] < r["recreate"]["wall_ms"]
        print(form, json.dumps(r))
    result["load_wall_below_recreate_wall"] = ok
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if not ok:
        sys.exit("the load is not faster than recreating the object (or the images differ)")


if __name__ == "__main__":
    main()
