"""The observation kernels' test matrix on the device, for one world of tests/obs_cases.py (test helper; needs a GPU).

One run of the world, the oracle in lock-step:
- before EVERY step: sf_observe_device_delta into one of two persistent buffers (obs_cases.delta_plan: runs of calls on one
  buffer, pointer changes, a plain call on the tracked buffer, the caller scribbling where the header allows it) against
  the plain call, bit for bit; at the end once more across sf_reset;
- at every sampled step: the dense observation from the host call and from the device call against the oracle (zero
  pattern exact, values within 1 float ulp, the two calls bitwise equal); the list against the dense form in key, value,
  count and pov, with the crowded marker asserted IF AND ONLY IF the oracle's window statistics say so; the overflow redo
  into a NaN-filled buffer (flagged rows = the dense rows, every other row still NaN, pov rows rewritten or untouched).

run() returns a report: how many windows were compared, how many took which path by the reference statistics, the largest
ulp difference.  As a program it runs one world against whatever library SF_LIBRARY_PATH names and prints the report as a
JSON line: tests/test_gpu_obs_edges.py starts it as a child process for the small-limits flavour (tests/obs_flavour.py)
and for SF_OBS_LIST_BLOCK=1, both of which the library reads once per process."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # (run as a program: the package lies beside tests/)
    sys.path.insert(0, ROOT)

import obs_cases as oc  # noqa: E402
import obs_flavour  # noqa: E402

F = 32 * oc.W2
GARBAGE = 7.0


def _ulp(x, y):
    return np.abs(x.view(np.int32).astype(np.int64) - y.view(np.int32).astype(np.int64))


def _centre(row):
    r = row.reshape(32, oc.W, oc.W)
    return np.stack([r[:, yy, xx] for yy, xx in oc.CENTRE]).reshape(160)


def delta_events(prev, st, s, lim):
    """What the delta call on the state after s steps meets, from the reference statistics of that state and of the
    state one step earlier (None if that one was not sampled)."""
    ev = {"incremental_calls": 0, "spilled_in_incremental": 0, "back_from_spill": 0, "observer_died": 0}
    if not oc.delta_is_incremental(s):
        return ev
    ev["incremental_calls"] = 1
    sp = oc.spilled(st, lim)
    ev["spilled_in_incremental"] = int(sp.sum())
    if prev is not None:
        ev["back_from_spill"] = int((oc.spilled(prev, lim) & st.live & ~sp).sum())
        ev["observer_died"] = int((prev.live & ~st.live).sum())
    return ev


def path_counts(st, lim, caps, list_block=False):
    """How many of the sample's live windows take each path, by the reference statistics (list_block: the list comes from
    mode 3 of the dense kernel, which marks the windows it spills)."""
    sp = oc.spilled(st, lim)
    mk = sp if list_block else oc.marked(st, lim)
    un = st.live & ~mk
    c = {"windows": int(st.live.sum()), "no_observer": int((~st.live).sum()), "marked": int(mk.sum()),
         "marked_by_records": int((st.live & (st.own > lim["ol_rec"])).sum()),
         "marked_by_cells": int((st.live & (st.cells > lim["ol_cells"])).sum()),
         "cells_at_limit": int((st.live & (st.cells == lim["ol_cells"])).sum()),
         "cells_one_over": int((st.live & (st.cells == lim["ol_cells"] + 1)).sum()),
         "last_pass": int((un & (st.cells > lim["ol_cells"] - 64)).sum()),
         "dense_spill": int(sp.sum()),
         "dense_queue_over": int((st.live & ~sp & (st.q_dense > lim["list"])).sum()),
         "list_queue_over": int((un & (st.q_list > lim["ol_powq"])).sum()),
         "over_staged": int((st.live & ~sp & (st.nz > lim["staged"])).sum())}
    for cap in caps:
        c["over_cap_%d" % cap] = int((un & (st.nz > cap)).sum())
    return c


def add(total, part):
    for k, v in part.items():
        total[k] = total.get(k, 0) + v


def oracle_report(world, lim):
    """The world's run on the oracle alone: the path counts and delta events run() will meet, and what else the run
    reaches (fewest / most non-zeros of a live window, most live zombies in an arena, finished episodes)."""
    rep = {"world": world.name, "samples": 0, "nz_min": 1 << 30, "nz_max": 0, "zombies_max": 0}
    prev, prev_s = None, None
    for s, o in oc.run_oracle(world):
        st = oc.window_stats(o, check=True)
        add(rep, path_counts(st, lim, world.caps))
        add(rep, delta_events(prev if prev_s == s - 1 else None, st, s, lim))
        rep["samples"] += 1
        if st.live.any():
            rep["nz_min"] = min(rep["nz_min"], int(st.nz[st.live].min()))
            rep["nz_max"] = max(rep["nz_max"], int(st.nz[st.live].max()))
        rep["zombies_max"] = max([rep["zombies_max"]] + [sum(z.alive for z in o.dump(a).zombies) for a in range(world.arenas)])
        prev, prev_s = st, s
    rep["episodes"] = int(sum(o.dump(a).hdr.episodes for a in range(world.arenas)))
    return rep


def run(world, lim, list_block=False, log=None):
    """list_block: the library runs the list as mode 3 of the dense kernel (SF_OBS_LIST_BLOCK): only the list checks are
    made, and the marker is the dense kernel's (more own records than it has)."""
    import torch
    from oracle_lib import Oracle
    from strikeforce_amd import env
    t0 = time.time()
    w = world.workload()
    o, g = Oracle(w), env.ArenaBatch(w)
    tb, sr = w.seeds()
    o.reset(tb, sr), g.reset(tb, sr)
    A, G = w.cfg.arenas, w.cfg.n_agents
    B = A * G
    cmds = np.ascontiguousarray(world.commands(G))
    d_cmds = torch.from_numpy(cmds).cuda()
    keep = [torch.full((B, F), GARBAGE, dtype=torch.float32, device="cuda") for _ in range(2)]
    full = torch.empty((B, F), dtype=torch.float32, device="cuda")
    d_obs = torch.zeros((B, F), dtype=torch.float32, device="cuda")
    d_fb = torch.empty((B, F), dtype=torch.float32, device="cuda")
    rep = {"world": world.name, "list_block": bool(list_block), "samples": 0, "max_ulp": 0, "delta_calls": 0}
    samples = set(world.samples)

    def delta_call(s, what=None):
        buf, plan = oc.delta_plan(s)
        k = keep[buf]
        what = what or plan
        if what == "switch":
            k.fill_(GARBAGE)  # (untracked since the other buffer's first call: the caller may have written to it)
        elif what == "plain-then-delta":
            g.observe_device(k.data_ptr())
            k[:, ::97] = 9.0
        g.observe_device_delta(k.data_ptr())
        g.observe_device(full.data_ptr())
        g.synchronize()
        assert torch.equal(k.view(torch.int32), full.view(torch.int32)), "%s: delta call after %d steps (%s)" % (world.name, s, what)
        rep["delta_calls"] += 1

    def check_list(s, cap, y, st, mark):
        keys = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
        vals = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
        counts = torch.full((B,), 12345, dtype=torch.int32, device="cuda")
        pov = torch.full((B, 160), GARBAGE, dtype=torch.float32, device="cuda")
        g.observe_sparse_device(keys.data_ptr(), vals.data_ptr(), counts.data_ptr(), pov.data_ptr(), cap)
        g.synchronize()
        k, v, n = keys.cpu().numpy().view(np.uint32), vals.cpu().numpy(), counts.cpu().numpy().view(np.uint32)
        pv = pov.cpu().numpy()
        live = st.flat("live")
        for b in range(B):
            where = "%s after %d steps, agent %d, cap %d" % (world.name, s, b, cap)
            if mark[b]:
                assert n[b] == oc.MARK, "%s: not marked (count %d; own %d, cells %d)" % (where, n[b], st.flat("own")[b], st.flat("cells")[b])
                continue
            assert n[b] != oc.MARK, "%s: marked (own %d, cells %d)" % (where, st.flat("own")[b], st.flat("cells")[b])
            nz = np.flatnonzero(y[b])
            assert n[b] == len(nz), "%s: count %d, the dense row has %d" % (where, n[b], len(nz))
            assert live[b] or n[b] == 0
            m = min(len(nz), cap)
            ch, r = np.divmod(nz[:m], oc.W2)
            yy, xx = np.divmod(r, oc.W)
            assert np.array_equal(k[b, :m], (ch * 9) | (yy << 9) | (xx << 14)), where
            assert np.array_equal(v[b, :m].view(np.uint32), y[b][nz[:m]].view(np.uint32)), where
            assert np.array_equal(pv[b].view(np.uint32), _centre(y[b]).view(np.uint32)), where
        if list_block:
            return
        # the overflow redo: exactly the flagged agents' rows, from the dense kernel
        flagged = mark | (st.flat("live") & (st.flat("nz") > cap))
        d_fb.fill_(float("nan"))
        g.observe_overflow_device(counts.data_ptr(), cap, d_fb.data_ptr(), pov.data_ptr())
        g.synchronize()
        fb, pv2 = d_fb.cpu().numpy(), pov.cpu().numpy()
        for b in range(B):
            where = "%s after %d steps, agent %d, cap %d: redo" % (world.name, s, b, cap)
            if flagged[b]:
                assert np.array_equal(fb[b].view(np.uint32), y[b].view(np.uint32)), where
                assert np.array_equal(pv2[b].view(np.uint32), _centre(y[b]).view(np.uint32)), where
            else:
                assert np.isnan(fb[b]).all(), where
                assert np.array_equal(pv2[b].view(np.uint32), pv[b].view(np.uint32)), where
        rep["redone_rows"] = rep.get("redone_rows", 0) + int(flagged.sum())

    def sample(s, prev):
        x = o.observe().reshape(B, F)
        st = oc.window_stats(o, x)
        y = g.observe().reshape(B, F)  # the host call
        assert np.array_equal(x == 0, y == 0), "%s after %d steps: zero pattern" % (world.name, s)
        ulp = int(_ulp(x, y).max())
        rep["max_ulp"] = max(rep["max_ulp"], ulp)
        if log:
            log("%s after %d steps: %d windows, max ulp %d" % (world.name, s, int(st.live.sum()), ulp))
        assert ulp <= 1, "%s after %d steps: max ulp %d" % (world.name, s, ulp)
        assert not y[~st.flat("live")].any()
        if not list_block:
            g.observe_device(d_obs.data_ptr())
            g.synchronize()
            assert np.array_equal(d_obs.cpu().numpy().view(np.uint32), y.view(np.uint32)), "%s after %d steps: host and device call" % (world.name, s)
        mark = (oc.spilled(st, lim) if list_block else oc.marked(st, lim)).reshape(-1)
        for cap in world.caps:
            check_list(s, cap, y, st, mark)
        rep["samples"] += 1
        add(rep, path_counts(st, lim, world.caps, list_block))
        add(rep, delta_events(prev, st, s, lim))
        return st

    start = max(0, world.samples[0] - 24)  # (a world that is sampled late gets there in one launch)
    if start:
        o.step_many(cmds[:start])
        g.step_device(d_cmds.data_ptr(), start)
        g.synchronize()
    prev = None
    for s in range(start, world.steps + 1):
        if not list_block:
            delta_call(s)
        prev = sample(s, prev) if s in samples else None
        if s < world.steps:
            o.step(cmds[s])
            g.step_device(d_cmds.data_ptr() + s * B, 1)
    assert (o.digest() == g.digest()).all()
    rep["episodes"] = int(sum(o.dump(a).hdr.episodes for a in range(A)))
    if not list_block:  # across sf_reset: the tracked buffer still holds the last game's observation
        o.reset(tb, sr), g.reset(tb, sr)
        for s in range(3):
            delta_call(world.steps, "delta")
            o.step(cmds[s])
            g.step_device(d_cmds.data_ptr() + s * B, 1)
        assert (o.digest() == g.digest()).all()
    rep["seconds"] = round(time.time() - t0, 1)
    return rep


def main(argv):
    world, lim = oc.WORLDS[argv[0]], {"product": obs_flavour.PRODUCT, "small": obs_flavour.SMALL}[argv[1]]
    rep = run(world, lim, list_block="--list-block" in argv, log=lambda m: print(m, flush=True))
    print("REPORT " + json.dumps(rep), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
