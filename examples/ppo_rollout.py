"""gail_loop.py plus the rollout buffer: the learner's whole input collected on the device.

    python examples/ppo_rollout.py [arenas] [steps] [T] [--swap]

One reference `Agent` keeps `states, log_probs, values, rewards, actions` per game and, once T ticks are in, runs
computeReturns() and train_log() over them before its PPO epochs (bots/bot-1/Agent.hpp:200-234, 333-351).  `RolloutBatch`
keeps those five vectors for every agent behind `PolicyBatch.predict_sparse` and `RewardBatch.reward_sparse`: one more launch
per tick, reading the same restart flags.  When agents are ready, the loop takes their returns and advantages (where a PPO
learner would run its epochs over `rb.state(t)`, `rb.action[t]`, `rb.logp[t]`, the returns and the advantages), gives them
a fresh memory in both networks as train() does (:432) and releases their buffers.  Both parameter sets are random here;
the learners themselves are the caller's.  Prints agent-steps/s with and without the record call.

--swap adds the other half of the hand-over, parameters in: both networks' parameters live as torch tensors on the device,
and at every hand-over a STAND-IN for the learner's update — a little noise added in place, NOT a learner — changes them and
`load_weights` puts them into the live objects in stream order (optimizer->step(), Agent.hpp:415-417: the next predict()
runs the new parameters), before the ready agents' memory is reset as above.  A third loop then prints how many loads it did.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from strikeforce_amd import config, env, policy, rollout

SWAP = "--swap" in sys.argv[1:]
argv = [a for a in sys.argv if a != "--swap"]
arenas = int(argv[1]) if len(argv) > 1 else 1024
steps = int(argv[2]) if len(argv) > 2 else 200
T = int(argv[3]) if len(argv) > 3 else 64
CAP, LIST_CAP, CHECK_EVERY = 2048, 512, 16
w = config.baseline_workload("C2", arenas=arenas)           # 64x64 map, 1 player + 16 zombies, auto-reset
sim = env.ArenaBatch(w)
agents = arenas * w.cfg.n_agents
net = policy.PolicyBatch(policy.init_parameters(seed=0), agents)
disc = policy.RewardBatch(policy.init_parameters(seed=1), agents)
rb = rollout.RolloutBatch(agents, T, LIST_CAP)               # T * agents * (8 * LIST_CAP + 640 + ~60) bytes of torch tensors
stream = torch.cuda.Stream()                                 # one stream for the four of them
torch.cuda.set_stream(stream)
for x in (sim, net, disc, rb):
    x.set_stream(stream.cuda_stream)
d_keys = torch.zeros((agents, CAP), dtype=torch.int32, device="cuda")
d_vals = torch.zeros((agents, CAP), dtype=torch.float32, device="cuda")
d_counts = torch.zeros(agents, dtype=torch.int32, device="cuda")
d_pov = torch.zeros((agents, 160), dtype=torch.float32, device="cuda")
d_dense = torch.empty((agents, 32, 31, 31), dtype=torch.float32, device="cuda")  # rows only for lists that do not fit
d_probs = torch.empty((agents, 9), dtype=torch.float32, device="cuda")
d_value = torch.empty(agents, dtype=torch.float32, device="cuda")
d_reward = torch.empty(agents, dtype=torch.float32, device="cuda")
d_cmd = torch.zeros(agents, dtype=torch.uint8, device="cuda")
d_action = torch.zeros(agents, dtype=torch.int32, device="cuda")
d_ready = torch.zeros(agents, dtype=torch.uint8, device="cuda")
restarted = sim.done_view_device()                           # the games that just restarted, where the library keeps the flags
lists = (d_keys.data_ptr(), d_vals.data_ptr(), d_counts.data_ptr(), d_pov.data_ptr(), CAP)
out = None
loads = 0
if SWAP:  # the parameters where a learner holds them: on the device, next to the rollout buffer
    net_params = {k: torch.from_numpy(v).cuda() for k, v in policy.init_parameters(seed=0).items()}
    disc_params = {k: torch.from_numpy(v).cuda() for k, v in policy.init_parameters(seed=1).items() if not k.startswith("policy.")}


def stand_in_update():
    """NOT a learner: noise of 1e-3 of a parameter's scale added in place where optimizer->step() would change it (:415-417,
    RewardNet::train_epoch :428), then the new parameters into the live objects, on the stream the forwards run on."""
    global loads
    for params, obj in ((net_params, net), (disc_params, disc)):
        for p in params.values():
            p.add_(torch.randn_like(p) * p.abs().mean(), alpha=1e-3)
        obj.load_weights(params)
    loads += 1


def loop(record, swap=False):
    global out
    sim.reset(*w.seeds())
    net.reset_memory(), disc.reset_memory(), rb.release(torch.ones(agents, dtype=torch.uint8, device="cuda"))
    trained = 0
    sim.synchronize(), rb.synchronize()
    t0 = time.perf_counter()
    for t in range(steps):
        sim.observe_sparse_device(*lists)
        sim.observe_overflow_device(d_counts.data_ptr(), CAP, d_dense.data_ptr(), d_pov.data_ptr())
        net.predict_sparse(*lists, agents, d_probs.data_ptr(), d_value.data_ptr(), d_cmd.data_ptr(), seed=1234, d_action_ptr=d_action.data_ptr(),
                           d_dense_ptr=d_dense.data_ptr(), reset_words=restarted)
        disc.reward_sparse(*lists, agents, d_action.data_ptr(), d_reward_ptr=d_reward.data_ptr(), d_dense_ptr=d_dense.data_ptr(),
                           reset_words=restarted)
        if record:
            # the five push_backs of this tick, behind the two networks and in front of the step: the same restart flags
            rb.record(d_probs.data_ptr(), d_value.data_ptr(), d_action.data_ptr(), d_reward.data_ptr(), *lists, reset_words=restarted)
        sim.step_device(d_cmd.data_ptr(), 1)
        if record and t % CHECK_EVERY == CHECK_EVERY - 1 and rb.status()[0]:   # (the one synchronisation, every 16th tick)
            out = rb.returns(0.99, out=out)            # returns, log V, advantages [T][agents], statistics [agents][4]
            rb.ready_mask(d_ready)
            # ... a learner's epochs over the ready agents' columns go here ...
            if swap:
                stand_in_update()
            net.reset_memory(d_ready.data_ptr()), disc.reset_memory(d_ready.data_ptr())   # model->reset_memory(), Agent.hpp:432
            trained += int(d_ready.sum().item())
            rb.release()                                # clear(), :430-431
    sim.synchronize(), net.synchronize(), disc.synchronize(), rb.synchronize()
    return time.perf_counter() - t0, trained


dt0, _ = loop(False)
dt1, trained = loop(True)
ready, dropped, missing = rb.status()
print("%d arenas x %d steps, T = %d: %.2f M agent-steps/s without record, %.2f M with; %d buffers handed over, %d ticks dropped, "
      "%d states whose list did not fit %d entries"
      % (arenas, steps, T, agents * steps / dt0 / 1e6, agents * steps / dt1 / 1e6, trained, dropped, missing, LIST_CAP))
if SWAP:
    dt2, trained2 = loop(True, swap=True)
    print("--swap: %d loads of both networks' parameters (a stand-in update, not a learner) at the hand-overs of %d buffers: "
          "%.2f M agent-steps/s" % (loads, trained2, agents * steps / dt2 / 1e6))
if out is not None:
    stats = out[3][~torch.isnan(out[3][:, 0])]
    print("last hand-over: r_avg0 %.4f r_avg1 %.4f n_avg0 %.3f n_avg1 %.3f (means over the %d agents handed over so far)"
          % (tuple(stats.mean(dim=0).tolist()) + (stats.shape[0],)))
