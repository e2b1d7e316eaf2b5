"""Acting-step, training-epoch and update-step times of rec_qmix at one shape (Level-Based Foraging 2s-8x8-2p-2f-coop, 16 envs, ring 1000,
32 windows of 32 steps), the summed time of its mixer launches, and rec_iql's epoch at the same shape, all in ONE process:

    python scripts/qmix_timing.py [--steps 50] [--warmup 5] [--out FILE]

HIP events after warm-up; medians over --steps repetitions of each timed region.  The rings are filled with real transitions before an epoch
is timed.  ``calls`` counts the library entry points of one epoch by name (an entry point is one launch, except: magpo_clip_adam 3,
magpo_qmix_bwd 2, magpo_qmix_td_loss 2, magpo_q_td_loss 2, magpo_wgrad / magpo_dense_bwd with their slab folds).  Prints one JSON line.
"""
import argparse
import collections
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magpo_amd._lib import lib  # noqa: E402
from magpo_amd.envs import LbfConfig, host_split, prng_key  # noqa: E402
from magpo_amd.q_learner import QLearner, QSystemConfig  # noqa: E402
from magpo_amd.qmix_learner import QmixLearner  # noqa: E402

ENV = dict(grid_size=8, fov=2, num_agents=2, num_food=2, max_agent_level=2, force_coop=True, time_limit=100)


def _median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2]


class _Counter:
    def __init__(self):
        self.n = collections.Counter()

    def begin(self, name, args):
        self.n[name] += 1
        return None


def _calls(fn):
    c = _Counter()
    lib().timer = c
    try:
        fn()
    finally:
        del lib().timer   # (back to the class default: no timer)
    return dict(c.n)


def _fill(l):
    while not l.ready():
        l.rollout()
        l._carry_over()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16)
    ap.add_argument("--buffer-size", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    key = host_split(prng_key(1), 2)[0]
    res = {}
    # ---- rec_qmix
    l = QmixLearner(LbfConfig(**ENV), a.num_envs, QSystemConfig(buffer_size=a.buffer_size), "cuda", net_seed=0, mixer_seed=0)
    l.setup(key)
    l.use_graph = False

    def act():
        l.rollout()
        l._carry_over()
    res["qmix_us_per_env_step_eager"] = round(_median_ms(act, a.steps, a.warmup) * 1e3 / l.T, 1)
    l.use_graph = True
    _fill(l)
    epochs = l.sys.epochs
    res["qmix_ms_per_update_step"] = round(_median_ms(lambda: l.update_step(), a.steps, a.warmup + 2), 3)
    res["qmix_epochs_per_update_step"], res["graph"] = epochs, l.groups[0].graph is not None
    l.sys.epochs = 1
    res["qmix_ms_per_epoch"] = round(_median_ms(lambda: l.update(), a.steps, a.warmup), 3)
    res["qmix_calls_per_epoch"] = _calls(lambda: l.update())
    # the mixer's launches on the buffers the last epoch left: target forward, online forward, TD loss, backward with slab fold
    m, s, A, K = l._mb, l.sys, l.A, l.K
    L_, Rm = int(s.sample_sequence_length), l._mb["Rm"]
    T = L_ - 1
    q_all, q_target, st = l.q_net.b.t["t_logits"], l.target_net.b.t["t_logits"], l._st()
    parts = {
        "target_fwd": lambda: l.mixer_target.apply(m["obs"], l.Fld, Rm, q_target, q_online=q_all, mask=m["mask"], K=K, steps=(T, L_, 1), out=m["next_q_tot"]),
        "online_fwd": lambda: l.mixer.apply(m["obs"], l.Fld, Rm, q_all, index=m["action"], K=K, steps=(T, L_, 0), train=True, out=m["q_tot"]),
        "td_loss": lambda: l.L.call("magpo_qmix_td_loss", m["q_tot"], m["next_q_tot"], m["reward"], m["tot"], L_, s.gamma, m["dq_tot"], l.ws64, l.loss_out, Rm, 1, st),
        "bwd_with_fold": lambda: l.mixer.bwd(m["dq_tot"], dq64=m["dq"]),
    }
    res["mixer_us"] = {k: round(_median_ms(fn, a.steps, a.warmup) * 1e3, 1) for k, fn in parts.items()}
    res["mixer_us_sum"] = round(sum(res["mixer_us"].values()), 1)
    res["mixer_rows"], res["unroll_rows"] = Rm, m["R"]
    # ---- rec_iql at the same shape (the parent commit's code)
    li = QLearner(LbfConfig(**ENV), a.num_envs, QSystemConfig(buffer_size=a.buffer_size), "cuda", net_seed=0)
    li.setup(key)
    _fill(li)
    li.sys.epochs = 1
    res["iql_ms_per_epoch"] = round(_median_ms(lambda: li.update(), a.steps, a.warmup), 3)
    res["iql_calls_per_epoch"] = _calls(lambda: li.update())
    res["qmix_over_iql_epoch"] = round(res["qmix_ms_per_epoch"] / res["iql_ms_per_epoch"], 3)
    line = json.dumps(dict(workload="lbf 2s-8x8-2p-2f-coop rec_qmix vs rec_iql", num_envs=a.num_envs, buffer_size=a.buffer_size, sample_batch_size=int(s.sample_batch_size),
                           sample_sequence_length=L_, device=torch.cuda.get_device_name(0), **res))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
