"""Acting-step and training-epoch times of rec_iql at the default config's shape (Level-Based Foraging 2s-8x8-2p-2f-coop, 16 envs, ring 1000,
32 windows of 32 steps) and at 4 096 envs.

    python scripts/iql_timing.py --what act      # one acting step: Q-network step, eps-greedy sample, env step with real_next_obs, ring add
    python scripts/iql_timing.py --what epoch    # one training epoch: sample, gather, three unrolls, TD loss, backward, clip + Adam, target update
    python scripts/iql_timing.py --what update   # one whole update step (rollout_length acting steps as a replayed graph + epochs)

Each measurement is its own process run.  HIP events after warm-up; the median over --steps repetitions.  The ring is filled with real
transitions before an epoch is timed.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magpo_amd.envs import LbfConfig, host_split, prng_key  # noqa: E402
from magpo_amd.q_learner import QLearner, QSystemConfig  # noqa: E402

ENV = dict(grid_size=8, fov=2, num_agents=2, num_food=2, max_agent_level=2, force_coop=True, time_limit=100)


def learner(N, buffer_size):
    l = QLearner(LbfConfig(**ENV), N, QSystemConfig(buffer_size=buffer_size), "cuda", net_seed=0)
    l.setup(host_split(prng_key(1), 2)[0])
    return l


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
    return sorted(ms)[len(ms) // 2], ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("act", "epoch", "update"), required=True)
    ap.add_argument("--num-envs", type=int, default=16)
    ap.add_argument("--buffer-size", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    l = learner(a.num_envs, a.buffer_size)
    g = l.groups[0]
    if a.what == "act":      # eager acting steps of rollout_length 2: the time per env step
        l.use_graph = False

        def fn():
            l.rollout()
            l._carry_over()
        med, ms = _median_ms(fn, a.steps, a.warmup)
        res = dict(median_us_per_env_step=round(med * 1e3 / l.T, 1), first=[round(x * 1e3 / l.T, 1) for x in ms[:6]])
    else:
        while not l.ready():
            l.rollout()
            l._carry_over()
        if a.what == "epoch":
            s = l.sys
            s.epochs = 1
            med, ms = _median_ms(lambda: l.update(), a.steps, a.warmup)
            res = dict(median_ms_per_epoch=round(med, 3), first=[round(x, 3) for x in ms[:6]], rows=l._mb["R"])
        else:
            med, ms = _median_ms(lambda: l.update_step(), a.steps, a.warmup + 2)
            res = dict(median_ms_per_update_step=round(med, 3), first=[round(x, 3) for x in ms[:6]], graph=g.graph is not None)
    line = json.dumps(dict(workload="lbf 2s-8x8-2p-2f-coop rec_iql", what=a.what, num_envs=a.num_envs, buffer_size=a.buffer_size,
                           ring_mib=round(g.ring_bytes() / 2 ** 20, 2), device=torch.cuda.get_device_name(0), **res))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
