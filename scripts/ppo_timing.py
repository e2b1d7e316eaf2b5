"""Acting-step and update-step times of the recurrent PPO systems on the bench's headline shape: CoordSum-4ag, 16 384 envs, default nets.

    python scripts/ppo_timing.py --what step-fused     # one acting step (critic.step_pair) through magpo_gru_cell_step
    python scripts/ppo_timing.py --what step-composed  # the same step as the composed GruActor.step of each network
    python scripts/ppo_timing.py --what update         # one rec_mappo update step (128-step rollout, 4 epochs x 2 minibatches)

Each measurement is its own process run.  HIP events after warm-up: the acting step is the median over --steps launches of the whole step
(both pre-torsos, the GRU cells, both post-torsos and heads, the sample), the update step one event pair per step as in bench.py (two untimed
set-up steps for workspaces and the rollout graph capture, then --warmup steps).  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magpo_amd.critic import step_pair  # noqa: E402
from magpo_amd.learner import CoordSumConfig, SystemConfig, host_split, prng_key  # noqa: E402
from magpo_amd.ppo_learner import PpoLearner  # noqa: E402
from magpo_amd.tuning import Tuning  # noqa: E402

CFG = dict(num_agents=4, num_actions=20, time_limit=100, maxval=60)


def learner(N, fused):
    t = Tuning.from_env()
    t.ppo_fused_step = fused
    l = PpoLearner(CoordSumConfig(**CFG), N, SystemConfig(), "cuda", centralised=True, net_seed=0, tuning=t)
    l.setup(host_split(prng_key(42), 4)[0])
    return l


def time_step(N, fused, steps, warmup):
    l = learner(N, fused)
    g, tr = l.groups[0], l.groups[0].traj
    obs_c = l._critic_rows(tr["obs"][0], N, l._gs_step)

    def one(i):
        step_pair(l.actor, l.critic, l._net_view(tr["obs"][0]), obs_c, tr["done"][0], g.policy_h[i & 1], g.policy_h[1 - (i & 1)], g.critic_h[i & 1],
                  g.critic_h[1 - (i & 1)], key=g.key, action=tr["action"][0], log_prob=tr["log_prob"][0], value=tr["value"][0])
    for i in range(warmup):
        one(i)
    torch.cuda.synchronize()
    us = []
    for i in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        one(i)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return dict(us_per_step=[round(x, 1) for x in us[:8]], median_us=round(sorted(us)[len(us) // 2], 1))


def time_update(N, steps, warmup):
    l = learner(N, Tuning().ppo_fused_step)
    for _ in range(2 + warmup):
        l.update_step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        l.update_step()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(ms_per_update_step=[round(x, 2) for x in ms], median_ms=round(sorted(ms)[len(ms) // 2], 2), fused_step=bool(l.tuning.ppo_fused_step))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("step-fused", "step-composed", "update"), required=True)
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.what == "update":
        res = time_update(a.num_envs, a.steps or 3, 1 if a.warmup is None else a.warmup)
    else:
        res = time_step(a.num_envs, a.what == "step-fused", a.steps or 200, 20 if a.warmup is None else a.warmup)
    line = json.dumps(dict(workload="coordsum-4ag rec_mappo", what=a.what, num_envs=a.num_envs, device=torch.cuda.get_device_name(0), **res))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
