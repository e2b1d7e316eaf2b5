"""Acting-step and update-step times of the feed-forward PPO systems on the bench's headline shape: CoordSum-4ag, 16 384 envs, default nets
([128, 128] relu), ff_mappo.

    python scripts/ff_ppo_timing.py --what step-fused     # one acting step (ff_nets.act_pair) through magpo_mlp_act_step
    python scripts/ff_ppo_timing.py --what step-composed  # the same step as the composed chain of dense kernels per network
    python scripts/ff_ppo_timing.py --what update         # one ff_mappo update step (128-step rollout, 4 epochs x 2 minibatches)
    python scripts/ff_ppo_timing.py --what all --out profiles/ff_ppo_step_time.json   # the three above, one child process each

Each measurement is its own process run.  HIP events after warm-up: the acting step is the median over --steps launches of the whole step
(both networks and the sample; ``nets_median_us`` is the same without the sample), the update step one event pair per step as in bench.py (two
untimed set-up steps for workspaces and the rollout graph capture, then --warmup steps).  The composed chain consists of kernels that exist
without magpo_mlp_act_step, so it is the yardstick of the fused step.  Prints one JSON line per measurement.
"""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magpo_amd.ff_nets import act_pair  # noqa: E402
from magpo_amd.ff_ppo_learner import FfPpoLearner  # noqa: E402
from magpo_amd.learner import CoordSumConfig, SystemConfig, host_split, prng_key  # noqa: E402
from magpo_amd.tuning import Tuning  # noqa: E402

CFG = dict(num_agents=4, num_actions=20, time_limit=100, maxval=60)


def learner(N, fused):
    t = Tuning.from_env()
    if fused is not None:
        t.ff_fused_step = fused
    l = FfPpoLearner(CoordSumConfig(**CFG), N, SystemConfig(), "cuda", centralised=True, net_seed=0, tuning=t)
    l.setup(host_split(prng_key(42), 4)[0])
    return l


def _median_us(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return us, round(sorted(us)[len(us) // 2], 1)


def time_step(N, fused, steps, warmup):
    l = learner(N, fused)
    g, tr = l.groups[0], l.groups[0].traj
    obs_c = l._critic_rows(tr["obs"][0], N, l._gs_step)
    obs_a = l._net_view(tr["obs"][0])
    us, med = _median_us(lambda: act_pair(l.actor, l.critic, obs_a, obs_c, key=g.key, action=tr["action"][0], log_prob=tr["log_prob"][0],
                                          value=tr["value"][0]), steps, warmup)
    _, nets = _median_us(lambda: act_pair(l.actor, l.critic, obs_a, obs_c, value=tr["value"][0]), steps, warmup)
    return dict(us_per_step=[round(x, 1) for x in us[:8]], median_us=med, nets_median_us=nets)


def time_update(N, steps, warmup):
    l = learner(N, None)
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
    sps = l.T * N / (sorted(ms)[len(ms) // 2] * 1e-3)
    return dict(ms_per_update_step=[round(x, 2) for x in ms], median_ms=round(sorted(ms)[len(ms) // 2], 2), env_steps_per_second=round(sps),
                fused_step=bool(l.tuning.ff_fused_step), graph=l.groups[0].graph is not None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("step-fused", "step-composed", "update", "all"), required=True)
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.what == "all":   # one fresh child process per measurement
        lines = []
        for what in ("step-fused", "step-composed", "update"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--what", what, "--num-envs", str(a.num_envs)], capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:
                sys.exit(f"{what} failed ({r.returncode}):\n{r.stderr[-2000:]}")
            lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(lines[-1]))
        text = json.dumps(dict(workload="coordsum-4ag ff_mappo", num_envs=a.num_envs, measurements=lines), indent=1)
    else:
        if a.what == "update":
            res = time_update(a.num_envs, a.steps or 3, 1 if a.warmup is None else a.warmup)
        else:
            res = time_step(a.num_envs, a.what == "step-fused", a.steps or 200, 20 if a.warmup is None else a.warmup)
        text = json.dumps(dict(workload="coordsum-4ag ff_mappo", what=a.what, num_envs=a.num_envs, device=torch.cuda.get_device_name(0), **res))
        print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
