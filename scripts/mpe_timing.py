"""MPE simple_spread measurements (csrc/mpe.hip and a training step on simple_spread_10ag).

  env     reset once, then --steps env steps of --num-envs envs with uniform random actions on the device.  Run it under a kernel
          trace for the per-launch time of k_mpe_reset / k_mpe_step:
            rocprofv3 --kernel-trace --stats -d OUT -o mpe -- python scripts/mpe_timing.py env --scenario simple_spread_10ag
  update  ms_per_step of the full update step (128-step rollout, GAE, epochs x minibatches, Adam) on simple_spread_10ag with its tuned
          MAGPO net and system settings (experiment_data/params.csv:101: n_embd 128, n_head 2, n_block 1, ppo_epochs 5, num_minibatches 4,
          clip_eps 0.2, ent_coef 0.01, actor_lr 1e-3, max_grad_norm 10, decay_scaling_factor 0.3, alpha 2), as bench.py times its
          workloads: two untimed set-up steps, --warmup steps, then --steps timed ones.
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

SCENARIOS = {"simple_spread_3ag": 3, "simple_spread_5ag": 5, "simple_spread_10ag": 10}


def env_run(a):
    from magpo_amd.learner import MpeConfig, MpeEnvBatch, host_split, obs_row_stride, prng_key
    A = SCENARIOS[a.scenario]
    cfg, N = MpeConfig(A, A), a.num_envs
    env = MpeEnvBatch(cfg, N, "cuda")
    keys = torch.empty(N, 2, dtype=torch.int32, device="cuda")
    key = torch.from_numpy(host_split(prng_key(a.seed), 2)[0].view(np.int32)).cuda()
    env.L.call("magpo_threefry_split", key, keys, N, torch.cuda.current_stream().cuda_stream)
    obs, obs_step = torch.zeros(N, A, obs_row_stride(cfg.obs_dim), device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    done = torch.zeros(N, dtype=torch.uint8, device="cuda")
    reward, discount = torch.zeros(N, A, device="cuda"), torch.zeros(N, A, device="cuda")
    m_ret, m_len, m_term = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    actions = torch.randint(0, 5, (a.steps, N, A), dtype=torch.int32, device="cuda", generator=gen)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    env.reset(keys, obs, obs_step)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ends = torch.zeros((), dtype=torch.int64, device="cuda")
    for t in range(a.steps):
        env.step(actions[t], reward, done, obs, obs_step, m_ret, m_len, m_term, auto_reset=True, discount=discount)
        ends += done.sum()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return dict(mode="env", scenario=a.scenario, num_envs=N, steps=a.steps, host_reset_ms=round((t1 - t0) * 1e3, 3),
                host_step_ms=round((t2 - t1) * 1e3 / a.steps, 3), episodes_ended=int(ends.item()))


def update_run(a):
    from magpo_amd.learner import MagpoLearner, MpeConfig, SystemConfig, host_split, prng_key
    sysc = SystemConfig(ppo_epochs=5, num_minibatches=4, clip_eps=0.2, ent_coef=0.01, actor_lr=1e-3, max_grad_norm=10.0, alpha=2.0)
    learner = MagpoLearner(MpeConfig(10, 10), a.num_envs, sysc, torch.device("cuda"), net_seed=0, n_block=1, n_head=2, embed_dim=128,
                           decay_scaling_factor=0.3)
    learner.setup(host_split(prng_key(a.seed), 4)[0])
    for _ in range(2 + a.warmup):   # workspaces, rollout graph capture, warm-up
        learner.update_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        learner.update_step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return dict(mode="update", scenario="simple_spread_10ag", net=dict(embed_dim=128, n_head=2, n_block=1), num_envs=a.num_envs,
                rollout_length=sysc.rollout_length, ppo_epochs=sysc.ppo_epochs, num_minibatches=sysc.num_minibatches, steps=a.steps,
                ms_per_step=round(el / a.steps * 1e3, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["env", "update"])
    ap.add_argument("--scenario", default="simple_spread_3ag", choices=sorted(SCENARIOS))
    ap.add_argument("--num-envs", type=int, default=None, help="default: 16384 (env), 4096 (update)")
    ap.add_argument("--steps", type=int, default=None, help="default: 50 env steps / 5 update steps")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.mode == "env":
        a.num_envs, a.steps = a.num_envs or 16384, a.steps or 50
        out = env_run(a)
    else:
        a.num_envs, a.steps = a.num_envs or 4096, a.steps or 5
        out = update_run(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
