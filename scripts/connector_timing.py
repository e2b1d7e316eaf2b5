"""VectorConnector measurements (csrc/connector.hip and a training step on a Connector scenario).

  env     reset once, then --steps env steps of --num-envs envs with uniform random actions (illegal ones included) on the device.
          Run it under a kernel trace for the per-launch time of k_connector_reset / k_connector_step:
            rocprofv3 --kernel-trace --stats -d OUT -o connector -- python scripts/connector_timing.py env --scenario con-15x15x23a
  update  ms_per_step of the full update step (128-step rollout, GAE, epochs x minibatches, Adam) on con-7x7x5a with its tuned
          MAGPO net and system settings (experiment_data/params.csv: n_embd 128, n_head 1, n_block 3, ppo_epochs 5,
          num_minibatches 8), as bench.py times its workloads: two untimed set-up steps, --warmup steps, then --steps timed ones.
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

SCENARIOS = {"con-5x5x3a": (5, 3, 25), "con-7x7x5a": (7, 5, 49), "con-10x10x10a": (10, 10, 100), "con-15x15x23a": (15, 23, 225)}


def env_run(a):
    from magpo_amd.learner import ConnectorEnvBatch, VectorConnectorConfig, host_split, prng_key
    G, A, TL = SCENARIOS[a.scenario]
    cfg, N = VectorConnectorConfig(G, A, TL), a.num_envs
    env = ConnectorEnvBatch(cfg, N, "cuda")
    keys = torch.empty(N, 2, dtype=torch.int32, device="cuda")
    key = torch.from_numpy(host_split(prng_key(a.seed), 2)[0].view(np.int32)).cuda()
    env.L.call("magpo_threefry_split", key, keys, N, torch.cuda.current_stream().cuda_stream)
    obs, obs_step = torch.zeros(N, A, 128, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    mask, done = torch.zeros(N, A, 5, dtype=torch.uint8, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
    reward, discount = torch.zeros(N, A, device="cuda"), torch.zeros(N, A, device="cuda")
    m_ret, m_len, m_term = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(a.seed)
    actions = torch.randint(0, 5, (a.steps, N, A), dtype=torch.int32, device="cuda", generator=gen)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    env.reset(keys, obs, obs_step, mask)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ends = torch.zeros((), dtype=torch.int64, device="cuda")
    for t in range(a.steps):
        env.step(actions[t], reward, done, obs, obs_step, m_ret, m_len, m_term, auto_reset=True, mask=mask, discount=discount)
        ends += done.sum()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return dict(mode="env", scenario=a.scenario, num_envs=N, steps=a.steps, host_reset_ms=round((t1 - t0) * 1e3, 3),
                host_step_ms=round((t2 - t1) * 1e3 / a.steps, 3), episodes_ended=int(ends.item()))


def update_run(a):
    from magpo_amd.learner import MagpoLearner, SystemConfig, VectorConnectorConfig, host_split, prng_key
    G, A, TL = SCENARIOS["con-7x7x5a"]
    sysc = SystemConfig(ppo_epochs=5, num_minibatches=8, clip_eps=0.1, ent_coef=0.001, actor_lr=5e-4, max_grad_norm=0.5)
    learner = MagpoLearner(VectorConnectorConfig(G, A, TL), a.num_envs, sysc, torch.device("cuda"), net_seed=0, n_block=3, n_head=1,
                           embed_dim=128)
    learner.setup(host_split(prng_key(a.seed), 4)[0])
    for _ in range(2 + a.warmup):   # workspaces, rollout graph capture, warm-up
        learner.update_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        learner.update_step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return dict(mode="update", scenario="con-7x7x5a", net=dict(embed_dim=128, n_head=1, n_block=3), num_envs=a.num_envs,
                rollout_length=sysc.rollout_length, ppo_epochs=sysc.ppo_epochs, num_minibatches=sysc.num_minibatches, steps=a.steps,
                ms_per_step=round(el / a.steps * 1e3, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["env", "update"])
    ap.add_argument("--scenario", default="con-5x5x3a", choices=sorted(SCENARIOS))
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
