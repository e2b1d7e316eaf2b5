"""ms per update step of rec_sable next to rec_magpo on the bench's headline shape: CoordSum-4ag, 16 384 envs, default net, reference default
system settings (128-step rollout, 4 epochs x 2 minibatches).  Same protocol as bench.py: two untimed set-up steps (workspaces, rollout graph
capture), --warmup steps, then --steps steps timed with one HIP event pair each.  Prints one line per system and one JSON line.

    python scripts/sable_timing.py [--num-envs 16384] [--steps 3] [--warmup 1] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magpo_amd.learner import CoordSumConfig, MagpoLearner, SystemConfig, host_split, prng_key  # noqa: E402
from magpo_amd.sable_learner import SableLearner  # noqa: E402


def measure(cls, N, steps, warmup):
    learner = cls(CoordSumConfig(num_agents=4, num_actions=20, time_limit=100, maxval=60), N, SystemConfig(), "cuda", net_seed=0)
    learner.setup(host_split(prng_key(42), 4)[0])
    for _ in range(2 + warmup):
        learner.update_step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        learner.update_step()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    del learner
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    for name, cls in (("rec_magpo", MagpoLearner), ("rec_sable", SableLearner)):
        ms = measure(cls, a.num_envs, a.steps, a.warmup)
        res[name] = dict(ms_per_update_step=[round(x, 2) for x in ms], median_ms=round(sorted(ms)[len(ms) // 2], 2))
        print(f"{name}: ms per update step {res[name]['ms_per_update_step']} (median {res[name]['median_ms']}) at {a.num_envs} envs, "
              f"{a.num_envs * 128 / res[name]['median_ms'] * 1e-3:.2f} M env-steps/s")
    line = json.dumps(dict(workload="coordsum-4ag", num_envs=a.num_envs, warmup=a.warmup, steps=a.steps, device=torch.cuda.get_device_name(0), **res))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
