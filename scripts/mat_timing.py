"""Acting-step and update-step times of the MAT system against ff_sable at the same shape: CoordSum 8x15 (8 agents, 15 actions), 16 384
envs, 128-step rollout, the tuned network of the reference's experiment_data/params.csv for that task (embed_dim 64, two blocks; --n-head
for the heads), both systems at configs/system defaults of ff_sable (4 epochs x 2 minibatches) so that only the network differs.

    python scripts/mat_timing.py --what act --system mat        # one acting step: MatNetwork.act (encoder + A decoder iterations)
    python scripts/mat_timing.py --what act --system ff_sable   # SableGuider.act, the kernel-by-kernel chain on team-retention kernels
    python scripts/mat_timing.py --what update --system mat|ff_sable
    python scripts/mat_timing.py --what all --out profiles/mat_step_time.json   # the four of them, one child process each

Each measurement is its own process under its own time limit.  HIP events after warm-up: the acting step is a median over --steps calls,
the update step one event pair per step as in bench.py (two untimed set-up steps for workspaces and the rollout graph capture, then
--warmup steps).  ``calls_per_act`` is the number of library entry points one acting step makes.  There is no pass / fail threshold on
time.  Prints one JSON line per measurement.
"""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magpo_amd.learner import CoordSumConfig, SystemConfig, host_split, obs_row_stride, prng_key  # noqa: E402

CFG = dict(num_agents=8, num_actions=15, time_limit=100, maxval=100)
N_BLOCK = 2
WORKLOAD = "coordsum-8x15 mat vs ff_sable"


def learner(system, N, n_head):
    from magpo_amd.ff_sable_learner import FfSableLearner
    from magpo_amd.tuning import Tuning
    cfg, sysc = CoordSumConfig(**CFG), SystemConfig()
    if system == "mat":
        from magpo_amd.mat import MatNetwork
        from magpo_amd.optim import ClipAdam
        net = MatNetwork(cfg.num_agents, cfg.num_actions, cfg.obs_dim, "cuda", n_head=n_head, n_block=N_BLOCK, seed=0, obs_ld=obs_row_stride(cfg.obs_dim))
        l = FfSableLearner(cfg, N, sysc, "cuda", guider=net, optim=ClipAdam(net, sysc), apply_fns=(net.act, net.apply))
    else:
        t = Tuning.from_env()
        t.ff_sable_fused_act = False
        l = FfSableLearner(cfg, N, sysc, "cuda", net_seed=0, n_block=N_BLOCK, n_head=n_head, tuning=t)
    l.setup(host_split(prng_key(42), 3)[0])
    return l


def time_act(system, N, n_head, steps, warmup):
    l = learner(system, N, n_head)
    g, tr = l.groups[0], l.groups[0].traj
    l._rollout_keys(g)
    obs, act = l._net_view(tr["obs"][0]), l.sable_action_select_fn
    fn = lambda: act(obs, tr["step_count"][0], None, g.keys_host[0], tr["action"][0], tr["log_prob"][0], tr["value"][0])
    counts = {}
    orig = l.L.call

    def counting(name, *a):
        counts[name] = counts.get(name, 0) + 1
        return orig(name, *a)
    l.L.call = counting
    fn()
    del l.L.call
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
    return dict(method=f"{type(l.guider).__name__}.{act.__name__}", calls_per_act=sum(counts.values()), us_per_step=[round(x, 1) for x in us[:8]],
                median_us=round(sorted(us)[len(us) // 2], 1))


def time_update(system, N, n_head, steps, warmup):
    l = learner(system, N, n_head)
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
    med = sorted(ms)[len(ms) // 2]
    return dict(ms_per_update_step=[round(x, 2) for x in ms], median_ms=round(med, 2), env_steps_per_second=round(l.T * N / (med * 1e-3)),
                graph=l.groups[0].graph is not None, peak_hbm_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("act", "update", "all"), required=True)
    ap.add_argument("--system", choices=("mat", "ff_sable"), default="mat")
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--n-head", type=int, default=2)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.what == "all":   # one fresh child process per measurement, each under its own time limit
        lines = []
        for what in ("act", "update"):
            for system in ("mat", "ff_sable"):
                cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--what", what, "--system", system,
                       "--num-envs", str(a.num_envs), "--n-head", str(a.n_head)]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:   # nothing more is started on the GPU after a failed measurement
                    sys.exit(f"{what} {system} failed ({r.returncode}):\n{r.stderr[-2000:]}")
                lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(json.dumps(lines[-1]), flush=True)
        text = json.dumps(dict(workload=WORKLOAD, num_envs=a.num_envs, measurements=lines), indent=1)
    else:
        if a.what == "act":
            res = time_act(a.system, a.num_envs, a.n_head, a.steps or 50, 5 if a.warmup is None else a.warmup)
        else:
            res = time_update(a.system, a.num_envs, a.n_head, a.steps or 3, 1 if a.warmup is None else a.warmup)
        text = json.dumps(dict(workload=WORKLOAD, what=a.what, system=a.system, num_envs=a.num_envs, n_head=a.n_head, n_block=N_BLOCK,
                               device=torch.cuda.get_device_name(0), **res))
        print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
