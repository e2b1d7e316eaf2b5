"""Acting-step, update-step and retention-kernel times of the memoryless Sable system (ff_sable) on the bench's headline shape: CoordSum-4ag,
16 384 envs, 128-step rollout, 4 epochs x 2 minibatches, configs/network/ff_retention.yaml defaults (embed_dim 64, 1 head, 1 block).

    python scripts/ff_sable_timing.py --what act          # one acting step both ways, one child process each: --fused 0 (SableGuider.act, the
                                                          # kernel-by-kernel chain on team kernels) and --fused 1 (act_team_fused: magpo_ff_sable_act)
    python scripts/ff_sable_timing.py --what act --fused 1 --num-envs 4096     # one of them, in this process
    python scripts/ff_sable_timing.py --what act --shape 8x15                  # 8 agents, 15 actions, two blocks
    python scripts/ff_sable_timing.py --what update --fused 0|1                # one ff_sable update step
    python scripts/ff_sable_timing.py --what rec-update   # the same update step of rec_sable, for scale
    python scripts/ff_sable_timing.py --what kernels      # team kernels against the chunk kernels run as T = 1 sequences, 65 536 teams of 4
    python scripts/ff_sable_timing.py --what all --out profiles/ff_sable_step_time.json   # all of the above, one child process each

Each measurement is its own process under its own time limit.  HIP events after warm-up: the acting step and the kernels are medians over
--steps launches, the update steps one event pair per step as in bench.py (two untimed set-up steps for workspaces and the rollout graph
capture, then --warmup steps).  HBM bytes of the kernels are the algorithmic count (operands read once, results written once, plus the
chunk kernels' chunk-entry state tile per sequence), not a counter.  Prints one JSON line per measurement.
"""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from magpo_amd.learner import CoordSumConfig, SystemConfig, host_split, prng_key  # noqa: E402

CFG = dict(num_agents=4, num_actions=20, time_limit=100, maxval=60)
WORKLOAD = "coordsum-4ag ff_sable"


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


SHAPES = {"4ag": (CFG, 1), "8x15": (dict(num_agents=8, num_actions=15, time_limit=100, maxval=100), 2)}   # env, n_block


def learner(N, rec, fused=None, shape="4ag"):
    cfg, nb = SHAPES[shape]
    if rec:
        from magpo_amd.sable_learner import SableLearner
        l = SableLearner(CoordSumConfig(**cfg), N, SystemConfig(), "cuda", net_seed=0, n_block=nb)
    else:
        from magpo_amd.ff_sable_learner import FfSableLearner
        from magpo_amd.tuning import Tuning
        t = Tuning.from_env()
        if fused is not None:
            t.ff_sable_fused_act = bool(fused)
        l = FfSableLearner(CoordSumConfig(**cfg), N, SystemConfig(), "cuda", net_seed=0, n_block=nb, tuning=t)
    l.setup(host_split(prng_key(42), 3)[0])
    return l


def time_act(N, steps, warmup, fused, shape):
    """One acting step as the rollout makes it: the learner's action-select function (Tuning.ff_sable_fused_act: magpo_ff_sable_act, or the
    chain SableGuider.act)."""
    l = learner(N, False, fused, shape)
    g, tr = l.groups[0], l.groups[0].traj
    l._rollout_keys(g)
    obs = l._net_view(tr["obs"][0])
    act = l.sable_action_select_fn
    us, med = _median_us(lambda: act(obs, tr["step_count"][0], None, g.keys_host[0], tr["action"][0], tr["log_prob"][0], tr["value"][0]),
                         steps, warmup)
    return dict(shape=shape, fused_act=bool(l.tuning.ff_sable_fused_act), method=act.__name__, us_per_step=[round(x, 1) for x in us[:8]], median_us=med)


def time_update(N, steps, warmup, rec, fused=None, shape="4ag"):
    l = learner(N, rec, fused, shape)
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
    return dict(system="rec_sable" if rec else "ff_sable", shape=shape, fused_act=None if rec else bool(l.tuning.ff_sable_fused_act), ms_per_update_step=[round(x, 2) for x in ms], median_ms=round(med, 2),
                env_steps_per_second=round(l.T * N / (med * 1e-3)), graph=l.groups[0].graph is not None,
                peak_hbm_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))


def time_kernels(nteams, A, steps, warmup):
    from magpo_amd._lib import lib
    L, hs, R = lib(), 64, nteams * A
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v, dr = (torch.randn(R, hs, device="cuda", generator=g) for _ in range(4))
    r, dq, dk, dv = (torch.empty(R, hs, device="cuda") for _ in range(4))
    nch = L.call("magpo_retention_num_chunks", 1, A, 0)
    states = torch.zeros(nteams, nch, 64, 64, device="cuda")
    dones = torch.zeros(nteams, 1, dtype=torch.uint8, device="cuda")
    tile = R * hs * 4
    runs = {
        "team_fwd": (lambda: L.call("magpo_team_retention_fwd", q, hs, k, hs, v, hs, r, hs, nteams, A, A, 0, 1, hs, None, 0, None, None, 0, st), 4 * tile),
        "chunk_fwd": (lambda: L.call("magpo_retention_chunk_fwd", q, hs, k, hs, v, hs, r, hs, None, None, dones, states, None, nteams, 1, A, 1, 1.0, hs, None,
                                     0, st), 4 * tile + states.numel() * 4),
        "team_bwd": (lambda: L.call("magpo_team_retention_bwd", q, hs, k, hs, v, hs, dr, hs, dq, hs, dk, hs, dv, hs, nteams, A, 1, hs, st), 7 * tile),
        "chunk_bwd": (lambda: L.call("magpo_retention_chunk_bwd", q, hs, k, hs, v, hs, dr, hs, dq, hs, dk, hs, dv, hs, dones, states, nteams, 1, A, 1, 1.0,
                                     hs, None, 0, st), 7 * tile + states.numel() * 4),
    }
    out = {}
    for name, (fn, nbytes) in runs.items():
        _, med = _median_us(fn, steps, warmup)
        out[name] = dict(median_us=med, hbm_bytes=nbytes, gb_per_s=round(nbytes / (med * 1e-6) / 1e9, 1))
    return dict(nteams=nteams, A=A, hs=hs, masked=1, kernels=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("act", "update", "rec-update", "kernels", "all"), required=True)
    ap.add_argument("--num-envs", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fused", type=int, choices=(0, 1), default=None,
                    help="ff_sable acting step: 1 = magpo_ff_sable_act, 0 = the chain; default: --what act measures both (one child process each), "
                         "update follows the environment (MAGPO_FF_SABLE_FUSED_ACT) or the default")
    ap.add_argument("--shape", choices=sorted(SHAPES), default="4ag", help="4ag: CoordSum-4ag, one block; 8x15: 8 agents, 15 actions, two blocks")
    a = ap.parse_args()
    both = a.what == "act" and a.fused is None
    if a.what == "all" or both:   # one fresh child process per measurement, each under its own time limit
        lines = []
        jobs = [("act", "0"), ("act", "1")] if both else [("act", "0"), ("act", "1"), ("kernels", None), ("update", "0"), ("update", "1"), ("rec-update", None)]
        for what, fused in jobs:
            cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--what", what, "--num-envs", str(a.num_envs),
                   "--shape", a.shape] + ([] if fused is None else ["--fused", fused])
            for opt, val in (("--steps", a.steps), ("--warmup", a.warmup)):
                if both and val is not None:
                    cmd += [opt, str(val)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:   # nothing more is started on the GPU after a failed measurement
                sys.exit(f"{what} failed ({r.returncode}):\n{r.stderr[-2000:]}")
            lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(lines[-1]), flush=True)
        text = json.dumps(dict(workload=WORKLOAD, num_envs=a.num_envs, measurements=lines), indent=1)
    else:
        if a.what == "act":
            res = time_act(a.num_envs, a.steps or 100, 10 if a.warmup is None else a.warmup, a.fused, a.shape)
        elif a.what == "kernels":
            res = time_kernels(65536, 4, a.steps or 100, 10 if a.warmup is None else a.warmup)
        else:
            res = time_update(a.num_envs, a.steps or 3, 1 if a.warmup is None else a.warmup, a.what == "rec-update", a.fused, a.shape)
        text = json.dumps(dict(workload=WORKLOAD, what=a.what, num_envs=a.num_envs, device=torch.cuda.get_device_name(0), **res))
        print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
