"""The parity cases of the one-launch ff_sable acting step (tests/test_ff_sable_act_gpu.py) and their fp64 reference, shared with the CPU
module that qualifies the seeds (tests/test_ff_sable_act_cases.py).  The product never imports it.

A case fixes the network shape, the batch and the inputs; ``make_inputs`` builds parameters (oracle.networks.init_guider_params, with the
norm scales, GroupNorm affine and biases moved off their 1 / 0 init so that a wrong index shows, and the logit head scaled up so that the
policy has a visible spread), observations (random, env 0 agent 0 all-zero), the action mask and the sample key; ``reference`` is
``oracle.networks.sable_get_actions`` on zero hidden states with the ff configuration, in fp64.

ENVS = 32 is what one workgroup of magpo_ff_sable_act carries; every wave of it works on all 32 rows, so the env counts that matter are
1, ENVS - 1, ENVS, ENVS + 1 and a count with a partly filled second tile."""
import numpy as np
import torch

from oracle import networks as nets
from oracle import prng
from tests import ff_sable_ref as fs

ENVS = 32
SEED = 7

# id -> A, N, n_head, n_block, embed_dim, K, F, obs_ld, mask, act_scale (dec.act.kernel multiplier; > 1: the autoregression case)
CASES = {
    "A4-N33-64.1.1-K10-F5": dict(A=4, N=ENVS + 1, nh=1, nb=1, E=64, K=10, F=5, ld=5, mask=False),
    "A1-N1-64.1.1-K2-F3": dict(A=1, N=1, nh=1, nb=1, E=64, K=2, F=3, ld=3, mask=False),
    "A2-N31-64.2.2-K31-F3-ld7-mask": dict(A=2, N=ENVS - 1, nh=2, nb=2, E=64, K=31, F=3, ld=7, mask=True),
    "A3-N32-64.4.1-K6-F128-mask": dict(A=3, N=ENVS, nh=4, nb=1, E=64, K=6, F=128, ld=128, mask=True),
    "A5-N45-64.1.4-K5-F9": dict(A=5, N=ENVS + 13, nh=1, nb=4, E=64, K=5, F=9, ld=9, mask=False),
    "A8-N33-32.2.2-K7-F12-mask": dict(A=8, N=ENVS + 1, nh=2, nb=2, E=32, K=7, F=12, ld=12, mask=True),
    "A4-N8-16.1.1-K4-F6-ld8": dict(A=4, N=8, nh=1, nb=1, E=16, K=4, F=6, ld=8, mask=False),
    "A3-N5-64.1.1-K8-F4-autoregressive": dict(A=3, N=5, nh=1, nb=1, E=64, K=8, F=4, ld=4, mask=False, act_scale=8.0),
}
SEED_BUMP = {}   # case id -> seed increment, where the fp64 reference has a Gumbel near-tie at SEED (tests/test_ff_sable_act_cases.py)


def make_inputs(cid):
    """dict(cfg, gp (fp32 parameters), obs [N, A, F] fp32, mask [N, A, K] bool, key [2] uint32) of case ``cid``."""
    c = CASES[cid]
    A, N, K, F = c["A"], c["N"], c["K"], c["F"]
    seed = SEED + SEED_BUMP.get(cid, 0) + 1000 * sorted(CASES).index(cid)
    gen = torch.Generator().manual_seed(seed)
    gp = nets.init_guider_params(seed, c["E"], F, K, nh=c["nh"], nb=c["nb"])
    for n in gp:
        if n.endswith("scale"):
            gp[n] = gp[n] * (1.0 + 0.2 * (torch.rand(gp[n].shape, generator=gen) - 0.5))
        elif n.endswith("bias"):
            gp[n] = gp[n] + 0.1 * (torch.rand(gp[n].shape, generator=gen) - 0.5)
    gp["dec.head.dense1.kernel"] = gp["dec.head.dense1.kernel"] * 30.0
    if c.get("act_scale", 1.0) != 1.0:   # the action embedding is RMS-normalised and the retention outputs GroupNorm-ed, so the previous action
        gp["dec.act.kernel"] = gp["dec.act.kernel"] * c["act_scale"]                     # reaches the logits through the decoder's W_o: they grow with it
        for n in gp:
            if n.startswith("dec.") and n.endswith(".w_o"):
                gp[n] = gp[n] * c["act_scale"]
    obs = torch.randn(N, A, F, generator=gen)
    obs[0, 0] = 0.0
    mask = torch.ones(N, A, K, dtype=torch.bool)
    if c["mask"]:
        mask = torch.rand(N, A, K, generator=gen) < 0.6
        mask[..., 0] |= ~mask.any(-1)                 # at least one legal action
        only = torch.zeros(K, dtype=torch.bool)
        only[K - 1] = True
        mask[0, A - 1] = only                         # rows with exactly one legal action: the action is forced, its log-prob 0
        mask[N - 1, 0] = only
    key = prng.split(prng.prng_key(seed), 2)[1]
    return dict(cfg=fs.ff_cfg(A, K, F, c["E"], c["nh"], c["nb"]), gp=gp, obs=obs, mask=mask, key=key)


def sample_keys(key, A):
    """The A per-agent sample keys of one acting step: key, sample_key = split(key) per agent (decode.py:141)."""
    keys, k = np.zeros((A, 2), np.uint32), np.asarray(key, np.uint32)
    for i in range(A):
        ks = prng.split(k, 2)
        k, keys[i] = ks[0], ks[1]
    return keys


_REF = {}


def reference(cid):
    """(action [N, A] int32, logp, value (fp64), normalised log-probs [N, A, K]) of the fp64 restatement; computed once per case."""
    if cid not in _REF:
        x = make_inputs(cid)
        cfg, N = x["cfg"], x["obs"].shape[0]
        p64 = {k: v.double() for k, v in x["gp"].items()}
        sc = torch.zeros(N, cfg.A, dtype=torch.int32)
        with torch.no_grad():
            a, lp, v, _, lp_all = nets.sable_get_actions(p64, cfg, x["obs"].double(), x["mask"], sc, nets.init_sable_hstates(N, cfg, torch.float64), x["key"])
        _REF[cid] = (a, lp, v, lp_all)
    return _REF[cid]
