"""CPU restatement of the guider-only Sable system (mava/systems/sable/anakin/rec_sable.py), for the tests only: the PPO loss of
magpo_ppo_loss_fwd_bwd with its case builders, the learner of rec_sable.py:65-317 and the evaluator act function of :498-513.  Built on
oracle.networks / oracle.prng / oracle.learner (calculate_gae, clip_adam_step) and the oracle env modules; the product never imports it."""
import math

import numpy as np
import torch

from oracle import coordsum as cs
from oracle import learner as olearn
from oracle import networks as nets
from oracle import prng
from tests import kernel_refs as kr

SYSC = kr.SYSC
KINK = kr.KINK
PPO_LOSS_NAMES = ("total", "actor_loss", "entropy", "value_loss")   # order of k_ppo_loss_final


# ----------------------------------------------------------------------------- PPO loss (rec_sable.py:177-226)
def ppo_case(R, K, seed, mask_p=None, one_legal=0.0):
    """fp32 inputs of one magpo_ppo_loss_fwd_bwd case: kr.loss_case without its actor logits (logits N(0, 0.7), value within 0.3 of the
    old value, old log-prob = the fp64 log-prob + N(0, 0.1), illegal logits 1e4)."""
    c = kr.loss_case(R, K, seed, mask_p=mask_p, one_legal=one_legal)
    c.pop("al")
    return c


def ppo_loss_ref(c, dtype=torch.float64):
    """The loss of rec_sable.py:177-226 on the case in ``dtype``, gradients by autograd.  Returns loss [4] (PPO_LOSS_NAMES), dl [R, K],
    dv [R] and per row: ratio, vd = value - old value, e1 / e2 (the two value-loss branches), A_ (normalised advantage), p / lp [R, K]
    (masked softmax and its log), ent [R]."""
    eps = SYSC.clip_eps
    gl, v = (c[n].to(dtype).requires_grad_(True) for n in ("gl", "value"))
    legal, action = c["legal"], c["action"]
    lp = nets.masked_log_softmax(gl, legal)
    logp = lp.gather(1, action[:, None])[:, 0]
    p = lp.exp()
    ent = -torch.where(p == 0, torch.zeros_like(p), p * lp).sum(-1)
    old, adv, vold, tgt = (c[n].to(dtype) for n in ("old", "adv", "vold", "tgt"))
    ratio = torch.exp(logp - old)
    A_ = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
    actor = -torch.minimum(ratio * A_, torch.clamp(ratio, 1.0 - eps, 1.0 + eps) * A_).mean()
    entropy = ent.mean()
    vcl = vold + (v - vold).clamp(-eps, eps)
    e1, e2 = (v - tgt) ** 2, (vcl - tgt) ** 2
    vl = 0.5 * torch.maximum(e1, e2).mean()
    total = actor - SYSC.ent_coef * entropy + SYSC.vf_coef * vl
    dl, dv = torch.autograd.grad(total, [gl, v])
    out = dict(loss=torch.stack([total, actor, entropy, vl]), dl=dl, dv=dv, ratio=ratio, vd=v - vold, e1=e1, e2=e2, A_=A_, p=p, lp=lp, ent=ent,
               vcl=vcl)
    return {k: t.detach() for k, t in out.items()}


def ppo_near_kink(ref, m=KINK):
    """Rows [R] of the fp64 reference within m of a kink: the ratio at 1 +- clip_eps, the value difference at +- clip_eps, and equal
    value-loss branches of a clipped value."""
    eps = SYSC.clip_eps
    r = ref["ratio"]
    near = ((r - (1 - eps)).abs() < m) | ((r - (1 + eps)).abs() < m) | ((ref["vd"].abs() - eps).abs() < m)
    return near | ((ref["vd"].abs() > eps) & ((ref["e1"] - ref["e2"]).abs() < m))


def ppo_kink_case(seed=5, R=256, K=5):
    """A case with rows ON every kink, as close as fp32 inputs can put them: 64 rows with ratio = 1 + eps and 64 with 1 - eps (old
    log-prob = fp32(log-prob - log(1 +- eps))), 32 rows with value - old value = +eps and 32 with -eps exactly (old value 0, value =
    +-float32(eps)), 32 rows whose clipped and unclipped value losses are equal (target midway between the value and its clipped copy).
    Returns (case, row groups)."""
    eps = SYSC.clip_eps
    c = ppo_case(R, K, seed, mask_p=0.7)
    lp = nets.masked_log_softmax(c["gl"].double(), c["legal"]).gather(1, c["action"][:, None])[:, 0]
    c["old"][0:64] = (lp[0:64] - math.log(1 + eps)).float()
    c["old"][64:128] = (lp[64:128] - math.log(1 - eps)).float()
    e32 = torch.tensor(eps, dtype=torch.float32)
    c["vold"][128:224] = 0.0
    c["value"][128:160] = e32
    c["value"][160:192] = -e32
    c["value"][192:224] = 0.5
    c["tgt"][192:224] = ((0.5 + e32.double()) / 2).float()
    return c, dict(ratio_hi=slice(0, 64), ratio_lo=slice(64, 128), v_hi=slice(128, 160), v_lo=slice(160, 192), v_equal=slice(192, 224))


def ppo_kink_candidates(c, ref):
    """The one-sided gradients a kernel may produce for a row on a kink.  dl candidates [3, R, K]: the surrogate's logit gradient with
    the weight of the unclipped branch at 1, 1/2 and 0 (plus the entropy term, which has no kink); dv candidates [6, R]: the value-loss
    derivative taken from the unclipped branch, the clipped branch on its open side, the clipped branch on its flat side, and their
    pairwise means."""
    R = c["R"]
    onehot = torch.nn.functional.one_hot(c["action"], c["K"]).double()
    p, lp, ent = ref["p"], ref["lp"], ref["ent"]
    ent_term = SYSC.ent_coef * torch.where(p == 0, torch.zeros_like(p), p * (lp + ent[:, None]))
    pg = -(ref["ratio"] * ref["A_"])[:, None] * (onehot - p)
    dl = torch.stack([(w * pg + ent_term) / R for w in (1.0, 0.5, 0.0)])
    dl = torch.where(c["legal"][None], dl, torch.zeros_like(dl))
    v, tgt = c["value"].double(), c["tgt"].double()
    g1, gc, z = 2 * (v - tgt), 2 * (ref["vcl"] - tgt), torch.zeros(R, dtype=torch.float64)
    dv = torch.stack([g1, gc, z, 0.5 * (g1 + gc), 0.5 * g1, 0.5 * gc]) * (0.5 * SYSC.vf_coef / R)
    return dl, dv


# the case matrix of tests/test_sable_loss_gpu.py: R around the 256-thread block (16 rows) and grid edges x K x mask x strides
PPO_R, PPO_K = (1, 255, 256, 257, 1500), (2, 5, 20, 64)
PPO_MATRIX = [(R, K, masked, strides) for R in PPO_R for K in PPO_K for masked in (False, True) for strides in ("s64", "tight")]
PPO_SEED_BUMP = {}      # case index -> seed increment, for a case whose fp64 reference has more than 2 % of its rows near a kink
_ppo_cache = {}


def ppo_strides(kind, K):
    """(ld, lddl): the learner's 64 / 64, or tight: logits rows of exactly K floats, gradient rows of K rounded up to a multiple of 4."""
    return (64, 64) if kind == "s64" else (K, kr.ceil4(K))


def ppo_case_id(i):
    R, K, masked, strides = PPO_MATRIX[i]
    return f"{i}-R{R}-K{K}-{'mask' if masked else 'nomask'}-{strides}"


def ppo_matrix_case(i):
    """(case, fp64 reference, fp32 restatement) of matrix entry i, computed once per process.  Masked cases have 15 % rows with a
    single legal action."""
    if i not in _ppo_cache:
        R, K, masked, strides = PPO_MATRIX[i]
        c = ppo_case(R, K, 3000 + i + PPO_SEED_BUMP.get(i, 0), **(dict(mask_p=0.6, one_legal=0.15) if masked else {}))
        c.update(strides=ppo_strides(strides, K), name=ppo_case_id(i))
        _ppo_cache[i] = (c, ppo_loss_ref(c), ppo_loss_ref(c, torch.float32))
    return _ppo_cache[i]


# ----------------------------------------------------------------------------- learner (rec_sable.py:65-317)
class SableOracleLearner(olearn.OracleLearner):
    """Single-group Sable learner on the CPU: OracleLearner's set-up (PRNG layout of rec_sable.py:423-455 = rec_magpo's), envs,
    optimiser and learning-rate schedule, with the rollout, the minibatches, the loss and the update of rec_sable.py restated."""

    def __init__(self, spec, num_envs, sys, scfg, params, dtype=torch.float32, env=cs):
        super().__init__(spec, num_envs, sys, scfg, params, {}, dtype, env)
        self.opt = self.g_opt

    @torch.no_grad()
    def rollout(self, T=None):
        """_env_step x T (rec_sable.py:86-126), the bootstrap value with its own key (:130-134) and GAE (:136-167)."""
        sys, scfg, spec = self.sys, self.scfg, self.spec
        T = T or sys.rollout_length
        traj = {k: [] for k in ("done", "action", "value", "reward", "log_prob", "obs", "step_count", "mask")}
        metrics = {k: [] for k in ("episode_return", "episode_length", "is_terminal_step")}
        self.prev_sable_hs = tuple(h.clone() for h in self.sable_hs)                         # :121
        for _ in range(T):
            ks = prng.split(self.key, 2)                                                     # :93
            self.key, policy_key = ks[0], ks[1]
            ob = self.timestep["observation"]
            obs, mask, sc = torch.from_numpy(ob["agents_view"]), torch.from_numpy(ob["action_mask"]), torch.from_numpy(ob["step_count"])
            action, logp, value, new_hs, _ = nets.sable_get_actions(self.gp, scfg, obs, mask, sc, self.sable_hs, policy_key)
            prev_done = self.dones.copy()                                                    # last_timestep.last() per agent (:112)
            self.env_state, self.timestep = self.env.step(spec, self.env_state, action.numpy(), auto_reset=True)
            done = self.timestep["step_type"] == cs.STEP_LAST
            dmask = torch.from_numpy(done)[:, None, None, None, None]
            self.sable_hs = tuple(torch.where(dmask, torch.zeros_like(h), h) for h in new_hs)   # :108-110
            self.dones = np.repeat(done[:, None], spec.num_agents, axis=1)
            for k, x in (("done", torch.from_numpy(prev_done)), ("action", action), ("value", value),
                         ("reward", torch.from_numpy(self.timestep["reward"]).to(self.dtype)), ("log_prob", logp), ("obs", obs), ("step_count", sc),
                         ("mask", mask)):
                traj[k].append(x)
            for k in metrics:
                metrics[k].append(self.timestep["episode_metrics"][k].copy())
        ks = prng.split(self.key, 2)                                                         # :130
        self.key, last_val_key = ks[0], ks[1]
        ob = self.timestep["observation"]
        _, _, last_val, _, _ = nets.sable_get_actions(self.gp, scfg, torch.from_numpy(ob["agents_view"]), torch.from_numpy(ob["action_mask"]),
                                                      torch.from_numpy(ob["step_count"]), self.sable_hs, last_val_key)
        traj = {k: torch.stack(v, dim=0) for k, v in traj.items()}
        traj["adv"], traj["targets"] = olearn.calculate_gae(traj["reward"], traj["value"], traj["done"], last_val, torch.from_numpy(self.dones),
                                                            sys.gamma, sys.gae_lambda)
        self.traj, self.last_val = traj, last_val
        return {k: np.stack(v, axis=0) for k, v in metrics.items()}

    def make_minibatches(self, batch_perm, agent_perm, prev_hstates=None):
        """rec_sable.py:266-289: take the env axis, take the agent axis, concatenate time and agents, split; the hidden states are taken
        by the batch permutation alone and carried SHUFFLED into the next epoch (:272, :298 -- quirk B19)."""
        M, N = self.sys.num_minibatches, self.N
        bp, apm = torch.from_numpy(batch_perm.astype(np.int64)), torch.from_numpy(agent_perm.astype(np.int64))

        def prep(x):  # (T, N, A, ...) -> (M, N / M, T * A, ...)
            x = x.index_select(1, bp).index_select(2, apm).transpose(0, 1)
            x = x.reshape(N, x.shape[1] * x.shape[2], *x.shape[3:])
            return x.reshape(M, N // M, *x.shape[1:])
        fields = {k: prep(self.traj[k]) for k in ("done", "action", "value", "log_prob", "obs", "step_count", "mask", "adv", "targets")}
        carried = self.prev_sable_hs if prev_hstates is None else prev_hstates
        self._epoch_prev_hs = tuple(h.index_select(0, bp) for h in carried)
        prev = tuple(h.reshape(M, N // M, *h.shape[1:]) for h in self._epoch_prev_hs)
        return [dict({k: v[m] for k, v in fields.items()}, prev_hs=tuple(h[m] for h in prev)) for m in range(M)]

    def loss(self, params, mb):
        """_loss_fn (rec_sable.py:177-226)."""
        s = self.sys
        value, logp, ent, _ = nets.sable_train(params, self.scfg, mb["obs"], mb["action"], mb["mask"], mb["step_count"], mb["prev_hs"], mb["done"])
        ratio = torch.exp(logp - mb["log_prob"])
        gae = mb["adv"]
        gae = (gae - gae.mean()) / (gae.std(unbiased=False) + 1e-8)
        actor = -torch.minimum(ratio * gae, torch.clamp(ratio, 1.0 - s.clip_eps, 1.0 + s.clip_eps) * gae).mean()
        entropy = ent.mean()
        vclip = mb["value"] + (value - mb["value"]).clamp(-s.clip_eps, s.clip_eps)
        vl = 0.5 * torch.maximum((value - mb["targets"]) ** 2, (vclip - mb["targets"]) ** 2).mean()
        total = actor - s.ent_coef * entropy + s.vf_coef * vl
        return total, dict(total_loss=total, actor_loss=actor, entropy=entropy, value_loss=vl), dict(value=value, log_prob=logp)

    def minibatch_grads(self, mb):
        p = {k: v.detach().clone().requires_grad_(True) for k, v in self.gp.items()}
        total, info, inter = self.loss(p, mb)
        grads = torch.autograd.grad(total, list(p.values()), allow_unused=True)
        gg = {k: (g if g is not None else torch.zeros_like(v)) for (k, v), g in zip(p.items(), grads)}
        return gg, {k: float(v.detach()) for k, v in info.items()}, {k: v.detach() for k, v in inter.items()}

    def update(self, grad_hook=None):
        """_update_epoch x ppo_epochs (rec_sable.py:169-306)."""
        s, infos, prev_hstates = self.sys, [], None
        for _ in range(s.ppo_epochs):
            ks = prng.split(self.key, 4)                                                     # :263
            self.key, kb, ka, ke = ks[0], ks[1], ks[2], ks[3]
            mbs = self.make_minibatches(prng.permutation(kb, self.N), prng.permutation(ka, self.spec.num_agents), prev_hstates)
            prev_hstates = self._epoch_prev_hs
            for mb in mbs:
                ke = prng.split(ke, 2)[0]                                                    # :229, unused for discrete actions
                gg, info, _ = self.minibatch_grads(mb)
                if grad_hook is not None:
                    gg = grad_hook(gg)
                self.gp, self.g_opt, _ = olearn.clip_adam_step(self.gp, gg, self.g_opt, self._lr(self.g_opt["count"]), s.max_grad_norm)
                self.opt = self.g_opt
                infos.append(info)
        return infos


def gae_quadratic(reward, value, done, last_val, last_done, gamma, lam):
    """GAE written out as the O(T^2) double sum, independent of the backward recurrence: A_t = sum_{l >= 0} (gamma lambda)^l
    [prod_{j < l} (1 - d_{t+j+1})] delta_{t+l}, delta_t = r_t + gamma V_{t+1} (1 - d_{t+1}) - V_t, d_t = "the observation of step t starts
    an episode" (d_T = last_done)."""
    T = reward.shape[0]
    d = torch.cat([done.to(value.dtype), last_done.to(value.dtype)[None]])
    v = torch.cat([value, last_val[None]])
    adv = torch.zeros_like(value)
    for t in range(T):
        live = torch.ones_like(last_val)
        for l in range(T - t):
            u = t + l
            nd = 1 - d[u + 1]
            adv[t] += (gamma * lam) ** l * live * (reward[u] + gamma * v[u + 1] * nd - v[u])
            live = live * nd
    return adv, adv + value


def compose_b19(perms):
    """Row of the ORIGINAL rollout-start states that sequence i of epoch e trains on when every epoch shuffles the already shuffled
    states (rec_sable.py:272,298): hs_idx_e = hs_idx_{e-1}[perm_e], hs_idx_0 = perm_0."""
    out, idx = [], None
    for p in perms:
        idx = p.copy() if idx is None else idx[p]
        out.append(idx)
    return out


# ----------------------------------------------------------------------------- evaluator with the Sable act function (rec_sable.py:498-513)
@torch.no_grad()
def evaluate_sable(spec, scfg, params, key, num_envs, eval_episodes, dtype=torch.float32, env=cs):
    """oracle.evaluator.evaluate with make_rec_sable_act_fn in place of the recurrent-actor act function: the action is sampled by
    get_actions from the step's act key, the hidden states are carried as they come back (no reset at an episode end), greedy does not
    exist.  Returns the flattened per-episode return and length arrays."""
    from oracle.evaluator import get_num_eval_envs
    n = get_num_eval_envs(num_envs, eval_episodes)
    loops = math.ceil(eval_episodes / n)
    params = {k: v.to(dtype) for k, v in params.items()}
    rets, lens = [], []
    key = np.asarray(key, np.uint32)
    for _ in range(loops):
        ks = prng.split(key, 2)
        key, reset_key = ks[0], ks[1]
        state, ts = env.reset(spec, prng.split(reset_key, n))
        hs = nets.init_sable_hstates(n, scfg, dtype)
        step_key = key
        last_t, m_ret, m_len = [], [], []
        for _t in range(spec.time_limit + 1):
            ks = prng.split(step_key, 2)
            step_key, act_key = ks[0], ks[1]
            ob = ts["observation"]
            action, _, _, hs, _ = nets.sable_get_actions(params, scfg, torch.from_numpy(ob["agents_view"]), torch.from_numpy(ob["action_mask"]),
                                                         torch.from_numpy(ob["step_count"]), hs, act_key)
            state, ts = env.step(spec, state, action.numpy(), auto_reset=False)
            last_t.append(ts["step_type"] == cs.STEP_LAST)
            m_ret.append(ts["episode_metrics"]["episode_return"].copy())
            m_len.append(ts["episode_metrics"]["episode_length"].copy())
        done_idx = np.argmax(np.stack(last_t), axis=0)
        ar = np.arange(n)
        rets.append(np.stack(m_ret)[done_idx, ar])
        lens.append(np.stack(m_len)[done_idx, ar])
    return {"episode_return": np.concatenate(rets), "episode_length": np.concatenate(lens)}
