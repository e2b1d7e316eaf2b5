"""CPU restatement of the Multi-Agent Transformer system (mava/systems/mat/anakin/mat.py), for the tests only: softmax attention over
the agents of one time step (mava/networks/attention.py:50-77), flax LayerNorm, the blocks, encoder and decoder of
mava/networks/mat_network.py:35-279, discrete_parallel_act / discrete_autoregressive_act (mava/networks/utils/mat/decode.py:33-58, 90-124)
on the restated PRNG of oracle/prng.py, the initialiser, and the learner of mat.py:56-283 on tests/ff_sable_ref.py (the two learners share
everything around the network: mat.py:82-283 against ff_sable.py:83-283).  Every function works in the dtype of its inputs, so the same
text is the fp64 reference and the fp32 yardstick.  The product never imports it.

Parameter names are the flax module paths joined by dots ("encoder.blocks.layers_0.attn.key.kernel"): nn.Sequential children are
layers_<i> (mat_network.py:39-45, 78-102, 151-160, 186-193), the decoder blocks carry their explicit names (:182), Decoder.obs_encoder
(:170-176) is never called and has no parameters."""
import math

import numpy as np
import torch

from oracle import coordsum as cs
from oracle import networks as nets
from oracle import prng
from tests import ff_sable_ref as fs

FMIN = float(np.finfo(np.float32).min)
LN_EPS = 1e-6   # flax.linen.LayerNorm default epsilon


# ----------------------------------------------------------------------------- attention between the projections (attention.py:59-72)
def attention(q, k, v, masked):
    """q, k, v [teams, A, hs] (one head) -> (y [teams, A, hs], lse [teams, A]): att = q k^T * (1 / sqrt(hs)) (:60), masked pairs set to
    finfo(float32).min (:63-68: their weight underflows to exactly 0), softmax over j (:70), y = att v (:72)."""
    A, hs = q.shape[1], q.shape[2]
    att = (q @ k.transpose(1, 2)) * (1.0 / math.sqrt(hs))
    if masked:
        att = torch.where(torch.tril(torch.ones(A, A, dtype=torch.bool)), att, torch.full_like(att, FMIN))
    return torch.softmax(att, dim=-1) @ v, torch.logsumexp(att, dim=-1)


def attention_bwd(q, k, v, dy, masked):
    """(dq, dk, dv) of sum(y * dy) by autograd."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    y, _ = attention(q, k, v, masked)
    return torch.autograd.grad((y * dy).sum(), [q, k, v])


def attention_partial(q, k, v, masked, ntok, ret_from):
    """Rows ret_from <= i < ntok of every team from the k / v rows j < ntok (the acting form)."""
    y, lse = attention(q[:, :ntok], k[:, :ntok], v[:, :ntok], masked)
    return y[:, ret_from:ntok], lse[:, ret_from:ntok]


def layer_norm(x, scale, bias):
    """flax.linen.LayerNorm (epsilon 1e-6, scale and bias) over the last axis."""
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) * torch.rsqrt(var + LN_EPS) * scale + bias


def resln(a, y, scale, bias, act=0):
    """What magpo_resln_fwd evaluates: LayerNorm(a + y), or with act 2 LayerNorm(gelu(y))."""
    x = nets.gelu(y) if act == 2 else (y if a is None else a + y)
    return layer_norm(x, scale, bias)


# ----------------------------------------------------------------------------- parameters
class MatCfg:
    def __init__(self, n_agents, action_dim, obs_dim, embed_dim=64, n_head=1, n_block=1):
        self.A, self.K, self.F = n_agents, action_dim, obs_dim
        self.E, self.nh, self.nb = embed_dim, n_head, n_block


def _attn_shapes(s, p, E):
    for n in ("key", "query", "value", "proj"):   # attention.py:31-36
        s[p + n + ".kernel"], s[p + n + ".bias"] = (E, E), (E,)


def _ln_shapes(s, p, W):
    s[p + "scale"], s[p + "bias"] = (W,), (W,)


def param_shapes(E, F, K, nb):
    """name -> shape, in creation order (mat_network.py:48-206)."""
    s = {}
    e = "encoder."
    _ln_shapes(s, e + "obs_encoder.layers_0.", F)                                            # :80
    s[e + "obs_encoder.layers_1.kernel"], s[e + "obs_encoder.layers_1.bias"] = (F, E), (E,)   # :81
    _ln_shapes(s, e + "ln.", E)                                                              # :85
    for b in range(nb):                                                                      # :86-94, EncodeBlock :53-62
        p = e + f"blocks.layers_{b}."
        _ln_shapes(s, p + "ln1.", E); _ln_shapes(s, p + "ln2.", E)
        _attn_shapes(s, p + "attn.", E)
        for l in ("layers_0", "layers_2"):                                                   # _make_mlp :39-45
            s[p + f"mlp.{l}.kernel"], s[p + f"mlp.{l}.bias"] = (E, E), (E,)
    s[e + "head.layers_0.kernel"], s[e + "head.layers_0.bias"] = (E, E), (E,)                 # :95-102
    _ln_shapes(s, e + "head.layers_2.", E)
    s[e + "head.layers_3.kernel"], s[e + "head.layers_3.bias"] = (E, 1), (1,)
    d = "decoder."
    s[d + "action_encoder.layers_0.kernel"] = (K + 1, E)                                     # :150-160: no bias for discrete actions
    _ln_shapes(s, d + "ln.", E)                                                              # :177
    for b in range(nb):                                                                      # :178-185, DecodeBlock :119-132
        p = d + f"cross_attention_block_{b}."
        for n in ("ln1.", "ln2.", "ln3."):
            _ln_shapes(s, p + n, E)
        _attn_shapes(s, p + "attn1.", E); _attn_shapes(s, p + "attn2.", E)
        for l in ("layers_0", "layers_2"):
            s[p + f"mlp.{l}.kernel"], s[p + f"mlp.{l}.bias"] = (E, E), (E,)
    s[d + "head.layers_0.kernel"], s[d + "head.layers_0.bias"] = (E, E), (E,)                 # :186-193
    _ln_shapes(s, d + "head.layers_2.", E)
    s[d + "head.layers_3.kernel"], s[d + "head.layers_3.bias"] = (E, K), (K,)
    return s


def kernel_gain(name):
    """orthogonal(gain) of a Dense kernel: 0.01 for the attention projections (attention.py:31-36), the second MLP layer
    (mat_network.py:43) and the last head layer (:100, :191); sqrt(2) for every other one (:41, :81, :97, :156, :188)."""
    small = any(t in name for t in (".key.", ".query.", ".value.", ".proj.", "mlp.layers_2.", "head.layers_3."))
    return 0.01 if small else math.sqrt(2.0)


def init_params(seed, cfg, dtype=torch.float32, randomize=False):
    """The reference's init distributions from a torch generator; ``randomize``: N(0, 0.3) biases and scales 1 + N(0, 0.3), and the 0.01
    kernels at gain 1, so that every term of the network and of its gradient is visibly non-zero."""
    gen = torch.Generator().manual_seed(seed)
    p = {}
    for name, shape in param_shapes(cfg.E, cfg.F, cfg.K, cfg.nb).items():
        if name.endswith("kernel"):
            gain = kernel_gain(name)
            p[name] = nets._orthogonal(gen, shape, 1.0 if randomize and gain == 0.01 else gain, dtype)
        else:
            base = 1.0 if name.endswith("scale") else 0.0
            r = torch.randn(shape, generator=gen, dtype=torch.float64) * 0.3 if randomize else 0.0
            p[name] = (torch.full(shape, base, dtype=torch.float64) + r).to(dtype)
    return p


def init_params_from_key(net_key, cfg, dtype=torch.float32):
    """The parameters flax creates from ``net_key`` (mat.py:353): per-parameter keys from the module path and the per-scope creation counter
    (Dense: kernel 1), orthogonal kernels, ones / zeros for everything else.  PARITY UNPINNED like the other initialisers (oracle/prng.py)."""
    p = {}
    for name, shape in param_shapes(cfg.E, cfg.F, cfg.K, cfg.nb).items():
        if name.endswith("kernel"):
            path = tuple(name.split(".")[:-1])
            p[name] = torch.from_numpy(np.ascontiguousarray(prng.init_orthogonal(prng.flax_param_key(net_key, path, 1), shape, kernel_gain(name)))).to(dtype)
        else:
            p[name] = (torch.ones if name.endswith("scale") else torch.zeros)(shape, dtype=dtype)
    return p


# ----------------------------------------------------------------------------- network (mat_network.py:48-206)
def _dense(p, n, x):
    y = x @ p[n + ".kernel"]
    return y + p[n + ".bias"] if n + ".bias" in p else y


def _ln(p, n, x):
    return layer_norm(x, p[n + ".scale"], p[n + ".bias"])


def self_attention(p, pre, key, value, query, nh, masked):
    """SelfAttention.__call__ (attention.py:42-77) on [B, S, E] inputs."""
    B, S, E = key.shape
    hs = E // nh
    heads = lambda t: t.reshape(B, S, nh, hs).permute(0, 2, 1, 3).reshape(B * nh, S, hs)
    y, _ = attention(heads(_dense(p, pre + "query", query)), heads(_dense(p, pre + "key", key)), heads(_dense(p, pre + "value", value)), masked)
    return _dense(p, pre + "proj", y.reshape(B, nh, S, hs).permute(0, 2, 1, 3).reshape(B, S, E))


def _mlp(p, pre, x):
    return _dense(p, pre + "layers_2", nets.gelu(_dense(p, pre + "layers_0", x)))   # :39-45


def encoder(p, cfg, obs):
    """Encoder.__call__ (:104-111) -> (value [B, A], rep [B, A, E])."""
    x = nets.gelu(_dense(p, "encoder.obs_encoder.layers_1", _ln(p, "encoder.obs_encoder.layers_0", obs)))
    x = _ln(p, "encoder.ln", x)
    for b in range(cfg.nb):   # EncodeBlock.__call__ (:64-67), unmasked
        pre = f"encoder.blocks.layers_{b}."
        x = _ln(p, pre + "ln1", x + self_attention(p, pre + "attn.", x, x, x, cfg.nh, False))
        x = _ln(p, pre + "ln2", x + _mlp(p, pre + "mlp.", x))
    h = _ln(p, "encoder.head.layers_2", nets.gelu(_dense(p, "encoder.head.layers_0", x)))
    return _dense(p, "encoder.head.layers_3", h)[..., 0], x


def decoder(p, cfg, shifted, rep):
    """Decoder.__call__ (:195-206) -> logits [B, A, K]."""
    x = _ln(p, "decoder.ln", nets.gelu(_dense(p, "decoder.action_encoder.layers_0", shifted)))
    for b in range(cfg.nb):   # DecodeBlock.__call__ (:134-138), both attentions masked
        pre = f"decoder.cross_attention_block_{b}."
        x = _ln(p, pre + "ln1", x + self_attention(p, pre + "attn1.", x, x, x, cfg.nh, True))
        x = _ln(p, pre + "ln2", rep + self_attention(p, pre + "attn2.", x, x, rep, cfg.nh, True))
        x = _ln(p, pre + "ln3", x + _mlp(p, pre + "mlp.", x))
    h = _ln(p, "decoder.head.layers_2", nets.gelu(_dense(p, "decoder.head.layers_0", x)))
    return _dense(p, "decoder.head.layers_3", h)


def shifted_actions(action, K, dtype):
    """decode.py:42-45: start token in slot 0 of agent 0, one-hot of agent i - 1's action in slots 1..K of agent i."""
    B, A = action.shape
    sh = torch.zeros(B, A, K + 1, dtype=dtype)
    sh[:, 0, 0] = 1
    sh[:, 1:, 1:] = torch.nn.functional.one_hot(action.long(), K).to(dtype)[:, :-1]
    return sh


def parallel_act(p, cfg, obs, action, mask):
    """MultiAgentTransformer.__call__ (:247-264) with discrete_parallel_act (decode.py:33-58).
    Returns value [B, A], log_prob [B, A], entropy [B, A], the normalised masked log-probs [B, A, K], raw logits."""
    dt = p["encoder.ln.scale"].dtype
    value, rep = encoder(p, cfg, obs.to(dt))
    logits = decoder(p, cfg, shifted_actions(action, cfg.K, dt), rep)
    lp_all = nets.masked_log_softmax(logits, mask)
    logp = torch.gather(lp_all, -1, action.long()[..., None])[..., 0]
    pr = lp_all.exp()
    ent = -torch.where(pr == 0, torch.zeros_like(pr), pr * lp_all).sum(-1)
    return value, logp, ent, lp_all, logits


def autoregressive_act(p, cfg, obs, mask, key, forced_actions=None):
    """MultiAgentTransformer.get_actions (:266-279) with discrete_autoregressive_act (decode.py:90-124): the whole decoder on the shifted
    actions so far, row i of its logits, key, sample_key = split(key), one categorical draw over the (B, K) batch.
    Returns action [B, A] int32, log_prob, value, normalised masked log-probs [B, A, K]."""
    dt = p["encoder.ln.scale"].dtype
    B, A = obs.shape[:2]
    value, rep = encoder(p, cfg, obs.to(dt))
    sh = torch.zeros(B, A, cfg.K + 1, dtype=dt)
    sh[:, 0, 0] = 1
    acts, logps, all_lp = torch.zeros(B, A, dtype=torch.int32), torch.zeros(B, A, dtype=dt), []
    key = np.asarray(key, np.uint32)
    for i in range(A):
        lp = nets.masked_log_softmax(decoder(p, cfg, sh, rep)[:, i], mask[:, i])
        ks = prng.split(key, 2)
        key, sample_key = ks[0], ks[1]
        a = torch.from_numpy(prng.categorical(sample_key, lp.detach().to(torch.float32).numpy())) if forced_actions is None else forced_actions[:, i]
        acts[:, i] = a
        logps[:, i] = torch.gather(lp, -1, a.long()[:, None])[:, 0]
        all_lp.append(lp)
        if i + 1 < A:
            sh[:, i + 1, 1:] = torch.nn.functional.one_hot(a.long(), cfg.K).to(dt)
    return acts, logps, value, torch.stack(all_lp, dim=1)


# ----------------------------------------------------------------------------- learner (mat.py:56-283)
class MatOracleLearner(fs.FfSableOracleLearner):
    """Single-group MAT learner on the CPU: ff_sable's restated learner (same key chain, GAE, permutations and clipped PPO loss: mat.py:82-283
    line for line ff_sable.py:83-283) with the MAT network in the two places a network is called."""

    @torch.no_grad()
    def rollout(self, T=None):
        """_env_step x T (mat.py:82-110), the bootstrap value with its own key (:115-120) and GAE (:122-149)."""
        sys, cfg, spec = self.sys, self.scfg, self.spec
        T = T or sys.rollout_length
        traj = {k: [] for k in ("done", "action", "value", "reward", "log_prob", "obs", "step_count", "mask", "lp_all")}
        metrics = {k: [] for k in ("episode_return", "episode_length", "is_terminal_step")}
        self.sample_keys = []
        obs_of = lambda ob: (torch.from_numpy(ob["agents_view"]), torch.from_numpy(ob["action_mask"]), torch.from_numpy(ob["step_count"]))
        for _ in range(T):
            ks = prng.split(self.key, 2)                                                     # :89
            self.key, policy_key = ks[0], ks[1]
            obs, mask, sc = obs_of(self.timestep["observation"])
            action, logp, value, lp_all = autoregressive_act(self.gp, cfg, obs, mask, policy_key)   # :90-94
            self.env_state, self.timestep = self.env.step(spec, self.env_state, action.numpy(), auto_reset=True)   # :96
            done = self.timestep["step_type"] == cs.STEP_LAST
            self.dones = np.repeat(done[:, None], spec.num_agents, axis=1)                   # :98
            for k, x in (("done", torch.from_numpy(self.dones.copy())), ("action", action), ("value", value),
                         ("reward", torch.from_numpy(self.timestep["reward"]).to(self.dtype)), ("log_prob", logp), ("obs", obs), ("step_count", sc),
                         ("mask", mask), ("lp_all", lp_all)):
                traj[k].append(x)
            self.sample_keys.append(policy_key)
            for k in metrics:
                metrics[k].append(self.timestep["episode_metrics"][k].copy())
        ks = prng.split(self.key, 2)                                                         # :115
        self.key, last_val_key = ks[0], ks[1]
        obs, mask, _ = obs_of(self.timestep["observation"])
        _, _, last_val, _ = autoregressive_act(self.gp, cfg, obs, mask, last_val_key)
        traj = {k: torch.stack(v, dim=0) for k, v in traj.items()}
        traj["adv"], traj["targets"] = fs.ff_gae(traj["reward"], traj["value"], traj["done"], last_val, sys.gamma, sys.gae_lambda)
        self.traj, self.last_val = traj, last_val
        return {k: np.stack(v, axis=0) for k, v in metrics.items()}

    def zero_hs(self, B):
        return ()

    def loss(self, params, mb):
        """_loss_fn (mat.py:159-205)."""
        s = self.sys
        value, logp, ent, _, _ = parallel_act(params, self.scfg, mb["obs"], mb["action"], mb["mask"])
        ratio = torch.exp(logp - mb["log_prob"])
        gae = mb["adv"]
        gae = (gae - gae.mean()) / (gae.std(unbiased=False) + 1e-8)
        actor = -torch.minimum(ratio * gae, torch.clamp(ratio, 1.0 - s.clip_eps, 1.0 + s.clip_eps) * gae).mean()
        entropy = ent.mean()
        vclip = mb["value"] + (value - mb["value"]).clamp(-s.clip_eps, s.clip_eps)
        vl = 0.5 * torch.maximum((value - mb["targets"]) ** 2, (vclip - mb["targets"]) ** 2).mean()
        total = actor - s.ent_coef * entropy + s.vf_coef * vl
        return total, dict(total_loss=total, actor_loss=actor, entropy=entropy, value_loss=vl), dict(value=value, log_prob=logp)


# ----------------------------------------------------------------------------- the parity cases of tests/test_mat_learner_gpu.py
# (env, env args, N, T, n_block, n_head); coordsum args = (A, K, time_limit, maxval), lbf = LbfSpec's
PARITY_CASES = [
    ("coordsum", (3, 10, 6, 30), 8, 8, 2, 2),
    ("lbf", (8, 8, 2, 2, 2, True, 6), 8, 8, 2, 2),     # a masked env: one rollout and one update
]
PARITY_SEED = 42
PARITY_SEED_BUMP = {}   # case id -> seed increment, where the fp64 restatement has a Gumbel near-tie at PARITY_SEED (tests/test_mat_system.py)
PARITY_EPOCHS, PARITY_MINIBATCHES = 2, 2


def case_id(c):
    env, args, N, T, nb, nh = c
    return f"{env}-A{args[0] if env == 'coordsum' else args[2]}-{nh}.{nb}"


def make_case(c, dtype=torch.float32):
    """(oracle learner after setup, env config of the product, dict of what the device learner needs) of one parity case.  The parameters
    are init_params(randomize=True): at the reference's init the 0.01-gain kernels make every attention and MLP branch vanish in fp32."""
    from magpo_amd.envs import CoordSumConfig, LbfConfig
    from oracle import lbf as olbf
    from oracle import learner as olearn
    env, args, N, T, nb, nh = c
    if env == "coordsum":
        spec, cfg, mod = cs.CoordSumSpec(*args), CoordSumConfig(*args), cs
        A, K, F = args[0], args[1], args[0] + 1
    else:
        spec, cfg, mod = olbf.LbfSpec(*args), LbfConfig(*args), olbf
        A, K, F = spec.num_agents, 6, spec.obs_dim
    mcfg = MatCfg(A, K, F, 64, nh, nb)
    gp = init_params(1, mcfg, randomize=True)
    sys = olearn.SystemCfg(rollout_length=T, ppo_epochs=PARITY_EPOCHS, num_minibatches=PARITY_MINIBATCHES)
    ol = MatOracleLearner(spec, N, sys, mcfg, gp, dtype=dtype, env=mod)
    key = prng.split(prng.prng_key(PARITY_SEED + PARITY_SEED_BUMP.get(case_id(c), 0)), 3)[0]
    ol.setup(key)
    return ol, cfg, dict(key=key, gp=gp, A=A, K=K, F=F, N=N, T=T, nb=nb, nh=nh)
