"""Configurable actor torsos on the GPU: the LayerNorm + activation row kernels and the tanh epilogues of magpo_linear against fp64
autograd, the actor's training forward / backward against an fp64 restatement (oracle.networks.gru_cell between in-test MLPTorsos),
and the learner end to end with non-default torsos (graph replay, class tables, checkpoint resume, one update against the oracle)."""
import math
import os

import numpy as np
import pytest
import torch

from magpo_amd.torso import TorsoSpec
from oracle import coordsum as ocs
from oracle import learner as olearn
from oracle import networks as onets
from oracle import prng as oprng
from tests.gpu_util import transpose_pad

pytestmark = pytest.mark.gpu
DEV = "cuda"


def close(a, b, rtol=2e-5, atol=2e-6, what=""):
    a = a.detach().cpu().double().reshape(-1)
    b = b.detach().cpu().double().reshape(-1)
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= atol + rtol * ref, f"{what}: max err {err:.3e} vs ref scale {ref:.3e}"


ACT = {"none": 0, "relu": 1, "tanh": 5}


def _act(x, name):
    return torch.relu(x) if name == "relu" else (torch.tanh(x) if name == "tanh" else x)


def _ln(x, b, eps=1e-6):
    """flax LayerNorm(use_scale=False) with its fast variance E[x^2] - E[x]^2 (clipped at 0)."""
    m = x.mean(-1, keepdim=True)
    var = ((x * x).mean(-1, keepdim=True) - m * m).clamp(min=0)
    return (x - m) * torch.rsqrt(var + eps) + b


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels

@pytest.mark.parametrize("D", [64, 128, 192, 256])
@pytest.mark.parametrize("act", ["relu", "tanh", "none"])
def test_layernorm_act_forward_backward(L, stream, D, act):
    R = 77 if D != 128 else 333   # ragged: not a multiple of the rows per wave / workgroup
    g = torch.Generator().manual_seed(D + ACT[act])
    z = (torch.randn(R, D, generator=g) * 1.7 + 0.4).double().requires_grad_(True)
    b = (torch.randn(D, generator=g) * 0.3).double().requires_grad_(True)
    dy = torch.randn(R, D, generator=g).double()
    ref = _act(_ln(z, b), act)
    (ref * dy).sum().backward()
    y = torch.full((R + 1, D), 7.0, device=DEV); xh = torch.empty(R, D, device=DEV); rs = torch.empty(R, device=DEV)
    zd, bd = z.detach().float().to(DEV), b.detach().float().to(DEV)
    assert L.call("magpo_ln_act_fwd", zd, D, bd, y, D, xh, D, rs, R, D, ACT[act], stream) == 0
    close(y[:R], ref, what="y")
    assert bool((y[R] == 7.0).all()), "wrote past the last row"
    dz = torch.full((R + 1, D), 7.0, device=DEV)
    grid = L.call("magpo_row_grid", R)
    slab = torch.empty(grid, D, device=DEV); db = torch.empty(D, device=DEV)
    assert L.call("magpo_ln_act_bwd", dy.float().to(DEV), D, y, D, xh, D, rs, dz, D, slab, R, D, ACT[act], stream) == 0
    L.call("magpo_reduce_slabs", slab, db, grid, D, D, 1.0, 0, stream)
    close(dz[:R], z.grad, 2e-5, 2e-6, "dz")
    close(db, b.grad, 2e-5, 2e-6, "dbias")
    assert bool((dz[R] == 7.0).all())


def test_layernorm_act_rejects_bad_shapes(L, stream):
    x = torch.zeros(4, 96, device=DEV)
    with pytest.raises(ValueError):
        L.call("magpo_ln_act_fwd", x, 96, x[0], x, 96, x, 96, x[:, 0], 4, 96, 1, stream)
    x = torch.zeros(4, 128, device=DEV)
    with pytest.raises(ValueError):
        L.call("magpo_ln_act_fwd", x, 128, x[0], x, 128, x, 128, x[:, 0], 4, 128, 2, stream)


@pytest.mark.parametrize("KIN,NOUT,R,variant", [(64, 256, 130, 0), (128, 128, 77, 0), (256, 64, 65, 0),
                                                (192, 192, 300, 0), (128, 384, 1000, 4), (64, 64, 33, 0)])
def test_linear_tanh_epilogue(L, stream, KIN, NOUT, R, variant):
    g = torch.Generator().manual_seed(KIN + NOUT)
    X = torch.randn(R, KIN, generator=g); W = torch.randn(KIN, NOUT, generator=g) / math.sqrt(KIN); b = torch.randn(NOUT, generator=g)
    Y = torch.zeros(R, NOUT, device=DEV)
    assert L.call("magpo_linear", X.to(DEV), KIN, transpose_pad(L, stream, W.to(DEV)), b.to(DEV), Y, NOUT, None, R, KIN, NOUT, 5, variant, stream) == 0
    z = X.double() @ W.double() + b.double()
    close(Y, torch.tanh(z), what="tanh")


@pytest.mark.parametrize("KIN,NOUT,R,variant", [(64, 256, 130, 0), (128, 128, 77, 0), (384, 128, 70, 0), (384, 256, 129, 0), (256, 64, 4001, 4)])
def test_linear_fused_tanh_backward(L, stream, KIN, NOUT, R, variant):
    """act 6: dX = (dY W^T) * (1 - y^2) with y (the forward's tanh output) as the mask argument, on the shared-tile kernels."""
    g = torch.Generator().manual_seed(3 * KIN + NOUT)
    dY = torch.randn(R, KIN, generator=g); W = torch.randn(NOUT, KIN, generator=g) / math.sqrt(KIN)   # natural [NOUT][KIN]: dX = dY W^T
    y = torch.tanh(torch.randn(R, NOUT, generator=g))
    out = torch.zeros(R, NOUT, device=DEV)
    assert L.call("magpo_linear", dY.to(DEV), KIN, W.to(DEV), None, out, NOUT, y.to(DEV), R, KIN, NOUT, 6, variant, stream) == 0
    close(out, (dY.double() @ W.double().T) * (1 - y.double() ** 2), what="tanh backward")
    with pytest.raises(ValueError):   # the mask is required
        L.call("magpo_linear", dY.to(DEV), KIN, W.to(DEV), None, out, NOUT, None, R, KIN, NOUT, 6, 0, stream)


# ---------------------------------------------------------------------------------------------------------------------------------
# the actor against an fp64 restatement

def _mlp(p, prefix, spec, x):
    """MLPTorso.__call__ (torsos.py:36-47) on the device actor's parameter names."""
    for i in range(len(spec.layer_sizes)):
        n = prefix if i == 0 else f"{prefix}{i}"
        x = x @ p[n + ".kernel"] + p[n + ".bias"]
        if spec.use_layer_norm:
            x = _ln(x, p[n + ".ln.bias"])
        if i < len(spec.layer_sizes) - 1 or spec.activate_final:
            x = _act(x, spec.activation)
    return x


def general_actor_apply(pre, post):
    """oracle.networks.actor_apply with the torsos of the config (RecurrentActor, base.py:161-184)."""
    def actor_apply(p, hidden, obs, done, mask):
        emb = _mlp(p, "pre", pre, obs.to(p["pre.kernel"].dtype))
        h, outs = hidden, []
        for t in range(obs.shape[0]):
            h = torch.where(done[t][..., None], torch.zeros_like(h), h)
            h = onets.gru_cell(p, h, emb[t])
            outs.append(h)
        ys = torch.stack(outs, 0)
        logits = _mlp(p, "post", post, ys) @ p["head.kernel"] + p["head.bias"]
        return h, onets.masked_log_softmax(logits, mask), ys
    return actor_apply


CASES = {
    "pre256-128-ln-tanh": (3, 10, 4, TorsoSpec((256, 128), "tanh", True), TorsoSpec((128,))),
    "pre64-post128x2": (3, 10, 4, TorsoSpec((64,)), TorsoSpec((128, 128))),
    "no-final-activation": (2, 6, 5, TorsoSpec((128,), activate_final=False), TorsoSpec((192, 64), "tanh", activate_final=False)),
    "rware-wide-ln": (2, 5, 73, TorsoSpec((128, 192), "relu", True), TorsoSpec((256,), "tanh", True)),
    "default": (3, 10, 4, TorsoSpec(), TorsoSpec()),
}


@pytest.mark.parametrize("case", list(CASES))
def test_actor_seq_fwd_bwd_carry_step_match_fp64(case):
    from magpo_amd.actor import GruActor
    A, K, F, pre, post = CASES[case]
    nseq, T = 5, 7
    R = nseq * T * A
    actor = GruActor(A, K, F, DEV, seed=5, wgrad_groups=4, pre_torso=pre, post_torso=post)
    with torch.no_grad():   # non-zero biases so that every bias path is exercised
        g0 = torch.Generator().manual_seed(1)
        for n, v in actor.named.items():
            if n.endswith("bias"):
                v.copy_(0.1 * torch.randn(v.shape, generator=g0))
    actor.refresh()
    g = torch.Generator().manual_seed(len(case))
    obs = torch.randn(nseq, T, A, F, generator=g)
    obs_d = torch.zeros(R, actor.Fld, device=DEV)
    obs_d[:, :F] = obs.reshape(R, F).to(DEV)
    dones = (torch.rand(nseq, T, generator=g) < 0.25).to(torch.uint8)
    h0 = 0.5 * torch.randn(nseq * A, 128, generator=g)
    h0_idx = torch.randperm(nseq * A, generator=g).int()
    dl = torch.zeros(R, 64)
    dl[:, :K] = torch.randn(R, K, generator=g)
    logits = actor.seq_fwd(obs_d, dones.to(DEV), h0.to(DEV), h0_idx.to(DEV), nseq, T)
    hs_dev = actor.b.t["t_hs"].clone()
    actor.grads.zero_()
    actor.seq_bwd(dl.to(DEV))
    torch.cuda.synchronize()

    p = {n: v.detach().cpu().double().clone().requires_grad_(True) for n, v in actor.named.items()}
    emb = _mlp(p, "pre", pre, obs.double())                          # [nseq, T, A, D_pre]
    h = h0.double()[h0_idx.long()].reshape(nseq, A, 128)
    outs = []
    for t in range(T):
        h = torch.where(dones[:, t].bool()[:, None, None], torch.zeros_like(h), h)
        h = onets.gru_cell(p, h, emb[:, t])
        outs.append(h)
    hs = torch.stack(outs, 1)                                         # [nseq, T, A, 128]
    ref = _mlp(p, "post", post, hs) @ p["head.kernel"] + p["head.bias"]
    (ref.reshape(R, K) * dl[:, :K].double()).sum().backward()
    close(logits[:, :K], ref.reshape(R, K), 1e-4, 1e-5, "logits")
    close(hs_dev, hs.reshape(R, 128), 1e-4, 1e-6, "hidden states")
    for n, gd in actor.named_grads.items():
        gr = p[n].grad
        scale = max(gr.abs().max().item(), 1e-6)
        close(gd / scale, gr.reshape(gd.shape) / scale, 0, 2e-3, f"grad {n}")

    # carry (whole rollout at once) and step (one env step at a time) give seq_fwd's hidden states: env = sequence, identity h0 gather
    ident = torch.arange(nseq * A, dtype=torch.int32, device=DEV)
    lg_ref = actor.seq_fwd(obs_d, dones.to(DEV), h0.to(DEV), ident, nseq, T).reshape(nseq, T, A, 64)[:, T - 1].reshape(-1, 64).clone()
    hs_ref = actor.b.t["t_hs"].reshape(nseq, T, A, 128).clone()
    obs_tm = obs_d.reshape(nseq, T, A, actor.Fld).transpose(0, 1).contiguous()
    reset_tm = dones.t().contiguous().to(DEV)
    h_out = torch.empty(nseq * A, 128, device=DEV)
    actor.carry(obs_tm, h0.to(DEV), reset_tm, h_out)
    close(h_out, hs_ref[:, T - 1].reshape(-1, 128), 1e-5, 1e-6, "carry")
    h_in = h0.to(DEV)
    for t in range(T):
        h_nx = torch.empty_like(h_in)
        lg = actor.step(obs_tm[t], h_in, reset_tm[t].contiguous(), h_nx, want_logits=(t == T - 1))
        close(h_nx, hs_ref[:, t].reshape(-1, 128), 1e-5, 1e-6, f"step {t}")
        h_in = h_nx
    close(lg[:, :K], lg_ref[:, :K], 1e-5, 1e-6, "step logits")


# ---------------------------------------------------------------------------------------------------------------------------------
# learner end to end

TORSO = (TorsoSpec((256, 128), "tanh", True), TorsoSpec((64, 128)))


def test_class_tables_equal_dense_path_with_torso():
    from magpo_amd.learner import CoordSumConfig, MagpoLearner, SystemConfig, host_split, prng_key
    A, K, N, T = 3, 10, 7, 9
    sysc = SystemConfig(rollout_length=T, ppo_epochs=1, num_minibatches=1)
    key = host_split(prng_key(33), 4)[0]
    ls = []
    for tables in (False, True):
        l = MagpoLearner(CoordSumConfig(A, K, 7, 3 * K), N, sysc, DEV, net_seed=3, wgrad_groups=4, actor_torso=TORSO)
        l.class_tables = tables
        l.use_graph = False
        l.setup(key)
        l.rollout()
        g = torch.Generator().manual_seed(1)
        l.minibatch_grads(torch.randperm(N, generator=g).int().cuda(), torch.randperm(A, generator=g).int().cuda())
        torch.cuda.synchronize()
        ls.append(l)
    a, b = ls
    close(b.loss_out, a.loss_out, 1e-5, 1e-6, "losses")
    assert "pre1.ln.bias" in a.actor.named_grads
    for n, ga in a.actor.named_grads.items():
        gb = b.actor.named_grads[n]
        scale = float(ga.abs().max())
        assert scale > 0 and float((ga - gb).abs().max()) <= 3e-5 * scale + 1e-9, f"actor gradient {n} differs between class tables and dense path"


@pytest.mark.parametrize("env", ["coordsum", "rware"])
def test_graph_replay_equals_eager_with_torso(env):
    from magpo_amd.learner import CoordSumConfig, MagpoLearner, RwareConfig, SystemConfig, host_split, prng_key
    cfg = CoordSumConfig(3, 10, 7, 30) if env == "coordsum" else RwareConfig(num_agents=2, request_queue_size=2, time_limit=12)
    torso = TORSO if env == "coordsum" else (TorsoSpec((128, 64), "relu", True), TorsoSpec((192,), "tanh"))
    sysc = SystemConfig(rollout_length=9, ppo_epochs=2, num_minibatches=2)
    key = host_split(prng_key(5), 4)[0]
    ls = []
    for use_graph in (False, True):
        l = MagpoLearner(cfg, 8, sysc, DEV, net_seed=4, wgrad_groups=4, actor_torso=torso)
        l.use_graph = use_graph
        l.setup(key)
        ls.append(l)
    p0 = ls[0].actor.P.flat.clone()
    for it in range(3):
        for l in ls:
            l.update_step()
        assert bool(torch.isfinite(ls[0].loss_out).all()), ls[0].loss_out
        for k in ("action", "value", "log_prob", "reward"):
            assert torch.equal(ls[0].traj[k], ls[1].traj[k]), (it, k)
        assert torch.equal(ls[0].actor.P.flat, ls[1].actor.P.flat) and torch.equal(ls[0].guider.P.flat, ls[1].guider.P.flat)
    assert ls[1].groups[0].graph is not None and not ls[1].groups[0].graph_failed
    assert not torch.equal(ls[0].actor.P.flat, p0), "the actor must train"


_TORSO_OVERRIDES = ["network.actor_network.pre_torso.layer_sizes=[256,128]", "network.actor_network.pre_torso.use_layer_norm=True",
                    "network.actor_network.pre_torso.activation=tanh", "network.actor_network.post_torso.layer_sizes=[64,128]"]


def _small_cfg(tmp_path, seed):
    from magpo_amd.config import compose
    return compose("rec_magpo", ["env=coordsum", "env/scenario=3x10-30", "arch.num_envs=6", "arch.num_evaluation=2", "arch.num_eval_episodes=6",
                                 "system.total_timesteps=~", "system.num_updates=4", "system.rollout_length=12", "system.ppo_epochs=2",
                                 "env.kwargs.time_limit=7", f"system.seed={seed}", f"logger.base_exp_path={tmp_path}/", *_TORSO_OVERRIDES])


def test_torso_config_trains_evaluates_and_resumes(tmp_path):
    from magpo_amd.learner import host_split, prng_key
    from magpo_amd.systems.gpo.anakin import rec_magpo
    from magpo_amd.utils import make_env as environments
    from magpo_amd.utils.checkpointing import Checkpointer, restore_learner_state
    from magpo_amd.utils.config import check_total_timesteps

    def setup(cfg):
        env, _ = environments.make(cfg)
        ks = host_split(prng_key(int(cfg.system.seed)), 4)
        learn, actor, state = rec_magpo.learner_setup(env, (ks[0], ks[2], ks[3]), cfg, torch.device(DEV))
        cfg = check_total_timesteps(cfg, 1)
        cfg.system.num_updates_per_eval = 1
        return learn, actor, state

    def flat(state):
        out = [state.params.actor_params[k] for k in sorted(state.params.actor_params)] + [state.params.guider_params[k] for k in sorted(state.params.guider_params)]
        out += [state.opt_states.actor_opt_state["mu"], state.opt_states.actor_opt_state["nu"], state.hstates.policy_hidden_state]
        return [t.detach().cpu() for t in out]

    learn, actor, s0 = setup(_small_cfg(tmp_path, 42))
    assert actor.pre_spec == TORSO[0] and actor.post_spec == TORSO[1]
    assert s0.params.actor_params["pre1.kernel"].shape == (256, 128) and s0.params.actor_params["head.kernel"].shape == (128, 10)
    s1 = learn(s0)
    assert np.isfinite(s1.train_metrics["total_loss"]).all()
    s1 = s1.learner_state
    ck = Checkpointer("rec_magpo", base_path=str(tmp_path), checkpoint_uid="torso")
    ck.save(1, s1, episode_return=1.0)
    s2 = learn(s1).learner_state
    learn2, _, _ = setup(_small_cfg(tmp_path, 7))
    restored, ts = restore_learner_state(os.path.join(tmp_path, "checkpoints", "rec_magpo", "torso", "1.pt"), DEV)
    r2 = learn2(restored).learner_state
    assert np.array_equal(r2.key, s2.key)
    for a, b in zip(flat(r2), flat(s2)):
        assert torch.equal(a, b), "resumed run differs from the uninterrupted one"
    # the whole entry point: training, sampled and greedy evaluation with the configured torso
    from magpo_amd.config import compose
    cfg = compose("rec_magpo", ["env=coordsum", "env/scenario=3x10-30", "arch.num_envs=8", "arch.num_evaluation=2", "arch.num_eval_episodes=8",
                                "arch.num_absolute_metric_eval_episodes=8", "system.total_timesteps=~", "system.num_updates=4",
                                "system.rollout_length=8", "system.ppo_epochs=1", "env.kwargs.time_limit=10", f"logger.base_exp_path={tmp_path}/",
                                "arch.evaluation_greedy=True", *_TORSO_OVERRIDES])
    assert np.isfinite(rec_magpo.run_experiment(cfg))


def test_update_step_parity_with_oracle_learner(monkeypatch):
    """One update step (rollout, GAE, 1 epoch x 2 minibatches, clip + Adam) with a non-default torso against the oracle learner, whose
    actor forward is swapped for the in-test general actor: actor gradients of one minibatch, parameters after the update, and the
    sampled actions of the following rollout."""
    from magpo_amd.learner import CoordSumConfig, MagpoLearner, SystemConfig
    from magpo_amd.params import FlatParams, actor_layout, actor_named_views, init_actor
    pre, post = TorsoSpec((192, 128), "tanh", True), TorsoSpec((256,), "relu", True)
    monkeypatch.setattr(olearn.nets, "actor_apply", general_actor_apply(pre, post))
    A, K, TL, maxval, N, T = 3, 10, 9, 30, 6, 11
    spec = ocs.CoordSumSpec(A, K, TL, maxval)
    scfg = onets.SableCfg(A, K, A + 1)
    osys = olearn.SystemCfg(rollout_length=T, ppo_epochs=1, num_minibatches=2)
    gp = onets.init_guider_params(1, 64, A + 1, K)
    P = FlatParams(actor_layout(A + 1, 128, K, pre, post), "cpu")
    ap = actor_named_views(P.views())
    init_actor(ap, 2)
    with torch.no_grad():
        ap["head.kernel"].mul_(30.0)   # the actor's logits then matter to the guider's KL term
    ap = {n: v.clone() for n, v in ap.items()}
    ol = olearn.OracleLearner(spec, N, osys, scfg, gp, ap)
    key = oprng.split(oprng.prng_key(42), 4)[0]
    ol.setup(key)
    dl = MagpoLearner(CoordSumConfig(A, K, TL, maxval), N, SystemConfig(rollout_length=T, ppo_epochs=1, num_minibatches=2), DEV,
                      net_seed=None, wgrad_groups=8, actor_torso=(pre, post))
    dl.guider.load_named(gp)
    dl.actor.load_named(ap)
    dl.setup(key)
    ol.rollout()
    dl.rollout()
    assert np.array_equal(dl.traj["action"].cpu().numpy(), ol.traj["action"].numpy())
    close(dl.policy_h[dl._cur], ol.policy_h.reshape(N * A, 128), 1e-4, 1e-6, "policy hidden")
    ks = oprng.split(ol.key, 4)
    bp, apm = oprng.permutation(ks[1], N), oprng.permutation(ks[2], A)
    bpd, apd = dl._permutation(ks[1], N), dl._permutation(ks[2], A)
    mbs = ol.make_minibatches(bp, apm)
    _, ag, info, _ = ol.minibatch_grads(mbs[1])
    mbsz = N // 2
    dl.minibatch_grads(bpd[mbsz:2 * mbsz].contiguous(), apd)
    close(dl.loss_out.cpu()[2], torch.tensor(info["actor_loss"]), 1e-3, 2e-6, "actor loss")
    for n, g in dl.actor.named_grads.items():
        scale = max(ag[n].abs().max().item(), 1e-6)
        close(g / scale, ag[n].reshape(g.shape) / scale, 0, 2e-3, f"actor grad {n}")
    ol.update()
    dl.update()
    assert np.array_equal(dl.key, ol.key)
    for n, v in dl.actor.named.items():
        close(v, ol.ap[n].reshape(v.shape), 0, 3e-5, f"actor param {n}")
    for n, v in dl.guider.named.items():
        close(v, ol.gp[n].reshape(v.shape), 0, 3e-5, f"guider param {n}")
    dl._carry_over()
    ol.rollout()
    dl.rollout()
    assert np.array_equal(dl.traj["action"].cpu().numpy(), ol.traj["action"].numpy()), "sampled actions of the next rollout differ"
