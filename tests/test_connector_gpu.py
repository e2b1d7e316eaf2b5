"""VectorConnector on the GPU (csrc/connector.hip) against tests/connector_ref.py -- both restate Jumanji's Connector (UNPINNED dynamics)
and the reference's VectorConnectorWrapper and must agree bit for bit; then the MAGPO learner on its 54 + A wide observations, including
the first teams of more than 8 agents on wide observations (SableGuider.act, the kernel-by-kernel acting path), and the evaluator."""
import numpy as np
import pytest
import torch

from oracle import evaluator as oeval
from oracle import learner as olearn
from oracle import networks as onets
from oracle import prng as oprng
from tests import connector_ref as C

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("G,A,TL,N", [(5, 3, 25, 64), (7, 5, 49, 40), (10, 10, 100, 24), (15, 23, 225, 16)])
def test_connector_env_matches_restatement(G, A, TL, N):
    from magpo_amd.learner import ConnectorEnvBatch, VectorConnectorConfig
    spec, cfg = C.ConnectorSpec(G, A, TL), VectorConnectorConfig(G, A, TL)
    F = cfg.obs_dim
    keys = oprng.split(oprng.prng_key(G * 10 + A), N)
    st, ts = C.reset(spec, keys)
    env = ConnectorEnvBatch(cfg, N, "cuda")
    obs, obs_step = torch.zeros(N, A, 128, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    mask = torch.zeros(N, A, 5, dtype=torch.uint8, device="cuda")
    reward, discount = torch.zeros(N, A, device="cuda"), torch.zeros(N, A, device="cuda")
    done = torch.zeros(N, dtype=torch.uint8, device="cuda")
    m_ret, m_len, m_term = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
    env.reset(torch.from_numpy(keys.view(np.int32)).cuda(), obs, obs_step, mask)

    def check(tag):
        assert np.array_equal(env.grid.cpu().numpy(), st["grid"]), (tag, "grid")
        for f in ("agent_start", "agent_target", "agent_pos", "step_count"):
            assert np.array_equal(getattr(env, f).cpu().numpy(), st[f]), (tag, f)
        assert np.array_equal(env.key.cpu().numpy().view(np.uint32), st["key"]), tag
        assert np.array_equal(env.metrics_key.cpu().numpy().view(np.uint32), st["metrics_key"]), tag
        assert np.array_equal(obs[:, :, :F].cpu().numpy(), ts["observation"]["agents_view"]), (tag, "observation")
        assert float(obs[:, :, F:].abs().max()) == 0.0, (tag, "padding")
        assert np.array_equal(mask.cpu().numpy().astype(bool), ts["observation"]["action_mask"]), (tag, "mask")
        assert np.array_equal(obs_step.cpu().numpy(), ts["observation"]["step_count"][:, 0]), (tag, "step_count")
    check("reset")
    rng = np.random.default_rng(7)
    early = horizon = 0
    for t in range(4 * TL):
        # uniform random actions, illegal ones included (they leave the agent in place); every fourth env only NOOPs, so that some
        # episodes run into the time limit
        a = rng.integers(0, 5, (N, A)).astype(np.int32)
        a[3::4] = C.NOOP
        st, ts = C.step(spec, st, a, auto_reset=True)
        env.step(torch.from_numpy(a).cuda(), reward, done, obs, obs_step, m_ret, m_len, m_term, auto_reset=True, mask=mask, discount=discount)
        check(t)
        assert np.array_equal(reward.cpu().numpy(), ts["reward"]), t
        assert np.array_equal(discount.cpu().numpy(), ts["discount"]), t
        d = ts["step_type"] == C.STEP_LAST
        assert np.array_equal(done.cpu().numpy().astype(bool), d), t
        assert np.array_equal(m_ret.cpu().numpy(), ts["episode_metrics"]["episode_return"]), t
        assert np.array_equal(m_len.cpu().numpy(), ts["episode_metrics"]["episode_length"]), t
        assert np.array_equal(m_term.cpu().numpy().astype(bool), ts["episode_metrics"]["is_terminal_step"]), t
        lens = ts["episode_metrics"]["episode_length"][d]
        early += int((lens < TL).sum())
        horizon += int((lens == TL).sum())
    assert early > 0 and horizon > 0, "the test must see all-connected-or-blocked endings and time-limit endings"


def _mk(G, A, TL, N, T, P=2, M=2, seed=5, E=64, nh=1, nb=1):
    from magpo_amd.learner import MagpoLearner, SystemConfig, VectorConnectorConfig
    spec, cfg = C.ConnectorSpec(G, A, TL), VectorConnectorConfig(G, A, TL)
    K, F = 5, spec.obs_dim
    scfg = onets.SableCfg(A, K, F, embed_dim=E, n_head=nh, n_block=nb)
    gp = onets.init_guider_params(1, E, F, K, nh=nh, nb=nb)
    ap = onets.init_actor_params(2, F, 128, K)
    gp["dec.head.dense1.kernel"] = gp["dec.head.dense1.kernel"] * 30
    ap["head.kernel"] = ap["head.kernel"] * 30
    ol = olearn.OracleLearner(spec, N, olearn.SystemCfg(rollout_length=T, ppo_epochs=P, num_minibatches=M), scfg, gp, ap, env=C)
    key = oprng.split(oprng.prng_key(seed), 4)[0]
    ol.setup(key)
    dl = MagpoLearner(cfg, N, SystemConfig(rollout_length=T, ppo_epochs=P, num_minibatches=M), "cuda", net_seed=None, wgrad_groups=4,
                      embed_dim=E, n_head=nh, n_block=nb)
    dl.guider.load_named(gp); dl.actor.load_named(ap)
    dl.setup(key)
    return ol, dl


def _close(a, b, rtol, atol, what):
    a, b = a.detach().cpu().double().reshape(-1), b.detach().cpu().double().reshape(-1)
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= atol + rtol * ref, f"{what}: max err {err:.3e} (ref scale {ref:.3e})"


@pytest.mark.parametrize("E,nh,nb,G,A,N,T", [(64, 1, 1, 5, 3, 8, 16), (128, 4, 1, 5, 3, 8, 16), (128, 1, 3, 7, 5, 6, 12),
                                             (128, 2, 1, 10, 10, 4, 12), (128, 4, 1, 15, 23, 4, 8)])
def test_connector_learner_parity(E, nh, nb, G, A, N, T):
    """Rollout, minibatch gradients and a full update against the oracle learner with the restatement plugged in.  (64, 1, 1) runs the
    fused acting kernel on wide rows; (128, 4, 1), (128, 1, 3) and (128, 2, 1) are the tuned MAGPO nets of the con-* rows of
    experiment_data/params.csv; 10 and 23 agents are the first teams of more than 8 agents on wide observations."""
    TL = 6   # short episodes: the rollout crosses episode ends and auto-resets
    ol, dl = _mk(G, A, TL, N, T, E=E, nh=nh, nb=nb)
    F = 54 + A
    om = ol.rollout()
    dl.rollout()
    tr, otr = dl.traj, ol.traj
    assert np.array_equal(tr["action"].cpu().numpy(), otr["action"].numpy()), "sampled actions differ"
    assert np.array_equal(tr["obs"][:T, :, :, :F].cpu().numpy(), otr["obs"].numpy())
    assert np.array_equal(tr["mask"][:T].cpu().numpy().astype(bool), otr["mask"].numpy())
    assert np.array_equal(tr["reward"].cpu().numpy(), otr["reward"].numpy())
    _close(tr["value"], otr["value"], 1e-4, 1e-6, "value")
    _close(tr["log_prob"], otr["log_prob"], 1e-4, 1e-6, "log_prob")
    _close(dl.policy_h[dl._cur], ol.policy_h.reshape(N * A, 128), 1e-4, 1e-6, "policy hidden")
    assert om["is_terminal_step"].any()
    ks = oprng.split(ol.key, 4)
    bp, apm = oprng.permutation(ks[1], N), oprng.permutation(ks[2], A)
    gg, ag, info, inter = ol.minibatch_grads(ol.make_minibatches(bp, apm)[1])
    dl.minibatch_grads(dl._permutation(ks[1], N)[N // 2:].contiguous(), dl._permutation(ks[2], A))
    for n, g in dl.guider.named_grads.items():
        scale = max(gg[n].abs().max().item(), 1e-6)
        _close(g / scale, gg[n].reshape(g.shape) / scale, 0, 2e-3, f"guider grad {n}")
    for n, g in dl.actor.named_grads.items():
        scale = max(ag[n].abs().max().item(), 1e-6)
        _close(g / scale, ag[n].reshape(g.shape) / scale, 0, 2e-3, f"actor grad {n}")
    ol.update()
    dl.update()
    assert np.array_equal(dl.key, ol.key)
    # the bound of test_rware_learner_parity: 3e-5 flat, except that the retention projections of the last encoder block of a three-block
    # net (the stiff direction) may hold elements within one Adam step (lr), at most 0.1 % of a tensor
    lr = 2.5e-4
    for net, ref in ((dl.guider, ol.gp), (dl.actor, ol.ap)):
        for n, v in net.named.items():
            d = (v.detach().cpu().double().reshape(-1) - ref[n].reshape(v.shape).double().reshape(-1)).abs()
            if nb == 3 and net is dl.guider and n.startswith("enc.block2.retn."):
                assert d.max().item() <= lr, f"param {n}: max err {d.max().item():.3e}"
                assert int((d > 3e-5).sum()) <= max(0, d.numel() // 1000), f"param {n}: {int((d > 3e-5).sum())} of {d.numel()} elements beyond 3e-5"
            else:
                assert d.max().item() <= 3e-5, f"param {n}: max err {d.max().item():.3e}"


def test_connector_evaluator_and_entry_point(tmp_path):
    from magpo_amd.actor import GruActor
    from magpo_amd.config import compose
    from magpo_amd.evaluator import get_eval_fn, get_num_eval_envs, make_rec_eval_act_fn
    from magpo_amd.systems.gpo.anakin import rec_magpo
    from magpo_amd.utils import make_env as environments
    cfg = compose("rec_magpo", ["env=vector-connector", "env/scenario=con-5x5x3a", "arch.num_envs=6", "arch.num_eval_episodes=12",
                                "env.scenario.env_kwargs.time_limit=15"])
    env, eval_env = environments.make(cfg)
    A, K, F = env.num_agents, env.action_dim, env.obs_dim
    assert (A, K, F) == (3, 5, 57)
    ap = onets.init_actor_params(17, F, 128, K)
    ap["head.kernel"] = ap["head.kernel"] * 40
    actor = GruActor(A, K, F, "cuda")
    evaluator = get_eval_fn(eval_env, make_rec_eval_act_fn(actor, cfg), cfg, absolute_metric=False, device="cuda")
    n = get_num_eval_envs(cfg, False)
    key = oprng.split(oprng.prng_key(2), 3)[1]
    got = evaluator({k: v.cuda() for k, v in ap.items()}, key, {"hidden_state": torch.zeros(n * A, 128, device="cuda")})
    want = oeval.evaluate(C.ConnectorSpec(5, 3, 15), ap, key, 6, 12, env=C)
    assert np.array_equal(got["episode_length"], want["episode_length"])
    assert np.array_equal(got["episode_return"], want["episode_return"])
    # the training entry point on con-7x7x5a, shortened
    cfg = compose("rec_magpo", ["env=vector-connector", "env/scenario=con-7x7x5a", "arch.num_envs=8", "arch.num_evaluation=2",
                                "arch.num_eval_episodes=8", "arch.num_absolute_metric_eval_episodes=16", "system.total_timesteps=~",
                                "system.num_updates=4", "system.rollout_length=16", "system.ppo_epochs=2",
                                "env.scenario.env_kwargs.time_limit=20", f"logger.base_exp_path={tmp_path}/"])
    perf = rec_magpo.run_experiment(cfg)
    assert np.isfinite(perf)
