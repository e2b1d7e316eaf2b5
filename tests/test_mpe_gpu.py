"""MPE simple_spread on the GPU (csrc/mpe.hip) against tests/mpe_ref.py -- both restate JaxMARL's MPE (UNPINNED dynamics) and the
reference's MPEWrapper and must agree bit for bit, contact forces and collisions included; then the MAGPO learner on the first env whose
agents get different rewards in one step (narrow rows with the fused acting kernel, 10 agents on wide rows through SableGuider.act), the
evaluator and the entry point."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import evaluator as oeval
from oracle import learner as olearn
from oracle import networks as onets
from oracle import prng as oprng
from tests import mpe_ref as M

pytestmark = pytest.mark.gpu


def _actions(st, A, rng, n_chase):
    """Uniform random actions, except that the first ``n_chase`` envs drive every agent at the next one along the axis of the larger
    gap: agents run into each other, so contact forces and collision penalties occur."""
    p = st["pos"][:, :A]
    d = p[:, (np.arange(A) + 1) % A] - p
    chase = np.where(np.abs(d[..., 0]) >= np.abs(d[..., 1]), np.where(d[..., 0] > 0, 2, 1), np.where(d[..., 1] > 0, 4, 3))
    a = rng.integers(0, 5, (p.shape[0], A)).astype(np.int32)
    a[:n_chase] = chase[:n_chase]
    return a


@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("A,N", [(3, 50), (5, 40), (10, 24)])
def test_mpe_env_matches_restatement(A, N, auto_reset):
    from magpo_amd.learner import MpeConfig, MpeEnvBatch, obs_row_stride
    spec, cfg = M.MpeSpec(A, A), MpeConfig(A, A)
    F, ld = cfg.obs_dim, obs_row_stride(cfg.obs_dim)
    keys = oprng.split(oprng.prng_key(100 + A), N)
    st, ts = M.reset(spec, keys)
    env = MpeEnvBatch(cfg, N, "cuda")
    obs, obs_step = torch.zeros(N, A, ld, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda")
    reward, discount = torch.zeros(N, A, device="cuda"), torch.zeros(N, A, device="cuda")
    done = torch.zeros(N, dtype=torch.uint8, device="cuda")
    m_ret, m_len, m_term = torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
    env.reset(torch.from_numpy(keys.view(np.int32)).cuda(), obs, obs_step)

    def check(tag):
        for f in ("pos", "vel", "inner_step", "step_count"):
            assert np.array_equal(getattr(env, f).cpu().numpy(), st[f]), (tag, f)
        for f in ("key", "metrics_key"):
            assert np.array_equal(getattr(env, f).cpu().numpy().view(np.uint32), st[f]), (tag, f)
        for f, g in (("run_ret", "running_return"), ("run_len", "running_length"), ("ep_ret", "episode_return"), ("ep_len", "episode_length")):
            assert np.array_equal(getattr(env, f).cpu().numpy(), st[g]), (tag, f)
        o = obs.cpu().numpy()
        assert np.array_equal(o[:, :, :F], ts["observation"]["agents_view"]), (tag, "observation")
        assert not o[:, :, F:].any(), (tag, "padding")
        assert np.array_equal(obs_step.cpu().numpy(), ts["observation"]["step_count"][:, 0]), (tag, "step_count")
    check("reset")
    rng = np.random.default_rng(A)
    contact = differ = ends = 0
    steps = 4 * (spec.time_limit + 1)
    for t in range(steps):
        a = _actions(st, A, rng, N // 2)
        contact += int((M.forces(spec, st["pos"], np.zeros((N, A, 2), np.float32)) != 0).any(axis=(1, 2)).sum())
        st, ts = M.step(spec, st, a, auto_reset=auto_reset)
        env.step(torch.from_numpy(a).cuda(), reward, done, obs, obs_step, m_ret, m_len, m_term, auto_reset=auto_reset, discount=discount)
        check(t)
        r = reward.cpu().numpy()
        assert np.array_equal(r, ts["reward"]), (t, "reward")
        assert np.array_equal(discount.cpu().numpy(), ts["discount"]), (t, "discount")
        assert np.array_equal(done.cpu().numpy().astype(bool), ts["step_type"] == M.STEP_LAST), (t, "done")
        assert np.array_equal(m_ret.cpu().numpy(), ts["episode_metrics"]["episode_return"]), (t, "episode_return")
        assert np.array_equal(m_len.cpu().numpy(), ts["episode_metrics"]["episode_length"]), (t, "episode_length")
        assert np.array_equal(m_term.cpu().numpy().astype(bool), ts["episode_metrics"]["is_terminal_step"]), (t, "is_terminal_step")
        differ += int((r != r[:, :1]).any(axis=1).sum())   # collision penalties are per agent
        ends += int(done.sum().item())
    assert contact > 0 and differ > 0, "the run must see contact forces and agents of one env with different rewards"
    assert ends == 4 * N   # every env ended 4 episodes of time_limit + 1 steps (the eval env continued past each LAST)


def _mk(A, N, T, TL, E, nh, nb, P=2, Mb=2, seed=5):
    from magpo_amd.learner import MagpoLearner, MpeConfig, SystemConfig
    spec, cfg = M.MpeSpec(A, A, time_limit=TL), MpeConfig(A, A, time_limit=TL)
    K, F = 5, spec.obs_dim
    scfg = onets.SableCfg(A, K, F, embed_dim=E, n_head=nh, n_block=nb)
    gp = onets.init_guider_params(1, E, F, K, nh=nh, nb=nb)
    ap = onets.init_actor_params(2, F, 128, K)
    gp["dec.head.dense1.kernel"] = gp["dec.head.dense1.kernel"] * 30
    ap["head.kernel"] = ap["head.kernel"] * 30
    ol = olearn.OracleLearner(spec, N, olearn.SystemCfg(rollout_length=T, ppo_epochs=P, num_minibatches=Mb), scfg, gp, ap, env=M)
    key = oprng.split(oprng.prng_key(seed), 4)[0]
    ol.setup(key)
    dl = MagpoLearner(cfg, N, SystemConfig(rollout_length=T, ppo_epochs=P, num_minibatches=Mb), "cuda", net_seed=None, wgrad_groups=4,
                      embed_dim=E, n_head=nh, n_block=nb)
    dl.guider.load_named(gp); dl.actor.load_named(ap)
    dl.setup(key)
    return ol, dl


def _close(a, b, rtol, atol, what):
    a, b = a.detach().cpu().double().reshape(-1), b.detach().cpu().double().reshape(-1)
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= atol + rtol * ref, f"{what}: max err {err:.3e} (ref scale {ref:.3e})"


@pytest.mark.parametrize("E,nh,nb,A,N,T", [(64, 1, 1, 3, 8, 16), (128, 1, 1, 3, 6, 16), (128, 2, 1, 10, 4, 12)])
def test_mpe_learner_parity(E, nh, nb, A, N, T):
    """Two consecutive update steps against the oracle learner with the restatement plugged in: actions bit-exact in both rollouts,
    parameters within the bound of test_connector_learner_parity after each.  (64, 1, 1) on 3 agents runs the fused acting kernel on
    narrow rows; (128, 2, 1) on 10 agents is the tuned net of simple_spread_10ag (experiment_data/params.csv:101) on wide rows through
    SableGuider.act; its rewards differ between agents, so GAE and both losses see non-identical per-agent values."""
    TL = 5   # episodes of 6 steps: both rollouts cross episode ends and auto-resets
    ol, dl = _mk(A, N, T, TL, E, nh, nb)
    F = M.MpeSpec(A, A).obs_dim
    differ = 0
    for it in range(2):
        om = ol.rollout()
        dl.rollout()
        tr, otr = dl.traj, ol.traj
        assert np.array_equal(tr["action"].cpu().numpy(), otr["action"].numpy()), (it, "sampled actions differ")
        assert np.array_equal(tr["obs"][:T, :, :, :F].cpu().numpy(), otr["obs"].numpy()), it
        assert np.array_equal(tr["step_count"][:T].cpu().numpy(), otr["step_count"][..., 0].numpy()), it
        rw = tr["reward"].cpu().numpy()
        assert np.array_equal(rw, otr["reward"].numpy()), it
        differ += int((rw != rw[..., :1]).any(-1).sum())
        _close(tr["value"], otr["value"], 1e-4, 1e-6, "value")
        _close(tr["log_prob"], otr["log_prob"], 1e-4, 1e-6, "log_prob")
        for k in ("episode_return", "episode_length"):
            assert np.array_equal(dl.metrics[k].cpu().numpy(), om[k]), (it, k)
        assert om["is_terminal_step"].any()
        ol.update()
        dl.update()
        dl._carry_over()   # what update_step does between a rollout and the next
        assert np.array_equal(dl.key, ol.key)
        for net, ref in ((dl.guider, ol.gp), (dl.actor, ol.ap)):
            for n, v in net.named.items():
                d = (v.detach().cpu().double().reshape(-1) - ref[n].reshape(v.shape).double().reshape(-1)).abs()
                assert d.max().item() <= 3e-5, f"update {it}, param {n}: max err {d.max().item():.3e}"
    if A == 10:   # crowded: collision penalties make the rewards of one env's agents differ (the 3-agent runs may see none)
        assert differ > 0, "per-agent rewards must differ somewhere in the rollouts"


def test_mpe_evaluator_and_entry_point(tmp_path):
    from magpo_amd.actor import GruActor
    from magpo_amd.config import compose
    from magpo_amd.evaluator import get_eval_fn, get_num_eval_envs, make_rec_eval_act_fn
    from magpo_amd.systems.gpo.anakin import rec_magpo
    from magpo_amd.utils import make_env as environments
    cfg = compose("rec_magpo", ["env=mpe", "env/scenario=simple_spread_3ag", "env.kwargs.action_type=Discrete", "arch.num_envs=6",
                                "arch.num_eval_episodes=12"])
    env, eval_env = environments.make(cfg)
    A, K, F = env.num_agents, env.action_dim, env.obs_dim
    assert (A, K, F) == (3, 5, 21)
    ap = onets.init_actor_params(17, F, 128, K)
    ap["head.kernel"] = ap["head.kernel"] * 40
    actor = GruActor(A, K, F, "cuda")
    evaluator = get_eval_fn(eval_env, make_rec_eval_act_fn(actor, cfg), cfg, absolute_metric=False, device="cuda")
    n = get_num_eval_envs(cfg, False)
    key = oprng.split(oprng.prng_key(2), 3)[1]
    got = evaluator({k: v.cuda() for k, v in ap.items()}, key, {"hidden_state": torch.zeros(n * A, 128, device="cuda")})
    want = oeval.evaluate(M.MpeSpec(3, 3), ap, key, 6, 12, env=M)
    assert np.array_equal(got["episode_length"], want["episode_length"]) and (want["episode_length"] == 26).all()
    assert np.array_equal(got["episode_return"], want["episode_return"])
    # the training entry point, shortened
    cfg = compose("rec_magpo", ["env=mpe", "env/scenario=simple_spread_3ag", "env.kwargs.action_type=Discrete", "arch.num_envs=8",
                                "arch.num_evaluation=2", "arch.num_eval_episodes=8", "arch.num_absolute_metric_eval_episodes=16",
                                "system.total_timesteps=~", "system.num_updates=4", "system.rollout_length=16", "system.ppo_epochs=2",
                                "logger.loggers.json.enabled=True", f"logger.base_exp_path={tmp_path}/", "logger.loggers.json.path=run"])
    perf = rec_magpo.run_experiment(cfg)
    assert np.isfinite(perf) and perf < 0
    data = json.load(open(os.path.join(tmp_path, "json", "run", "metrics.json")))
    run = data["MPE"]["simple_spread_3ag"]["rec_magpo"]["seed_42"]
    assert "step_0" in run and "absolute_metrics" in run and "mean_episode_return" in run["step_0"]
