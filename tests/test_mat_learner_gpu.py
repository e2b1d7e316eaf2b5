"""The MAT system on the GPU (magpo_amd/mat.py: MatNetwork inside FfSableLearner; systems/mat/anakin/mat.py) against its CPU restatement
(tests/mat_ref.py: MatOracleLearner) on identical seeds, parameters and PRNG keys, in the manner and with the bars of
tests/test_ff_sable_learner_gpu.py: sampled actions, observations, dones, rewards, env state and keys bit-exact in every rollout, values and
log-probs <= 1e-4, loss scalars <= 1e-3, every parameter gradient <= 2e-3 of the tensor's max, parameters <= 3e-5 per update step.
tests/test_mat_system.py shows that none of the seeds used here has a Gumbel near-tie; no step is excluded."""
import os

import numpy as np
import pytest
import torch

from oracle import prng as oprng
from tests import mat_ref as mr
from tests.test_ff_sable_learner_gpu import _rollout_parity, close

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 8


def _net(info, **kw):
    from magpo_amd.mat import MatNetwork
    return MatNetwork(info["A"], info["K"], info["F"], DEV, n_head=info["nh"], n_block=info["nb"], wgrad_groups=4, **kw)


def _learner(cfg, N, net, P=mr.PARITY_EPOCHS, M=mr.PARITY_MINIBATCHES, use_graph=True):
    from magpo_amd.ff_sable_learner import FfSableLearner
    from magpo_amd.learner import SystemConfig
    from magpo_amd.optim import ClipAdam
    sysc = SystemConfig(rollout_length=T, ppo_epochs=P, num_minibatches=M)
    dl = FfSableLearner(cfg, N, sysc, DEV, guider=net, optim=ClipAdam(net, sysc), apply_fns=(net.act, net.apply))
    dl.use_graph = use_graph
    return dl


def _mk(case):
    from magpo_amd.learner import obs_row_stride
    ol, cfg, info = mr.make_case(case)
    net = _net(info, obs_ld=obs_row_stride(cfg.obs_dim))
    net.load_named(info["gp"])
    dl = _learner(cfg, info["N"], net)
    dl.setup(info["key"])
    return ol, dl, info


def _sync_oracle(ol, dl):
    """The oracle takes over the device's parameters and Adam moments (each further step is compared from a common starting point; the
    drift up to there is bounded separately)."""
    from magpo_amd.params import mat_named_views
    drift = max((v.cpu() - ol.gp[n].reshape(v.shape)).abs().max().item() for n, v in dl.guider.named.items())
    assert drift <= 3e-5, f"parameter drift: {drift:.2e}"
    mn, nn = mat_named_views(dl.guider.P.views(dl.g_opt.mu)), mat_named_views(dl.guider.P.views(dl.g_opt.nu))
    for n in ol.gp:
        ol.gp[n] = dl.guider.named[n].detach().cpu().reshape(ol.gp[n].shape).clone()
        ol.g_opt["mu"][n] = mn[n].detach().cpu().reshape(ol.gp[n].shape).clone()
        ol.g_opt["nu"][n] = nn[n].detach().cpu().reshape(ol.gp[n].shape).clone()


@pytest.mark.parametrize("case", mr.PARITY_CASES, ids=mr.case_id)
def test_update_steps_against_the_restatement(case):
    """Two consecutive update steps on CoordSum; one rollout and one update on the masked env."""
    ol, dl, info = _mk(case)
    N, A = info["N"], info["A"]
    assert set(dl.guider.named) == set(ol.gp)
    for step in ((1, 2) if case[0] == "coordsum" else (1,)):
        what = f"update step {step}"
        if step > 1:
            _sync_oracle(ol, dl)
        _rollout_parity(ol, dl, what)
        if step == 1:   # one minibatch: losses and gradients (hand-written backward against the restatement's autograd)
            ks = oprng.split(ol.key, 4)
            bp, apm = oprng.permutation(ks[1], T * N), oprng.permutation(ks[2], A)
            bpd, apd = dl._permutation(ks[1], T * N), dl._permutation(ks[2], A)
            assert np.array_equal(bpd.cpu().numpy(), bp) and np.array_equal(apd.cpu().numpy(), apm)
            gg, oinfo, inter = ol.minibatch_grads(ol.make_minibatches(bp, apm)[1])
            dl.minibatch_grads(bpd[T * N // 2:].contiguous(), apd)
            lo = dl.loss_out.cpu()
            for i, k in enumerate(("total_loss", "actor_loss", "entropy", "value_loss")):
                close(lo[i], torch.tensor(oinfo[k]), 1e-3, 2e-6, k)
            close(dl.guider.b.t["t_value"], inter["value"], 1e-4, 1e-6, "train value")
            for n, g in dl.guider.named_grads.items():
                # a key bias adds the same q_i . b to every score of row i, which a softmax does not see: its gradient is identically zero
                # and both sides hold the rounding noise of sum_rows dk.  It is held to the scale of the same attention's query-bias gradient
                # (its neighbour in the fused bias vector).
                ref = gg[n.replace(".key.bias", ".query.bias")]
                assert ref.abs().max().item() > 0, f"grad {n}: the reference gradient is identically zero: the case tests nothing"
                scale = max(ref.abs().max().item(), 1e-6)
                close(g / scale, gg[n].reshape(g.shape) / scale, 0, 2e-3, f"grad {n}")
        oinfos, _ = ol.update()
        losses = dl.update().cpu()
        dl._carry_over()
        assert np.array_equal(dl.key, ol.key)
        assert losses.shape == (2, 2, 4)
        for n, v in dl.guider.named.items():
            close(v, ol.gp[n].reshape(v.shape), 0, 3e-5, f"param {n} ({what})")
        close(losses[-1, -1, 3], torch.tensor(oinfos[-1]["value_loss"]), 5e-3, 1e-5, "final value loss")
        assert dl.g_opt.count == ol.g_opt["count"] == 4 * step
    if case[0] == "coordsum":
        assert dl.groups[0].graph is not None, "the rollout of step 2 should have been a HIP-graph capture / replay"


def _coordsum_learner(use_graph, seed=4, N=6):
    from magpo_amd.learner import CoordSumConfig, obs_row_stride
    from magpo_amd.mat import MatNetwork
    cfg = CoordSumConfig(3, 10, 5, 30)
    net = MatNetwork(3, 10, 4, DEV, n_head=2, n_block=2, wgrad_groups=4, seed=seed, obs_ld=obs_row_stride(cfg.obs_dim))
    return _learner(cfg, N, net, P=1, M=1, use_graph=use_graph)


def test_graph_replay_equals_eager_rollout():
    from magpo_amd.learner import host_split, prng_key
    key = host_split(prng_key(5), 3)[0]
    ls = [_coordsum_learner(g) for g in (False, True)]
    for l in ls:
        l.setup(key)
    eager, graphed = ls
    for it in range(3):
        for l in ls:
            l.update_step()
        for k in ("action", "value", "log_prob", "reward", "adv"):
            assert torch.equal(eager.groups[0].traj[k], graphed.groups[0].traj[k]), (it, k)
        assert np.array_equal(eager.groups[0].key, graphed.groups[0].key)
        assert torch.equal(eager.guider.P.flat, graphed.guider.P.flat), it
    assert graphed.groups[0].graph is not None and not graphed.groups[0].graph_failed and eager.groups[0].graph is None
    assert bool(eager.groups[0].traj["done"].any())


def test_twin_acts_identically_after_load_named():
    from magpo_amd.mat import MatNetwork
    N, A, K, F = 7, 3, 10, 4
    net = MatNetwork(A, K, F, DEV, n_head=2, n_block=2, seed=11)
    tw = net.twin()
    assert tw is not net and tw.P.flat.data_ptr() != net.P.flat.data_ptr() and tw.tuning is net.tuning
    tw.load_named({k: v.clone() for k, v in net.named.items()})
    assert torch.equal(tw.P.flat, net.P.flat)
    obs = torch.randn(N, A, F, device=DEV)
    keys = oprng.split(oprng.prng_key(3), A)
    outs = []
    for n in (net, tw):
        action, logp, value = torch.empty(N, A, dtype=torch.int32, device=DEV), torch.empty(N, A, device=DEV), torch.empty(N, A, device=DEV)
        n.act(obs, None, None, keys, action, logp, value)
        outs.append((action, logp, value))
    assert all(torch.equal(a, b) for a, b in zip(*outs))
    with pytest.raises(NotImplementedError, match="embed_dim"):
        MatNetwork(A, K, F, DEV, embed_dim=128)


def _small_cfg(tmp_path, seed, extra=()):
    from magpo_amd.config import compose
    return compose("mat", ["env=coordsum", "env/scenario=3x10-30", "arch.num_envs=6", "arch.num_evaluation=2", "arch.num_eval_episodes=6",
                           "system.total_timesteps=~", "system.num_updates=4", f"system.rollout_length={T}", "system.ppo_epochs=2",
                           "system.update_batch_size=2", "network.n_block=2", "network.n_head=2", "env.kwargs.time_limit=5", f"system.seed={seed}",
                           f"logger.base_exp_path={tmp_path}/", *extra])


def _setup(cfg):
    from magpo_amd.learner import host_split, prng_key
    from magpo_amd.systems.mat.anakin import mat
    from magpo_amd.utils import make_env as environments
    from magpo_amd.utils.config import check_total_timesteps
    env, _ = environments.make(cfg)
    ks = host_split(prng_key(int(cfg.system.seed)), 3)
    learn, net, state = mat.learner_setup(env, (ks[0], ks[2]), cfg, torch.device(DEV))
    cfg = check_total_timesteps(cfg, 1)
    cfg.system.num_updates_per_eval = 1
    return learn, net, state


def _flat(state):
    out = [state.params[k] for k in sorted(state.params)] + [state.opt_states["mu"], state.opt_states["nu"], state.timestep["last"],
                                                             state.timestep["agents_view"], state.timestep["step_count"],
                                                             *[state.env_state[k] for k in sorted(state.env_state)]]
    return [t.detach().cpu() for t in out]


def test_learn_is_a_function_of_its_state_and_checkpoints_resume(tmp_path):
    """State in, state out: an OLD state passed again gives the same successor, and a checkpoint restored into a learner set up from
    another seed continues bit-identically to the uninterrupted run."""
    from magpo_amd.mat import MatNetwork
    from magpo_amd.systems.mat.types import LearnerState
    from magpo_amd.utils.checkpointing import Checkpointer, restore_learner_state
    learn, net, s0 = _setup(_small_cfg(tmp_path, 42))
    assert isinstance(net, MatNetwork) and net is learn.learner.guider and isinstance(s0, LearnerState) and (net.nb, net.nh) == (2, 2)
    s1 = learn(s0).learner_state
    s2 = learn(s1).learner_state
    ck = Checkpointer("mat", base_path=str(tmp_path), checkpoint_uid="resume")
    ck.save(2, s2, episode_return=1.0)
    out3 = learn(s2)
    s3 = out3.learner_state
    assert set(out3.train_metrics) == {"total_loss", "actor_loss", "entropy", "value_loss"} and out3.train_metrics["entropy"].shape == (1, 2, 1)
    s2b = learn(s1).learner_state
    assert np.array_equal(s2b.key, s2.key)
    for a, b in zip(_flat(s2b), _flat(s2)):
        assert torch.equal(a, b)
    learn2, _, t0 = _setup(_small_cfg(tmp_path, 7))
    assert not torch.equal(_flat(t0)[0], _flat(s0)[0])
    restored, ts = restore_learner_state(os.path.join(tmp_path, "checkpoints", "mat", "resume", "2.pt"), DEV)
    assert ts == 2 and isinstance(restored, LearnerState)
    r3 = learn2(restored).learner_state
    assert np.array_equal(r3.key, s3.key)
    for a, b in zip(_flat(r3), _flat(s3)):
        assert torch.equal(a, b), "resumed run differs from the uninterrupted one"


def test_hydra_entry_point_trains_and_evaluates(tmp_path):
    from magpo_amd.systems.mat.anakin import mat
    perf = mat.hydra_entry_point(["env=coordsum", "env/scenario=3x10-30", "arch.num_envs=8", "arch.num_evaluation=2", "arch.num_eval_episodes=8",
                                  "arch.absolute_metric=False", "system.num_updates=4", f"system.rollout_length={T}", "system.ppo_epochs=1",
                                  "env.kwargs.time_limit=6", f"logger.base_exp_path={tmp_path}/", "logger.checkpointing.save_model=True"])
    assert np.isfinite(perf) and 0.0 <= perf <= 20.0
    ckdir = os.path.join(tmp_path, "checkpoints", "mat")
    assert [f for d in os.listdir(ckdir) for f in os.listdir(os.path.join(ckdir, d)) if f.endswith(".pt")]
