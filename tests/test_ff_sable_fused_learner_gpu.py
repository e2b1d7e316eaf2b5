"""FfSableLearner with the one-launch acting step (Tuning.ff_sable_fused_act: SableGuider.act_team_fused, "magpo_ff_sable_act") against the
same learner on the kernel-by-kernel chain: which ABI calls a rollout and a minibatch step make, equal trajectories from one key, equal
parameters after an update within the bar of tests/test_ff_sable_learner_gpu.py, graph replay against eager with two env groups, and a
masked env (LBF)."""
import numpy as np
import pytest
import torch

from tests.gpu_util import _count_calls

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 8


def close(a, b, rtol, atol, what):
    a, b = a.detach().cpu().double().reshape(-1), b.detach().cpu().double().reshape(-1)
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= atol + rtol * ref, f"{what}: max err {err:.3e} (ref scale {ref:.3e})"


def _learner(fused, env_cfg=None, N=8, seed=4, num_groups=1, use_graph=False, P=1, M=1):
    from magpo_amd.ff_sable_learner import FfSableLearner
    from magpo_amd.learner import CoordSumConfig, SystemConfig
    from magpo_amd.tuning import Tuning
    t = Tuning()
    t.ff_sable_fused_act = fused
    l = FfSableLearner(env_cfg or CoordSumConfig(3, 10, 5, 30), N, SystemConfig(rollout_length=T, ppo_epochs=P, num_minibatches=M), DEV, net_seed=seed,
                       wgrad_groups=4, num_groups=num_groups, tuning=t)
    l.use_graph = use_graph
    return l


def _key(seed=5):
    from magpo_amd.learner import host_split, prng_key
    return host_split(prng_key(seed), 3)[0]


def test_default_follows_the_tuning_and_the_callers_functions_win():
    from magpo_amd.ff_sable_learner import FfSableLearner
    from magpo_amd.learner import CoordSumConfig, SystemConfig
    on, off = _learner(True), _learner(False)
    assert on.sable_action_select_fn.__name__ == "act_team_fused" and on.sable_action_select_fn.__self__ is on.guider
    assert off.sable_action_select_fn.__name__ == "act" and off.sable_action_select_fn.__self__ is off.guider
    g = on.guider
    mine = FfSableLearner(CoordSumConfig(3, 10, 5, 30), 8, SystemConfig(rollout_length=T), DEV, guider=g, apply_fns=(g.act, g.apply))
    assert mine.tuning.ff_sable_fused_act and mine.sable_action_select_fn.__name__ == "act"


def test_abi_calls_of_a_rollout_and_a_minibatch_step():
    on, off = _learner(True), _learner(False)
    for l in (on, off):
        l.setup(_key())
    c_on, c_off, c_mb = {}, {}, {}
    _count_calls(on.L, c_on, on.rollout)
    _count_calls(off.L, c_off, off.rollout)
    assert c_on.get("magpo_ff_sable_act") == T + 1, c_on
    for n in ("magpo_team_retention_fwd", "magpo_sample_categorical", "magpo_linear_pro", "magpo_linear"):
        assert c_on.get(n, 0) == 0, (n, c_on)
    assert c_off.get("magpo_ff_sable_act", 0) == 0 and c_off.get("magpo_team_retention_fwd", 0) > 0 and c_off.get("magpo_sample_categorical", 0) == T * 3
    from magpo_amd.learner import host_split
    ks = host_split(on.key, 4)
    bp, ap = on._permutation(ks[1], T * 8), on._permutation(ks[2], 3)
    _count_calls(on.L, c_mb, lambda: on.minibatch_grads(bp, ap))
    assert c_mb.get("magpo_team_retention_fwd", 0) > 0 and c_mb.get("magpo_team_retention_bwd", 0) > 0 and c_mb.get("magpo_ff_sable_act", 0) == 0


def _same_trajectories(on, off, what):
    for k in ("action", "obs", "reward", "done", "step_count"):
        assert torch.equal(on.traj[k], off.traj[k]), (what, k)
    if on.traj["mask"] is not None:
        assert torch.equal(on.traj["mask"], off.traj["mask"]), what
    for f in on.env.state_fields:
        assert torch.equal(getattr(on.env, f), getattr(off.env, f)), (what, f)
    assert np.array_equal(on.key, off.key), what
    close(on.traj["value"], off.traj["value"], 1e-4, 1e-6, f"{what}: value")
    close(on.traj["log_prob"], off.traj["log_prob"], 1e-4, 1e-6, f"{what}: log_prob")
    close(on.last_val, off.last_val, 1e-4, 1e-6, f"{what}: last_val")


def test_both_paths_from_one_key():
    """Two rollouts (the second after an update, so with parameters that moved): the same actions, observations, rewards, dones and env
    keys; values and log-probs within 1e-4 + 1e-6; parameters after one update within 3e-5."""
    on, off = _learner(True, P=2, M=2), _learner(False, P=2, M=2)
    for l in (on, off):
        l.setup(_key())
    for l in (on, off):
        l.rollout()
    _same_trajectories(on, off, "rollout 1")
    assert bool(on.traj["done"].any()) and len(torch.unique(on.traj["action"])) > 1
    for l in (on, off):
        l.update()
        l._carry_over()
    for (n, a), b in zip(on.guider.named.items(), off.guider.named.values()):
        close(a, b, 0, 3e-5, f"param {n}")
    off.guider.P.flat.copy_(on.guider.P.flat)   # rollout 2 from common parameters
    off.guider.refresh()
    for l in (on, off):
        l.rollout()
    _same_trajectories(on, off, "rollout 2")


def test_graph_replayed_rollout_equals_the_eager_one_with_two_groups():
    key = _key()
    ls = [_learner(True, num_groups=2, use_graph=g) for g in (False, True)]
    for l in ls:
        l.setup(key, n_groups=2)
    eager, graphed = ls
    for it in range(3):
        for l in ls:
            l.update_step()
        for gi, (ge, gg) in enumerate(zip(eager.groups, graphed.groups)):
            for k in ("action", "value", "log_prob", "reward", "adv"):
                assert torch.equal(ge.traj[k], gg.traj[k]), (it, gi, k)
            assert np.array_equal(ge.key, gg.key)
        assert torch.equal(eager.guider.P.flat, graphed.guider.P.flat), it
    assert all(g.graph is not None for g in graphed.groups) and not any(g.graph_failed for g in graphed.groups)
    assert all(g.graph is None for g in eager.groups)


def test_masked_env_samples_no_illegal_action():
    from magpo_amd.envs import LbfConfig
    cfg = LbfConfig(8, 8, 2, 2, 2, True, 6)
    on, off = _learner(True, cfg, seed=9), _learner(False, cfg, seed=9)
    for l in (on, off):   # (a logit head with a visible spread, as the parity cases of the masked envs)
        l.guider.named["dec.head.dense1.kernel"].mul_(30.0)
        l.guider.refresh()
        l.setup(_key(11))
        l.rollout()
    tr = on.traj
    assert tr["mask"] is not None and not bool(tr["mask"][:T].all()), "the env masks nothing: not what the case is for"
    assert bool(torch.gather(tr["mask"][:T], -1, tr["action"].long().unsqueeze(-1)).all()), "an illegal action was sampled"
    _same_trajectories(on, off, "lbf")
