"""rec_iql without a GPU: configs against the reference's values, exported names and types, what raises at set-up, the restated window
sampler and eps schedule (tests/iql_ref.py), and the near-tie count of every seed and shape the GPU parity tests use (zero: neither a greedy
selection nor an eps-greedy sample then hangs on fp32 rounding)."""
import numpy as np
import pytest
import torch

from oracle import prng
from tests import iql_ref as ref

MLP = dict(_target_="mava.networks.torsos.MLPTorso", layer_sizes=[128], use_layer_norm=False, activation="relu")
# mava/configs/system/q_learning/rec_iql.yaml
SYSTEM_DEFAULTS = dict(total_timesteps=None, num_updates=156250, seed=1, add_agent_id=True, min_buffer_size=32, update_batch_size=1, rollout_length=2,
                       epochs=2, buffer_size=1000, sample_batch_size=32, sample_sequence_length=32, q_lr=3e-4, max_grad_norm=10, hard_update=False,
                       update_period=200, tau=0.01, gamma=0.99, eps_min=0.05, eps_decay=1e5, replay_ratio=4, error_tolerance=64)
NETWORK_DEFAULTS = dict(hidden_state_dim=128, q_network=dict(pre_torso=MLP, post_torso=MLP))


def test_config_tree_and_defaults():
    from magpo_amd.config import compose
    cfg = compose("rec_iql")
    assert set(cfg.to_container()) == {"logger", "arch", "system", "network", "env"}
    assert cfg.system.to_container() == SYSTEM_DEFAULTS
    assert cfg.network.to_container() == NETWORK_DEFAULTS
    assert cfg.env.env_name == "LevelBasedForaging"      # defaults: env: lbf
    assert "q_network" not in compose("rec_ippo").network.to_container()     # configs/network/rnn.yaml stays as it is


def test_exported_names_and_type_fields():
    from magpo_amd.systems.q_learning import types as t
    from magpo_amd.systems.q_learning.anakin import rec_iql
    for n in ("get_learner_fn", "learner_setup", "run_experiment", "hydra_entry_point"):
        assert callable(getattr(rec_iql, n)), n
    assert t.Transition._fields == ("obs", "action", "reward", "terminal", "term_or_trunc", "next_obs")
    assert t.QNetParams._fields == ("online", "target")
    assert t.ActionSelectionState._fields == ("online_params", "hidden_state", "time_steps", "key")
    assert t.ActionState._fields == ("action_selection_state", "env_state", "buffer_state", "obs", "terminal", "term_or_trunc")
    assert t.LearnerState._fields == ("obs", "terminal", "term_or_trunc", "hidden_state", "env_state", "time_steps", "train_steps", "opt_state",
                                      "buffer_state", "params", "key")
    assert t.TrainState._fields == ("buffer_state", "params", "opt_state", "train_steps", "key")


@pytest.mark.parametrize("overrides,match", [(["env=rware"], "RobotWarehouse.*real_next_obs"), (["env=vector-connector"], "real_next_obs"),
                                             (["env=mpe", "env.kwargs.action_type=Discrete"], "real_next_obs"),
                                             (["+system.micro_batches=2"], "micro_batches"),
                                             (["CONTINUOUS"], "discrete action"),
                                             (["system.sample_sequence_length=9", "system.buffer_size=8"], "sample_sequence_length"),
                                             (["system.sample_sequence_length=1"], "sample_sequence_length"),
                                             (["network.hidden_state_dim=64"], "hidden_state_dim")])
def test_unsupported_settings_raise_before_any_device_work(overrides, match):
    from magpo_amd.config import compose
    from magpo_amd.systems.q_learning.anakin import rec_iql
    from magpo_amd.utils import make_env as environments
    continuous = overrides == ["CONTINUOUS"]       # (the env factories refuse the key themselves: set it behind them)
    cfg = compose("rec_iql", [] if continuous else overrides)
    env, _ = environments.make(cfg)
    if continuous:
        cfg.env.kwargs.action_type = "Continuous"
    with pytest.raises(NotImplementedError, match=match):
        rec_iql.check_supported(env.cfg, cfg)
    with pytest.raises(NotImplementedError, match=match):     # learner_setup refuses before it builds a network
        rec_iql.learner_setup(env, (prng.prng_key(0), prng.prng_key(1)), cfg, device="cpu")


def test_learner_refuses_unsupported_settings():
    from magpo_amd.envs import LbfConfig, RwareConfig
    from magpo_amd.q_learner import QLearner, QSystemConfig
    with pytest.raises(NotImplementedError, match="real_next_obs"):
        QLearner(RwareConfig(), 4, QSystemConfig(), "cpu")
    with pytest.raises(NotImplementedError, match="micro_batches"):
        QLearner(LbfConfig(), 4, QSystemConfig(micro_batches=2), "cpu")
    with pytest.raises(NotImplementedError, match="sample_sequence_length"):
        QLearner(LbfConfig(), 4, QSystemConfig(sample_sequence_length=9, buffer_size=8), "cpu")


# ----------------------------------------------------------------------------- the window sampler: ring 8, L = 4, N = 3
@pytest.mark.parametrize("adds", [5, 8, 11], ids=["before-wrap", "exactly-full", "after-wrap"])
def test_window_sampler_covers_every_valid_window_and_never_the_seam(adds):
    S, L_, N, B = 8, 4, 3, 16
    cursor, filled = adds % S, min(adds, S)
    n_valid = filled - L_ + 1
    oldest = cursor if filled == S else 0
    newest = (cursor - 1) % S
    seen = set()
    for seed in range(60):
        env_idx, start = ref.sample_indices(prng.prng_key(seed), B, L_, N, S, cursor, filled)
        assert env_idx.dtype == np.int32 and start.dtype == np.int32 and env_idx.shape == start.shape == (B,)
        for n, s0 in zip(env_idx.tolist(), start.tolist()):
            seen.add((n, s0))
            slots = [(s0 + i) % S for i in range(L_)]
            ages = [(x - oldest) % S for x in slots]            # steps since the oldest stored one
            assert ages == list(range(ages[0], ages[0] + L_)) and ages[-1] < filled, (adds, s0)   # stored steps, in time order
            assert all(not (a == newest and b == oldest) for a, b in zip(slots[:-1], slots[1:])), "a window contains the seam newest -> oldest"
    assert seen == {(n, (oldest + r) % S) for n in range(N) for r in range(n_valid)}
    with pytest.raises(ValueError):
        ref.sample_indices(prng.prng_key(0), B, L_, N, S, 3, 3)


def test_host_sampler_of_the_product_equals_the_restatement():
    """magpo_amd.q_learner.sample_window_indices (threefry host entry points) draws the restatement's indices bit for bit."""
    from magpo_amd.q_learner import sample_window_indices
    for seed, (N, S, L_, adds, B) in enumerate([(3, 8, 4, 5, 5), (3, 8, 4, 11, 7), (4096, 1000, 32, 40, 32), (16, 1000, 32, 2500, 32), (70000, 8, 2, 9, 9)]):
        key = prng.split(prng.prng_key(seed), 2)[1]
        want = ref.sample_indices(key, B, L_, N, S, adds % S, min(adds, S))
        got = sample_window_indices(key, B, L_, N, S, adds % S, min(adds, S))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), seed


def test_eps_schedule_in_float32():
    from magpo_amd.q_learner import epsilon
    f = np.float32
    eps_min, decay = 0.05, 1e5
    at_decay = f(f(1) - f(f(1) * f(f(1) - f(eps_min))))       # 1 - 0.95 in float32: one ulp above eps_min, so the maximum keeps it
    assert ref.epsilon(0, eps_min, decay) == f(1) and ref.epsilon(int(decay), eps_min, decay) == at_decay >= f(eps_min)
    assert ref.epsilon(2 * int(decay), eps_min, decay) == f(eps_min) and ref.epsilon(10 ** 9, eps_min, decay) == f(eps_min)
    assert ref.epsilon(50000, eps_min, decay) == f(f(1) - f(f(0.5) * f(f(1) - f(eps_min))))
    assert ref.epsilon(40, 0.0, 40.0) == f(0)
    for t in (0, 16, 50000, 100000, 300000):
        assert epsilon(t, eps_min, decay) == float(ref.epsilon(t, eps_min, decay))


# ----------------------------------------------------------------------------- no near ties at the GPU parity tests' seeds and shapes
@pytest.mark.parametrize("variant", list(ref.PARITY_VARIANTS))
@pytest.mark.parametrize("case", ref.PARITY_CASES, ids=[c[0] for c in ref.PARITY_CASES])
def test_parity_seeds_have_no_near_ties(case, variant):
    """The fp64 restatement over the update steps of tests/test_q_learner_gpu.py: no acting step and no double-Q selection whose two best
    legal Q values are closer than 1e-4, no eps-greedy sample whose two best perturbed log-probabilities are closer than 1e-4; the ring wraps,
    episodes end, training is skipped exactly while the ring cannot be sampled."""
    ol, _, info = ref.parity_case(case, variant, torch.float64)
    ended, infos_all = 0, []
    for _ in range(ref.PARITY_STEPS):
        metrics, infos = ol.update_step()
        ended += sum(int(m["is_terminal_step"].sum()) for m in metrics)
        infos_all += infos
    assert infos_all[:2] == [None, None] and all(i is not None for i in infos_all[2:])
    assert ended > 0 and all(g.ring.filled == 8 and g.ring.cursor == 0 for g in ol.groups)
    explored = 0
    for e in ol.log:
        q = e["q"].numpy()
        assert ref.top2_gap(q, e["mask"]).min() >= 1e-4, "acting step: near tie of the two best legal Q values"
        v = np.sort(ref.perturbed_log_probs(e["key"], ref.eps_greedy_probs(q.astype(np.float32), e["mask"], e["eps"])).astype(np.float64), axis=-1)
        finite = np.isfinite(v[..., -2])
        assert ((v[..., -1] - v[..., -2])[finite] >= 1e-4).all(), "eps-greedy sample: near tie of the two best perturbed log-probabilities"
        explored += int((e["action"] != ref.greedy_action(q, e["mask"])).sum())
    assert explored > 0, "eps must make some action non-greedy"
    terminal_rows = 0
    for tl in ol.train_log:
        for det in tl["details"]:
            assert ref.top2_gap(det["qn_online"].numpy(), None if det["next_mask"] is None else det["next_mask"].numpy()).min() >= 1e-4, \
                "double-Q selection: near tie"
            terminal_rows += int(det["rows"]["next_terminal"].sum())
    assert terminal_rows > 0, "sampled windows must contain terminal steps"
