"""MPE simple_spread without a GPU: the env factory (configs/env/mpe.yaml + scenario/simple_spread_*.yaml), the numpy restatement
tests/mpe_ref.py on hand-built states (the rules the GPU kernel csrc/mpe.hip is checked against bit for bit), and the kernel's resources."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import prng
from tests import mpe_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compose(*over):
    from magpo_amd.config import compose
    return compose("rec_magpo", ["env=mpe", *over])


@pytest.mark.parametrize("scenario,A,F", [("simple_spread_3ag", 3, 21), ("simple_spread_5ag", 5, 35), ("simple_spread_10ag", 10, 70)])
def test_mpe_factory(scenario, A, F):
    from magpo_amd.learner import MpeConfig, obs_row_stride
    from magpo_amd.utils import make_env as environments
    env, eval_env = environments.make(_compose(f"env/scenario={scenario}", "env.kwargs.action_type=Discrete"))
    for e in (env, eval_env):
        assert (e.num_agents, e.action_dim, e.obs_dim, e.time_limit) == (A, 5, F, 25)
        assert e.observation_spec.agents_view.shape == (A, F) and e.reward_spec.shape == (A,)
    assert env.auto_reset and not eval_env.auto_reset
    cfg = env.unwrapped
    assert isinstance(cfg, MpeConfig) and (cfg.num_agents, cfg.num_landmarks, cfg.local_ratio) == (A, A, 0.5)
    assert not cfg.has_mask and not cfg.class_tables and cfg.obs_dim == F == M.MpeSpec(A, A).obs_dim
    assert obs_row_stride(F) == (F if A == 3 else 128)


def test_mpe_factory_rejects():
    from magpo_amd.utils import make_env as environments
    with pytest.raises(NotImplementedError, match="env.kwargs.action_type=Discrete"):   # the reference's default action type
        environments.make(_compose())
    with pytest.raises(ValueError):
        environments.make(_compose("env.kwargs.action_type=Bogus"))
    with pytest.raises(NotImplementedError):
        environments.make(_compose("env.kwargs.action_type=Discrete", "+env.kwargs.dt=0.05"))
    with pytest.raises(ValueError):
        environments.make(_compose("env.kwargs.action_type=Discrete", "env.scenario.task_config.num_agents=33"))
    with pytest.raises(ValueError):
        environments.make(_compose("env.kwargs.action_type=Discrete", "env.scenario.task_config.num_landmarks=0"))
    with pytest.raises(NotImplementedError):   # 5 * 20 + 2 * 20 floats per observation row > 128
        environments.make(_compose("env.kwargs.action_type=Discrete", "env.scenario.task_config.num_agents=20",
                                   "env.scenario.task_config.num_landmarks=20"))
    env, _ = environments.make(_compose("env.kwargs.action_type=Discrete", "env.scenario.task_config.num_agents=16",
                                        "env.scenario.task_config.num_landmarks=24"))
    assert env.obs_dim == 128


def test_mpe_without_agent_id():
    from magpo_amd.utils import make_env as environments
    cfg = _compose("env.kwargs.action_type=Discrete", "system.add_agent_id=False")
    env, eval_env = environments.make(cfg)
    assert env.obs_dim == eval_env.obs_dim == 18 and cfg.system.add_agent_id is False
    with pytest.raises(NotImplementedError):   # 70-float rows are padded to 128 and cannot be read behind the one-hot id
        environments.make(_compose("env/scenario=simple_spread_10ag", "env.kwargs.action_type=Discrete", "system.add_agent_id=False"))


def _state(pos, vel=None, A=None):
    """A batch of restatement states from positions [N][A+L][2] (velocities 0 unless given)."""
    pos = np.asarray(pos, np.float32)
    n = pos.shape[0]
    vel = np.zeros((n, A, 2), np.float32) if vel is None else np.asarray(vel, np.float32)
    return dict(pos=pos, vel=vel, inner_step=np.zeros(n, np.int32), step_count=np.zeros(n, np.int32), key=np.zeros((n, 2), np.uint32),
                metrics_key=np.zeros((n, 2), np.uint32), running_return=np.zeros(n, np.float32), running_length=np.zeros(n, np.int32),
                episode_return=np.zeros(n, np.float32), episode_length=np.zeros(n, np.int32))


def test_reset_ranges_and_key_chain():
    spec = M.MpeSpec(5, 4)
    keys = prng.split(prng.prng_key(3), 64)
    st, ts = M.reset(spec, keys)
    pa, pl = st["pos"][:, :5], st["pos"][:, 5:]
    assert (pa >= -1).all() and (pa < 1).all() and (pl >= np.float32(-0.9)).all() and (pl < np.float32(0.9)).all()
    assert (st["vel"] == 0).all() and (st["inner_step"] == 0).all() and (st["step_count"] == 0).all()
    assert pa.std() > 0.4 and pl.std() > 0.35
    # RecordEpisodeMetrics: metrics_key, reset_key = split(key); JaxMarlWrapper: key, inner_key = split(reset_key); SimpleMPE: key_a, key_l
    mk, rk = prng.split(keys, 2)[:, 0], prng.split(keys, 2)[:, 1]
    wk, ik = prng.split(rk, 2)[:, 0], prng.split(rk, 2)[:, 1]
    ka, kl = prng.split(ik, 2)[:, 0], prng.split(ik, 2)[:, 1]
    assert np.array_equal(st["metrics_key"], mk) and np.array_equal(st["key"], wk)
    assert np.array_equal(pa.reshape(64, -1), prng.uniform(ka, 10, -1.0, 1.0))
    assert np.array_equal(pl.reshape(64, -1), prng.uniform(kl, 8, -0.9, 0.9))
    # step: key, step_key = split(state.key)
    st1, _ = M.step(spec, st, np.zeros((64, 5), np.int32))
    assert np.array_equal(st1["key"], prng.split(wk, 2)[:, 0]) and np.array_equal(st1["metrics_key"], mk)
    # auto-reset after the last step: key, _ = split(state.key) (the key that step stored), then the wrapper's reset on it
    st = st1
    for _ in range(spec.time_limit):
        prev = st["key"]
        st, ts = M.step(spec, st, np.zeros((64, 5), np.int32))
    assert ts["step_type"].tolist() == [M.STEP_LAST] * 64
    k = prng.split(prng.split(prev, 2)[:, 0], 2)[:, 0]       # this step's key, then the auto-reset's split
    fresh = M.wrapper_reset(spec, k)
    for f in ("pos", "vel", "inner_step", "step_count", "key"):
        assert np.array_equal(st[f], fresh[f]), f
    # the eval env resets only the inner env, from key_reset = split(step_key)[1], and keeps the wrapper's counter
    se = st1
    for _ in range(spec.time_limit):
        prev = se["key"]
        se, ts = M.step(spec, se, np.zeros((64, 5), np.int32), auto_reset=False)
    inner = M.inner_reset(spec, prng.split(prng.split(prev, 2)[:, 1], 2)[:, 1])
    for f in ("pos", "vel", "inner_step"):
        assert np.array_equal(se[f], inner[f]), f
    assert (se["step_count"] == spec.time_limit + 1).all() and np.array_equal(se["key"], prng.split(prev, 2)[:, 0])


def test_landmarks_never_move_and_observation_layout():
    spec = M.MpeSpec(4, 3)
    st, ts = M.reset(spec, prng.split(prng.prng_key(9), 16))
    land = st["pos"][:, 4:].copy()
    rng = np.random.default_rng(1)
    for t in range(spec.time_limit):
        st, ts = M.step(spec, st, rng.integers(0, 5, (16, 4)), auto_reset=False)
        assert np.array_equal(st["pos"][:, 4:], land), t
        ob = ts["observation"]["agents_view"]
        assert ob.shape == (16, 4, 4 + 4 + 6 + 12)
        assert np.array_equal(ob[:, :, :4], np.broadcast_to(np.eye(4, dtype=np.float32), (16, 4, 4)))
        f = ob[:, :, 4:]
        assert np.array_equal(f[:, :, 0:2], st["vel"]) and np.array_equal(f[:, :, 2:4], st["pos"][:, :4])
        for i in range(4):
            p = st["pos"][:, i]
            assert np.array_equal(f[:, i, 4:10].reshape(16, 3, 2), land - p[:, None])
            others = [j for j in range(4) if j != i]
            assert np.array_equal(f[:, i, 10:16].reshape(16, 3, 2), st["pos"][:, others] - p[:, None])
        assert (f[:, :, 16:] == 0).all(), "silent agents: comm columns are zero"
        assert (ts["observation"]["action_mask"]).all()


def test_contact_forces_equal_and_opposite():
    pi, pj = np.array([[0.1, -0.2]], np.float32), np.array([[0.31, -0.05]], np.float32)   # 0.258 apart: touching (< 0.3)
    fij, fji = M.pair_force(pi, pj), M.pair_force(pj, pi)
    assert np.abs(fij).max() > 1.0 and np.array_equal(fij, -fji)
    # far apart: the soft-plus underflows and the force is exactly zero
    assert (M.pair_force(pi, np.array([[0.9, 0.6]], np.float32)) == 0).all()
    spec = M.MpeSpec(2, 1)
    pos = np.array([[[0.1, -0.2], [0.31, -0.05], [0.5, 0.5]]], np.float32)
    f = M.forces(spec, pos, np.zeros((1, 2, 2), np.float32))
    assert np.array_equal(f[0, 0], -f[0, 1]) and np.array_equal(f[0, 0], fij[0])
    # actions add after the contact forces; the push separates the pair (velocity along p_i - p_j)
    st = _state(pos, A=2)
    st2, _ = M.step(spec, st, np.array([[0, 0]]))
    d0 = pos[0, 0] - pos[0, 1]
    assert np.dot(st2["vel"][0, 0], d0) > 0 and np.dot(st2["vel"][0, 1], d0) < 0
    assert np.array_equal(st2["pos"][0, :2], pos[0, :2]), "positions move by the pre-step velocity (zero) first"


def test_action_decoding_and_integration():
    spec = M.MpeSpec(1, 1)
    pos = np.array([[[0.0, 0.0], [0.5, 0.5]]] * 6, np.float32)
    vel = np.array([[[0.2, -0.4]]] * 6, np.float32)
    st2, _ = M.step(spec, _state(pos, vel, A=1), np.array([[0], [1], [2], [3], [4], [7]]))
    u = np.array([[0, 0], [-5, 0], [5, 0], [0, -5], [0, 5], [0, 0]], np.float32)
    assert np.array_equal(st2["pos"][:, 0], (pos[:, 0] + vel[:, 0] * np.float32(0.1)).astype(np.float32))
    want = (vel[:, 0] * np.float32(0.75) + u * np.float32(0.1)).astype(np.float32)
    assert np.array_equal(st2["vel"][:, 0], want)


def test_reward_by_hand():
    """Agents 0 and 1 overlap (0.25 apart), agent 2 sits on landmark 1; landmark 0 is 0.5 from agent 0 (its nearest agent).
    global = -(0.5 + 0) = -0.5; agents 0 and 1 each collide once: 0.5 * -1 + 0.5 * -0.5 = -0.75; agent 2: 0.5 * -0.5 = -0.25."""
    spec = M.MpeSpec(3, 2, local_ratio=0.5)
    pos = np.array([[[0.0, 0.0], [0.25, 0.0], [1.0, 1.0], [0.0, 0.5], [1.0, 1.0]]], np.float32)
    r, coll = M.rewards(spec, pos)
    assert coll.tolist() == [[1, 1, 0]]
    assert r.tolist() == [[-0.75, -0.75, -0.25]]
    r2, _ = M.rewards(M.MpeSpec(3, 2, local_ratio=0.25), pos)
    assert np.allclose(r2, [[-0.25 - 0.375, -0.25 - 0.375, -0.375]])


def test_episode_length_and_step_count():
    """The CHOICE for the open point: done tests the inner counter before its increment, so an episode lasts time_limit + 1 = 26 steps;
    observation.step_count is the wrapper's counter before its increment: 0 at the reset, then 0, 0, 1, ..., 24 and 0 again."""
    spec = M.MpeSpec(3, 3)
    st, ts = M.reset(spec, prng.split(prng.prng_key(4), 4))
    seen, lens, ends = [int(ts["observation"]["step_count"][0, 0])], [], []
    for t in range(3 * (spec.time_limit + 1)):
        st, ts = M.step(spec, st, np.ones((4, 3), np.int32))
        seen.append(int(ts["observation"]["step_count"][0, 0]))
        if ts["step_type"][0] == M.STEP_LAST:
            ends.append(t + 1)
            lens.append(int(ts["episode_metrics"]["episode_length"][0]))
            assert (ts["discount"] == 0).all()
        else:
            assert (ts["discount"] == 1).all()
    assert ends == [26, 52, 78] and lens == [26, 26, 26]
    assert seen[:27] == [0, 0] + list(range(1, 25)) + [0]
    assert seen[27:29] == [0, 1]
    # the eval env keeps counting past the end
    st, ts = M.reset(spec, prng.split(prng.prng_key(4), 4))
    for _ in range(27):
        st, ts = M.step(spec, st, np.zeros((4, 3), np.int32), auto_reset=False)
    assert ts["observation"]["step_count"][0, 0] == 26 and ts["step_type"][0] == M.STEP_MID


def test_episode_return_is_the_mean_over_agents():
    spec = M.MpeSpec(3, 3)
    st, ts = M.reset(spec, prng.split(prng.prng_key(5), 8))
    rng = np.random.default_rng(2)
    total = np.zeros(8, np.float32)
    for _ in range(spec.time_limit + 1):
        st, ts = M.step(spec, st, rng.integers(0, 5, (8, 3)))
        r = ts["reward"]
        total = (total + ((r[:, 0] + r[:, 1]) + r[:, 2]) / np.float32(3)).astype(np.float32)
    assert np.array_equal(ts["episode_metrics"]["episode_return"], total)
    assert ts["episode_metrics"]["is_terminal_step"].all() and (st["running_return"] == 0).all()


def test_mpe_kernels_use_no_scratch(tmp_path):
    """csrc/mpe.hip keeps its runtime-indexed entity arrays in LDS: the compiler's resource report shows no scratch."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wno-unused-value", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(ROOT, "magpo_amd", "csrc", "mpe.hip"), "-o", str(tmp_path / "mpe.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    scratch, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            scratch[cur] = int(m.group(1))
    kernels = {k: v for k, v in scratch.items() if "k_mpe_reset" in k or "k_mpe_step" in k}
    assert len(kernels) == 2 and all(v == 0 for v in kernels.values()), scratch
