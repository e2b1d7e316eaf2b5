"""MPE simple_spread (discrete actions) + Mava wrapper stack, batched numpy restatement (test infrastructure only; the product never
imports it).

Same contract as tests/connector_ref.py -- ``reset(spec, keys)`` / ``step(spec, state, actions, auto_reset)`` and the same timestep dict --
so that it plugs into oracle.learner.OracleLearner(..., env=...) and oracle.evaluator.evaluate(..., env=...) unchanged.

Wrapper order (mava/utils/make_env.py:90-104,138-170):
  RecordEpisodeMetrics (wrappers/episode_metrics.py:60-112)
    -> AutoResetWrapper (wrappers/auto_reset_wrapper.py:60-101)      [train env only]
      -> AgentIDWrapper (wrappers/observation.py:42-54: eye(A) in front of every row)
        -> MPEWrapper / JaxMarlWrapper (wrappers/jaxmarl.py:169-243,424-455)
          -> JaxMARL MPE_simple_spread_v3(num_agents, num_landmarks, local_ratio, action_type="Discrete")

PINNED by the reference tree:
  * keys: reset: key, reset_key = split(key) (RecordEpisodeMetrics), then key, reset_key = split(reset_key) (JaxMarlWrapper.reset; the
    state keeps key) and the inner reset on reset_key.  step: key, step_key = split(state.key); the inner step on step_key.  auto-reset:
    key, _ = split(state.key) (the key the step just stored), then the wrapper's reset on it.
  * rewards: one per agent (batchify), no aggregation; discount 1 - done, so 0 at the time limit (jaxmarl.py:237).
  * observation.step_count: 0 at a reset, else the wrapper's counter BEFORE its increment (jaxmarl.py:231,241): a training episode reads
    0, 0, 1, 2, ... and returns to 0 at the auto-reset.  The eval env (no auto-reset) keeps counting past the episode end.
  * action mask all ones (MPEWrapper.action_mask).
  * episode_return += mean over agents of the rewards (episode_metrics.py:91), here a sum in agent order divided by A in fp32.

UNPINNED DYNAMICS.  JaxMARL is third-party and absent from the reference tree; its MPE is restated here from memory (csrc/mpe.hip restates
the same rules and agrees bit for bit):
  * reset(key): key_a, key_l = split(key); agent positions uniform(key_a, (A, 2), -1, 1), landmark positions uniform(key_l, (L, 2), -0.9,
    0.9); velocities 0; the inner step counter 0.  Communication is all zeros (silent agents, dim_c = 2).
  * discrete action (_decode): 0 no-op; 1 / 2 = -x / +x; 3 / 4 = -y / +y; the chosen axis gets +-1 times accel 5.  Anything outside
    0..4 acts as a no-op.
  * world step: agents have radius 0.15, landmarks 0.05; only agents collide.  The contact force on agent i from agent j != i is
    contact_force * (p_i - p_j) / |p_i - p_j| * softplus(-(|p_i - p_j| - (r_i + r_j)) / k) * k with contact_force 100, k = 1e-3, fp32
    left to right; the forces are summed over j in index order (from 0) and the action force added last.  Then p += v * dt,
    v *= (1 - damping), v += F / m * dt with dt 0.1, damping 0.25, m 1, no speed cap.  Landmarks never move.
  * reward of agent i, on the post-step state: local_ratio * (-#{j != i : |p_i - p_j| < r_i + r_j}) + (1 - local_ratio) * G with
    G = sum over landmarks in index order (from 0) of -min over agents |p_a - p_l|; (1 - local_ratio) is evaluated in fp32.
  * observation of agent i: [v_i, p_i, p_l - p_i for every landmark, p_j - p_i for every other agent in index order (self skipped),
    comm of every other agent (zeros)]: 4 + 2 L + 4 (A - 1) floats behind the one-hot id.
  * episode end: done for every agent when the inner step counter, tested BEFORE its increment, is >= max_steps (time_limit 25).  This
    is the recalled form; the alternative (after the increment) would end episodes one step earlier.  OPEN POINT, CHOICE: episodes last
    time_limit + 1 = 26 steps (pinned by tests/test_mpe.py::test_episode_length).  On done the inner env resets itself
    (MultiAgentEnv.step) from key_reset = split(step_key)[1] and returns that state's observation; the train env's auto-reset then
    overwrites both, the eval env continues from them.

Numerics: every operation is fp32 and rounded on its own (no fused multiply-add); division and square root are correctly rounded; the
soft-plus is the one transcendental and is evaluated in fp64 as max(x, 0) + log1p(exp(-|x|)), rounded once to fp32 -- a sub-ulp deviation
from JaxMARL's fp32 logaddexp.  Every sum runs in the fixed order stated above (explicit loops, never np.sum).
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from oracle import prng

STEP_FIRST, STEP_MID, STEP_LAST = 0, 1, 2
NUM_ACTIONS = 5
DIM_C = 2
F32 = np.float32
AGENT_RADIUS, LANDMARK_RADIUS = F32(0.15), F32(0.05)
ACCEL, DT, DAMPING, MASS, CONTACT_FORCE, CONTACT_MARGIN = F32(5.0), F32(0.1), F32(0.25), F32(1.0), F32(100.0), F32(1e-3)


class MpeSpec:
    def __init__(self, num_agents=3, num_landmarks=3, local_ratio=0.5, time_limit=25):
        self.num_agents, self.num_landmarks = int(num_agents), int(num_landmarks)
        self.local_ratio, self.time_limit = float(local_ratio), int(time_limit)
        self.num_actions = NUM_ACTIONS

    @property
    def obs_dim(self) -> int:   # 4 + 2 L + (2 + dim_c) (A - 1) features + one-hot agent id (AgentIDWrapper)
        return 4 + 2 * self.num_landmarks + (2 + DIM_C) * (self.num_agents - 1) + self.num_agents


def _uniform(keys: np.ndarray, n: int, lo: float, hi: float) -> np.ndarray:
    return prng.uniform(keys, n, lo, hi)


def inner_reset(spec: MpeSpec, keys: np.ndarray) -> Dict[str, np.ndarray]:
    """SimpleMPE.reset for a batch of keys [N][2]: pos [N][A+L][2], vel [N][A][2], inner_step [N]."""
    A, L = spec.num_agents, spec.num_landmarks
    ks = prng.split(keys, 2)
    n = keys.shape[0]
    pa = _uniform(ks[:, 0, :], 2 * A, -1.0, 1.0).reshape(n, A, 2)
    pl = _uniform(ks[:, 1, :], 2 * L, -0.9, 0.9).reshape(n, L, 2)
    return dict(pos=np.concatenate([pa, pl], axis=1).astype(F32), vel=np.zeros((n, A, 2), F32), inner_step=np.zeros(n, np.int32))


def wrapper_reset(spec: MpeSpec, keys: np.ndarray) -> Dict[str, np.ndarray]:
    """JaxMarlWrapper.reset: key, reset_key = split(key); the inner reset on reset_key; the wrapper's counter at 0."""
    ks = prng.split(keys, 2)
    core = inner_reset(spec, ks[:, 1, :])
    core.update(step_count=np.zeros(keys.shape[0], np.int32), key=ks[:, 0, :].copy())
    return core


def decode(actions: np.ndarray) -> np.ndarray:
    """Discrete actions [N][A] -> accelerations [N][A][2] (the one function a continuous-action variant would replace)."""
    a = np.asarray(actions, np.int32)
    valid = (a >= 1) & (a < NUM_ACTIONS)
    sign = np.where(a % 2 == 0, F32(1.0), F32(-1.0)).astype(F32)
    u = np.zeros(a.shape + (2,), F32)
    u[..., 0] = np.where(valid & (a <= 2), sign * ACCEL, F32(0.0))
    u[..., 1] = np.where(valid & (a > 2), sign * ACCEL, F32(0.0))
    return u


def softplus(x: np.ndarray) -> np.ndarray:
    """fp64 max(x, 0) + log1p(exp(-|x|)), rounded once to fp32."""
    d = np.asarray(x, F32).astype(np.float64)
    return (np.maximum(d, 0.0) + np.log1p(np.exp(-np.abs(d)))).astype(F32)


def dist(dx: np.ndarray, dy: np.ndarray) -> np.ndarray:
    return np.sqrt((dx * dx + dy * dy).astype(F32)).astype(F32)


def pair_force(pi: np.ndarray, pj: np.ndarray) -> np.ndarray:
    """Contact force on an agent at pi from an agent at pj ([..., 2] each)."""
    dx, dy = (pi[..., 0] - pj[..., 0]).astype(F32), (pi[..., 1] - pj[..., 1]).astype(F32)
    d = dist(dx, dy)
    with np.errstate(divide="ignore", invalid="ignore"):
        pen = (softplus(-(d - (AGENT_RADIUS + AGENT_RADIUS)) / CONTACT_MARGIN) * CONTACT_MARGIN).astype(F32)
        fx = ((CONTACT_FORCE * dx) / d * pen).astype(F32)
        fy = ((CONTACT_FORCE * dy) / d * pen).astype(F32)
    return np.stack([fx, fy], axis=-1)


def forces(spec: MpeSpec, pos: np.ndarray, u: np.ndarray) -> np.ndarray:
    """Total force on every agent [N][A][2]: contact forces summed over the other agents in index order, then the action force."""
    A = spec.num_agents
    f = np.zeros(u.shape, F32)
    for i in range(A):
        for j in range(A):
            if j != i:
                f[:, i] = (f[:, i] + pair_force(pos[:, i], pos[:, j])).astype(F32)
    return (f + u).astype(F32)


def rewards(spec: MpeSpec, pos: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(per-agent rewards [N][A], collision counts [N][A]) on the given positions."""
    A, L = spec.num_agents, spec.num_landmarks
    N = pos.shape[0]
    g = np.zeros(N, F32)
    for l in range(L):
        lp = pos[:, A + l]
        best = np.full(N, np.inf, F32)
        for a in range(A):
            best = np.minimum(best, dist((pos[:, a, 0] - lp[:, 0]).astype(F32), (pos[:, a, 1] - lp[:, 1]).astype(F32)))
        g = (g + (-best)).astype(F32)
    coll = np.zeros((N, A), np.int32)
    rmin = AGENT_RADIUS + AGENT_RADIUS
    for i in range(A):
        for j in range(A):
            if j != i:
                coll[:, i] += dist((pos[:, i, 0] - pos[:, j, 0]).astype(F32), (pos[:, i, 1] - pos[:, j, 1]).astype(F32)) < rmin
    lr = F32(spec.local_ratio)
    glr = F32(1.0) - lr
    r = ((-coll).astype(F32) * lr + g[:, None] * glr).astype(F32)
    return r, coll


def world_step(spec: MpeSpec, pos: np.ndarray, vel: np.ndarray, actions: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """SimpleMPE._world_step: (new pos [N][A+L][2], new vel [N][A][2])."""
    A = spec.num_agents
    f = forces(spec, pos, decode(actions))
    pos = pos.copy()
    pos[:, :A] = (pos[:, :A] + vel * DT).astype(F32)
    vel = (vel * (F32(1.0) - DAMPING)).astype(F32)
    vel = (vel + (f / MASS) * DT).astype(F32)
    return pos, vel


def _observe(spec: MpeSpec, pos: np.ndarray, vel: np.ndarray) -> np.ndarray:
    """SimpleSpreadMPE.get_obs of every agent, batched: [N][A][4 + 2 L + 4 (A - 1)] fp32."""
    A, L = spec.num_agents, spec.num_landmarks
    N = pos.shape[0]
    out = np.zeros((N, A, spec.obs_dim - A), F32)
    for i in range(A):
        p = pos[:, i]
        cols = [vel[:, i], p] + [pos[:, A + l] - p for l in range(L)] + [pos[:, j] - p for j in range(A) if j != i]
        row = np.concatenate(cols, axis=1).astype(F32)
        out[:, i, :row.shape[1]] = row   # the comm columns stay zero
    return out


def make_obs(spec: MpeSpec, st: Dict[str, np.ndarray], obs_step: np.ndarray) -> Dict[str, np.ndarray]:
    """MPEWrapper observation + AgentIDWrapper (one-hot id in front); ``obs_step`` [N] is observation.step_count."""
    N, A = st["pos"].shape[0], spec.num_agents
    ids = np.broadcast_to(np.eye(A, dtype=F32)[None], (N, A, A))
    return dict(agents_view=np.concatenate([ids, _observe(spec, st["pos"], st["vel"])], axis=-1),
                action_mask=np.ones((N, A, NUM_ACTIONS), bool),
                step_count=np.repeat(np.asarray(obs_step, np.int32)[:, None], A, axis=1))


_CORE = ("pos", "vel", "inner_step", "step_count", "key")


def reset(spec: MpeSpec, env_keys: np.ndarray) -> Tuple[Dict, Dict]:
    env_keys = np.asarray(env_keys, np.uint32)
    ks = prng.split(env_keys, 2)   # key (kept, unused), reset_key  (episode_metrics.py:62)
    core = wrapper_reset(spec, ks[:, 1, :])
    n, a = env_keys.shape[0], spec.num_agents
    state = dict(core, metrics_key=ks[:, 0, :].copy(), running_return=np.zeros(n, F32), running_length=np.zeros(n, np.int32),
                 episode_return=np.zeros(n, F32), episode_length=np.zeros(n, np.int32))
    timestep = dict(step_type=np.full(n, STEP_FIRST, np.int8), reward=np.zeros((n, a), F32), discount=np.ones((n, a), F32),
                    observation=make_obs(spec, core, np.zeros(n, np.int32)),
                    episode_metrics=dict(episode_return=np.zeros(n, F32), episode_length=np.zeros(n, np.int32),
                                         is_terminal_step=np.zeros(n, bool)))
    return state, timestep


def step(spec: MpeSpec, state: Dict, actions: np.ndarray, auto_reset: bool = True) -> Tuple[Dict, Dict]:
    actions = np.asarray(actions, np.int32)
    N, A = actions.shape[0], spec.num_agents
    ks = prng.split(state["key"], 2)   # key, step_key = split(state.key)
    pos, vel = world_step(spec, state["pos"], state["vel"], actions)
    reward, _ = rewards(spec, pos)
    done = state["inner_step"] >= spec.time_limit   # tested before the increment: time_limit + 1 steps
    obs_step = state["step_count"].astype(np.int32).copy()
    core = dict(pos=pos, vel=vel, inner_step=(state["inner_step"] + 1).astype(np.int32), step_count=(state["step_count"] + 1).astype(np.int32),
                key=ks[:, 0, :].copy())
    if done.any():
        idx = np.nonzero(done)[0]
        if auto_reset:   # auto_reset_wrapper.py:60-83: key, _ = split(state.key); the wrapper's reset on it; reward etc. kept
            fresh = wrapper_reset(spec, prng.split(core["key"][idx], 2)[:, 0, :])
            obs_step[idx] = 0
        else:            # MultiAgentEnv.step: key, key_reset = split(step_key); the inner env resets itself on done
            fresh = inner_reset(spec, prng.split(ks[idx, 1, :], 2)[:, 1, :])
        for k, v in fresh.items():
            core[k][idx] = v
    discount = np.repeat(np.where(done, 0.0, 1.0).astype(F32)[:, None], A, axis=1)
    not_done = (~done).astype(F32)
    msum = np.zeros(N, F32)
    for i in range(A):
        msum = (msum + reward[:, i]).astype(F32)
    new_ret = (state["running_return"] + msum / F32(A)).astype(F32)   # episode_metrics.py:91-96
    new_len = state["running_length"] + 1
    ep_ret = np.where(done, new_ret, state["episode_return"]).astype(F32)
    ep_len = np.where(done, new_len, state["episode_length"]).astype(np.int32)
    new_state = dict(core, metrics_key=state["metrics_key"], running_return=(new_ret * not_done).astype(F32),
                     running_length=np.where(done, 0, new_len).astype(np.int32), episode_return=ep_ret, episode_length=ep_len)
    timestep = dict(step_type=np.where(done, STEP_LAST, STEP_MID).astype(np.int8), reward=reward, discount=discount,
                    observation=make_obs(spec, core, obs_step),
                    episode_metrics=dict(episode_return=ep_ret, episode_length=ep_len, is_terminal_step=done.copy()))
    return new_state, timestep
