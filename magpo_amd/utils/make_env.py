"""Environment factory (mava/utils/make_env.py:202-218, 288-315): config -> (train_env, eval_env) descriptors.

CoordSum (csrc/coordsum.hip), Level-Based Foraging (csrc/lbf.hip), Robot Warehouse (csrc/rware.hip), VectorConnector
(csrc/connector.hip) and MPE simple_spread with discrete actions (csrc/mpe.hip) are implemented.  LBF / RWARE / Connector dynamics live in
third-party Jumanji and MPE's in JaxMARL, both absent from the reference tree and from this image: all four are restated from the published
algorithms with UNPINNED dynamics (oracle/lbf.py, oracle/rware.py, tests/connector_ref.py and tests/mpe_ref.py list every rule).  The
grid-observation ``Connector`` (ConnectorWrapper) and MPE's continuous actions are not supported.  The wrapper stack the five kernels share
is csrc/env_wrappers.hpp; the configs and the device-resident batches are magpo_amd/envs.py.
"""
from __future__ import annotations

from functools import cached_property
from typing import Tuple

import numpy as np
import torch

from .. import specs
from ..envs import CoordSumConfig, LbfConfig, MpeConfig, RwareConfig, VectorConnectorConfig, make_env_batch, net_obs, obs_row_stride
from ..types import Observation, TimeStep

COORDSUM_REGISTRY = {  # mava/coordsum/__init__.py:6-45
    "5x20-80-v0": dict(num_agents=5, num_actions=20, time_limit=100, maxval=80),
    "3x30-50-v0": dict(num_agents=3, num_actions=30, time_limit=100, maxval=50),
    "3x10-30-v0": dict(num_agents=3, num_actions=10, time_limit=100, maxval=30),
    "8x15-100-v0": dict(num_agents=8, num_actions=15, time_limit=100, maxval=100),
}


class EnvState:
    """State of a batch of wrapped envs (the reference's vmapped State pytree: inner env state + RecordEpisodeMetricsState counters):
    ``fields`` are the device tensors named by the env's ``state_fields`` (leading env axis).  ``MarlEnv.step`` updates them IN PLACE
    and returns the same object -- the donated-buffer form of ``state -> new_state`` (the kernels own the env's auto-reset branch, so a
    step is one launch over the whole batch)."""

    def __init__(self, batch):
        self.batch = batch

    @property
    def fields(self):
        return {f: getattr(self.batch, f) for f in self.batch.state_fields}

    def __getattr__(self, name):   # state.key, state.step_count ... like the reference's State dataclasses
        batch = object.__getattribute__(self, "batch")
        if name in batch.state_fields:
            return getattr(batch, name)
        raise AttributeError(name)


class MarlEnv:
    """The env API the system file, the learner set-up and the evaluator use (mava/types.py:45-123 ``MarlEnv``): ``num_agents`` /
    ``time_limit`` / ``action_dim``, ``reset(key) -> (state, timestep)``, ``step(state, action) -> (state, timestep)``,
    ``observation_spec`` / ``action_spec`` / ``reward_spec`` / ``discount_spec`` and ``unwrapped`` -- driving the HIP env kernels
    (csrc/coordsum.hip, lbf.hip, rware.hip, connector.hip, mpe.hip), which implement the whole wrapper stack of mava/utils/make_env.py:90-104
    (env wrapper -> AgentIDWrapper -> AutoResetWrapper [train env] -> RecordEpisodeMetrics).

    The batch axis is explicit: the reference calls ``jax.vmap(env.reset)(keys)`` / ``jax.vmap(env.step)(state, action)``; here
    ``reset`` takes the ``[N, 2]`` key array itself (a single ``[2]`` key = one env) and ``step`` the ``[N, A]`` actions, one kernel
    launch per call.  ``extras`` carries ``episode_metrics`` and (empty) ``env_metrics``; the auto-reset wrapper's ``real_next_obs``
    entry is not produced (nothing on the MAGPO path reads it)."""

    def __init__(self, cfg, auto_reset: bool, add_agent_id: bool = True, device=None):
        self.cfg, self.auto_reset, self.add_agent_id, self.device = cfg, bool(auto_reset), bool(add_agent_id), device

    # ---- attributes (mava/types.py:53-55)
    @property
    def num_agents(self) -> int:
        return self.cfg.num_agents

    @property
    def action_dim(self) -> int:
        return self.cfg.num_actions

    @property
    def time_limit(self) -> int:
        return self.cfg.time_limit

    @property
    def obs_dim(self) -> int:
        """Width of ``agents_view`` as the networks see it: with the AgentIDWrapper's one-hot id, or (system.add_agent_id: False) without."""
        return net_obs(self.cfg)[0]

    @property
    def unwrapped(self):
        return self.cfg

    # ---- specs (per env, no batch axis)
    @cached_property
    def observation_spec(self) -> specs.Spec:
        A, K, F = self.num_agents, self.action_dim, self.obs_dim
        return specs.Spec(Observation, "ObservationSpec",
                          agents_view=specs.Array((A, F), np.float32, "agents_view"),
                          action_mask=specs.BoundedArray((A, K), bool, False, True, "action_mask"),
                          step_count=specs.BoundedArray((A,), np.int32, 0, self.time_limit, "step_count"))

    @cached_property
    def action_spec(self) -> specs.MultiDiscreteArray:
        return specs.MultiDiscreteArray(num_values=np.full(self.num_agents, self.action_dim, np.int32), name="action")

    @cached_property
    def reward_spec(self) -> specs.Array:
        return specs.Array((self.num_agents,), np.float32, "reward")

    @cached_property
    def discount_spec(self) -> specs.BoundedArray:
        return specs.BoundedArray((self.num_agents,), np.float32, 0.0, 1.0, "discount")

    # ---- dynamics
    def _dev(self):
        return self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())

    def _timestep(self, st: EnvState, step_type, reward, discount, obs, obs_step, mask, m_ret, m_len, m_term) -> TimeStep:
        N, A, K, F = obs.shape[0], self.num_agents, self.action_dim, self.obs_dim
        if mask is None:   # CoordSum: every action legal (matrax.py:117-134)
            if getattr(st, "_ones", None) is None or st._ones.shape[0] != N:
                st._ones = torch.ones(N, A, K, dtype=torch.uint8, device=obs.device)
            mask = st._ones
        off = net_obs(self.cfg)[1]     # the env kernels always write [one-hot id | features]: without the id the view starts behind it
        observation = Observation(obs[..., off:off + F], mask, obs_step.view(N, 1).expand(N, A))
        extras = {"episode_metrics": {"episode_return": m_ret, "episode_length": m_len, "is_terminal_step": m_term.bool()}, "env_metrics": {}}
        return TimeStep(step_type, reward, discount, observation, extras)

    def reset(self, key) -> Tuple[EnvState, TimeStep]:
        """``key``: [N, 2] (or [2]) uint32 keys, numpy or device tensor -- what the reference passes to ``jax.vmap(env.reset)``
        (rec_magpo.py:642-653, evaluator.py:128-130)."""
        dev = self._dev()
        if not torch.is_tensor(key):
            key = torch.from_numpy(np.ascontiguousarray(key, dtype=np.uint32).reshape(-1, 2).view(np.int32).copy())
        keys = key.reshape(-1, 2).to(dev).contiguous()
        N, A = keys.shape[0], self.num_agents
        batch = make_env_batch(self.cfg, N, dev)
        st = EnvState(batch)
        ld = obs_row_stride(self.cfg.obs_dim)
        obs = torch.zeros(N, A, ld, device=dev)
        obs_step = torch.zeros(N, dtype=torch.int32, device=dev)
        mask = torch.zeros(N, A, self.action_dim, dtype=torch.uint8, device=dev) if self.cfg.has_mask else None
        batch.reset(keys, obs, obs_step, mask)
        z = lambda dt: torch.zeros(N, dtype=dt, device=dev)
        ts = self._timestep(st, torch.zeros(N, dtype=torch.int8, device=dev), torch.zeros(N, A, device=dev), torch.ones(N, A, device=dev),
                            obs, obs_step, mask, z(torch.float32), z(torch.int32), z(torch.uint8))
        return st, ts

    def step(self, state: EnvState, action: torch.Tensor) -> Tuple[EnvState, TimeStep]:
        """One env step of the whole batch (``jax.vmap(env.step)(state, action)``): the env state is updated in place; the TimeStep's
        tensors are fresh, so earlier timesteps stay valid."""
        batch = state.batch
        N, A = batch.N, self.num_agents
        dev = action.device
        action = action.to(torch.int32).reshape(N, A).contiguous()
        ld = obs_row_stride(self.cfg.obs_dim)
        obs = torch.zeros(N, A, ld, device=dev) if ld != self.cfg.obs_dim else torch.empty(N, A, ld, device=dev)
        obs_step = torch.empty(N, dtype=torch.int32, device=dev)
        mask = torch.empty(N, A, self.action_dim, dtype=torch.uint8, device=dev) if self.cfg.has_mask else None
        reward, discount = torch.empty(N, A, device=dev), torch.empty(N, A, device=dev)
        done = torch.empty(N, dtype=torch.uint8, device=dev)
        m_ret, m_len, m_term = torch.empty(N, device=dev), torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.uint8, device=dev)
        batch.step(action, reward, done, obs, obs_step, m_ret, m_len, m_term, auto_reset=self.auto_reset, mask=mask, discount=discount)
        step_type = (done + 1).to(torch.int8)   # MID = 1, LAST = 2
        return state, self._timestep(state, step_type, reward, discount, obs, obs_step, mask, m_ret, m_len, m_term)


def _kwargs_and_agent_id(config, *sources, name=None, allowed=(), note=""):
    """The preamble of every factory: the env kwargs, later ``sources`` overriding earlier ones (make_env.py:107-135,211-213), refused unless
    ``allowed`` holds them all (``name`` None: passed on unchecked); and system.add_agent_id as add_extra_wrappers resolves it
    (make_env.py:90-104), written back to the config, where the network set-up reads it."""
    kw = {}
    for src in sources:
        kw.update(src if isinstance(src, dict) else src.to_container())
    unknown = set(kw) - set(allowed)
    if name is not None and unknown:
        raise NotImplementedError(f"{name} kwargs {sorted(unknown)} are not supported{note}")
    add_id = bool(config.system.add_agent_id) and not bool(config.env.implicit_agent_id)
    config.system.add_agent_id = add_id
    return kw, add_id


def _wide_rows_need_agent_id(add_id: bool, name: str):
    if not add_id:
        raise NotImplementedError(f"system.add_agent_id=False with {name}: its 128-float padded observation rows are read with 16-byte "
                                  "vector loads that the column offset behind the one-hot id would misalign (CoordSum and LBF support it)")


def _envs(cfg, add_id: bool):
    """(train_env, eval_env): the eval env has no AutoResetWrapper (make_env.py:90-104)."""
    return MarlEnv(cfg, auto_reset=True, add_agent_id=add_id), MarlEnv(cfg, auto_reset=False, add_agent_id=add_id)


def make_coordsum_env(config):
    task = config.env.scenario.task_name
    if task not in COORDSUM_REGISTRY:
        raise ValueError(f"{task} is not a registered CoordSum scenario")
    # **config.env.kwargs override the registered kwargs (make_env.py:211-213)
    kw, add_id = _kwargs_and_agent_id(config, COORDSUM_REGISTRY[task], config.env.kwargs)
    return _envs(CoordSumConfig(**kw, add_agent_id=add_id), add_id)   # False: the networks read the rows behind the one-hot id (envs.net_obs)


def make_lbf_env(config):
    """make_jumanji_env (make_env.py:107-135) for LevelBasedForaging: generator = RandomGenerator(**scenario.task_config), env
    kwargs = {**env.kwargs, **scenario.env_kwargs}; LbfWrapper's aggregate_rewards keeps its default True whatever
    env.aggregate_rewards says (the factory never passes it)."""
    tc = config.env.scenario.task_config.to_container()
    kw, add_id = _kwargs_and_agent_id(config, config.env.kwargs, config.env.scenario.env_kwargs, name="LevelBasedForaging", allowed={"time_limit"},
                                      note=" (grid observations, penalties, unnormalised rewards)")
    cfg = LbfConfig(grid_size=int(tc["grid_size"]), fov=int(tc["fov"]), num_agents=int(tc["num_agents"]), num_food=int(tc["num_food"]),
                    max_agent_level=int(tc.get("max_agent_level", 2)), force_coop=bool(tc.get("force_coop", False)),
                    time_limit=int(kw.get("time_limit", 100)), add_agent_id=add_id)
    if cfg.obs_dim > 32:
        raise NotImplementedError("LevelBasedForaging: num_agents + 3 (num_food + num_agents) <= 32 (the LBF kernel writes unpadded observation rows)")
    G = cfg.grid_size
    if (G - 2) ** 2 < 5 * (cfg.num_food - 1) + 1 or G * G - cfg.num_food < cfg.num_agents:
        # a food blocks up to 5 interior cells for the later ones; jax.random.choice on an all-zero mask would silently return cell 0
        raise ValueError(f"LevelBasedForaging: a {G}x{G} grid cannot be guaranteed to hold {cfg.num_food} food items and {cfg.num_agents} agents")
    return _envs(cfg, add_id)


def make_rware_env(config):
    """make_jumanji_env (make_env.py:107-135) for RobotWarehouse: generator = RandomGenerator(**scenario.task_config), env kwargs =
    {**env.kwargs (time_limit: 500), **scenario.env_kwargs}, wrapped by RwareWrapper."""
    tc = config.env.scenario.task_config.to_container()
    kw, add_id = _kwargs_and_agent_id(config, config.env.kwargs, config.env.scenario.env_kwargs, name="RobotWarehouse", allowed={"time_limit"})
    _wide_rows_need_agent_id(add_id, "Robot Warehouse")
    cfg = RwareConfig(column_height=int(tc["column_height"]), shelf_rows=int(tc["shelf_rows"]), shelf_columns=int(tc["shelf_columns"]),
                      num_agents=int(tc["num_agents"]), sensor_range=int(tc["sensor_range"]), request_queue_size=int(tc["request_queue_size"]),
                      time_limit=int(kw.get("time_limit", 500)))
    if cfg.sensor_range != 1:
        raise NotImplementedError("RobotWarehouse: sensor_range 1 only (observation rows are padded to 128 floats)")
    return _envs(cfg, add_id)


def make_vector_connector_env(config):
    """make_jumanji_env (make_env.py:107-135) for VectorConnector (_jumanji_registry, make_env.py:64-75): generator =
    RandomWalkGenerator(**scenario.task_config), env kwargs = {**env.kwargs, **scenario.env_kwargs} (time_limit only), wrapped by
    VectorConnectorWrapper with its default aggregate_rewards (the factory never passes env.aggregate_rewards, as for LBF)."""
    tc = config.env.scenario.task_config.to_container()
    kw, add_id = _kwargs_and_agent_id(config, config.env.kwargs, config.env.scenario.env_kwargs, name="VectorConnector", allowed={"time_limit"})
    _wide_rows_need_agent_id(add_id, "VectorConnector")
    cfg = VectorConnectorConfig(grid_size=int(tc["grid_size"]), num_agents=int(tc["num_agents"]), time_limit=int(kw.get("time_limit", 100)))
    G, A = cfg.grid_size, cfg.num_agents
    if not (2 <= G <= 16 and 1 <= A <= 32 and A <= G * G):
        raise NotImplementedError("VectorConnector: 2 <= grid_size <= 16 and 1 <= num_agents <= min(32, grid_size^2) (csrc/connector.hip)")
    return _envs(cfg, add_id)


def make_mpe_env(config):
    """make_jaxmarl_env (make_env.py:138-170) for MPE: kwargs = {**env.kwargs, **scenario.task_config} for
    jaxmarl.make(scenario.name, **kwargs), wrapped by MPEWrapper (time_limit = the env's max_steps).  Discrete actions only."""
    kw, add_id = _kwargs_and_agent_id(config, config.env.kwargs, config.env.scenario.task_config, name="MPE",
                                      allowed={"action_type", "num_agents", "num_landmarks", "local_ratio", "max_steps"})
    action_type = kw.get("action_type", "Discrete")
    if action_type == "Continuous":
        raise NotImplementedError("MPE with continuous actions (tanh-Gaussian heads) is not supported: override env.kwargs.action_type=Discrete")
    if action_type != "Discrete":
        raise ValueError(f"MPE action_type {action_type!r}: 'Discrete' or 'Continuous'")
    cfg = MpeConfig(num_agents=int(kw.get("num_agents", 3)), num_landmarks=int(kw.get("num_landmarks", 3)),
                    local_ratio=float(kw.get("local_ratio", 0.5)), time_limit=int(kw.get("max_steps", 25)), add_agent_id=add_id)
    A, L = cfg.num_agents, cfg.num_landmarks
    if not (1 <= A <= 32 and 1 <= L <= 32 and cfg.time_limit >= 1):
        raise ValueError("MPE: 1 <= num_agents <= 32, 1 <= num_landmarks <= 32 and max_steps >= 1 (csrc/mpe.hip)")
    if cfg.obs_dim > 128:
        raise NotImplementedError(f"MPE: observations of {cfg.obs_dim} floats (5 num_agents + 2 num_landmarks <= 128 required)")
    net_obs(cfg)   # system.add_agent_id=False needs narrow rows (3 agents: 18 features)
    return _envs(cfg, add_id)


FACTORIES = {"CoordSum": make_coordsum_env, "LevelBasedForaging": make_lbf_env, "RobotWarehouse": make_rware_env,
             "VectorConnector": make_vector_connector_env, "MPE": make_mpe_env}


def make(config, add_global_state: bool = False):
    """``add_global_state`` (make_env.py:202-218,288-315; rec_mappo.py:558): the centralised critic's observation.global_state -- the
    concatenation over agents of the raw agent views, taken before the AgentIDWrapper and tiled to every agent.  On the HIP path the
    learner forms those rows from the stored observation rows (magpo_global_state) whenever it needs them, so the flag only checks that
    the env supports it (num_agents * raw features <= 128) and marks the envs (``env.add_global_state``, ``env.global_state_dim``)."""
    env_name = config.env.env_name
    if env_name not in FACTORIES:
        raise ValueError(f"{env_name} is not a supported environment.")
    env, eval_env = FACTORIES[env_name](config)
    if add_global_state:
        from ..critic import global_state_ld
        raw = env.cfg.obs_dim - env.cfg.num_agents
        global_state_ld(env.cfg.num_agents, raw)   # NotImplementedError that names the limit (Robot Warehouse and anything wider)
        for e in (env, eval_env):
            e.add_global_state, e.global_state_dim = True, env.cfg.num_agents * raw
    return env, eval_env
