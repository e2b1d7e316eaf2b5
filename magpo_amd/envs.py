"""The environments: their configs and the device-resident batches that drive the HIP env kernels.

Every environment runs under the same Mava wrapper stack (env wrapper -> AgentIDWrapper -> AutoResetWrapper -> RecordEpisodeMetrics,
mava/utils/make_env.py:90-104), which the kernels implement once in csrc/env_wrappers.hpp; on the host it is ``EnvBatch``.  An
environment is its dynamics and observation function (csrc/<env>.hip), a config dataclass and an ``EnvBatch`` subclass that names its
state tensors, its scalar arguments and its entry points, plus one entry of ``ENV_BATCHES``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ._lib import lib


@dataclass
class CoordSumConfig:
    num_agents: int
    num_actions: int
    time_limit: int = 100
    maxval: Optional[int] = None
    add_agent_id: bool = True  # system.add_agent_id (AgentIDWrapper, make_env.py:90-104): False = the networks read the rows behind the one-hot id
    has_mask = False          # action_mask is all-True (matrax.py:117-134): never stored
    class_tables = True       # observations take few distinct values: first-layer class tables apply (csrc/classtab.hip)

    def __post_init__(self):
        if not self.maxval:
            self.maxval = self.num_actions  # coordsum/env.py:49-53

    @property
    def obs_dim(self) -> int:   # AgentIDWrapper (observation.py:42-54): [one-hot id | target]
        return self.num_agents + 1


@dataclass
class LbfConfig:
    """jumanji LevelBasedForaging-v0 + RandomGenerator(**task_config) (configs/env/scenario/*-coop.yaml) under LbfWrapper."""
    grid_size: int = 8
    fov: int = 8
    num_agents: int = 2
    num_food: int = 2
    max_agent_level: int = 2
    force_coop: bool = True
    time_limit: int = 100
    add_agent_id: bool = True
    has_mask = True
    class_tables = False
    num_actions = 6

    @property
    def obs_dim(self) -> int:   # vector observation 3 (num_food + num_agents) + one-hot agent id
        return 3 * (self.num_food + self.num_agents) + self.num_agents


@dataclass
class RwareConfig:
    """jumanji RobotWarehouse-v0 + RandomGenerator(**task_config) (configs/env/scenario/tiny-4ag.yaml ...) under RwareWrapper."""
    column_height: int = 8
    shelf_rows: int = 1
    shelf_columns: int = 3
    num_agents: int = 4
    sensor_range: int = 1
    request_queue_size: int = 4
    time_limit: int = 500
    has_mask = True
    class_tables = False
    num_actions = 5

    @property
    def obs_dim(self) -> int:   # 8 + 7 (2 r + 1)^2 vector observation + one-hot agent id
        return 8 + 7 * (2 * self.sensor_range + 1) ** 2 + self.num_agents


@dataclass
class VectorConnectorConfig:
    """jumanji Connector-v2 + RandomWalkGenerator(**task_config) (configs/env/scenario/con-*.yaml) under VectorConnectorWrapper."""
    grid_size: int = 10
    num_agents: int = 10
    time_limit: int = 100
    has_mask = True
    class_tables = False
    num_actions = 5

    @property
    def obs_dim(self) -> int:   # 4 coordinates + two 5 x 5 windows + one-hot agent id
        return 54 + self.num_agents


@dataclass
class MpeConfig:
    """JaxMARL MPE_simple_spread_v3(**task_config) (configs/env/scenario/simple_spread_*.yaml), discrete actions, under MPEWrapper."""
    num_agents: int = 3
    num_landmarks: int = 3
    local_ratio: float = 0.5
    time_limit: int = 25        # SimpleMPE max_steps; an episode lasts time_limit + 1 steps (csrc/mpe.hip)
    add_agent_id: bool = True   # system.add_agent_id: False = the networks read the rows behind the one-hot id (narrow rows only, net_obs)
    has_mask = False            # every action is legal (MPEWrapper.action_mask): never stored
    class_tables = False
    num_actions = 5

    @property
    def obs_dim(self) -> int:   # vel, pos, landmarks, other agents' positions and (silent) comm + one-hot agent id
        return 4 + 2 * self.num_landmarks + 4 * (self.num_agents - 1) + self.num_agents


def net_obs(cfg) -> Tuple[int, int]:
    """(features the networks read, column offset of the first one inside an observation row).  The env kernels always write
    [one-hot agent id | features] rows (AgentIDWrapper, observation.py:42-54); with ``system.add_agent_id: False`` (make_env.py:90-104: the
    wrapper is not applied) the networks are built for the features alone and every consumer gets the row pointer advanced by num_agents
    floats with the row stride unchanged.  Narrow observations only (the 128-float padded rows of wide observations are read with
    16-byte vector loads that a column offset would misalign)."""
    if getattr(cfg, "add_agent_id", True):
        return cfg.obs_dim, 0
    if cfg.obs_dim > 32:
        raise NotImplementedError("system.add_agent_id=False with wide observations (obs_dim > 32: Robot Warehouse)")
    return cfg.obs_dim - cfg.num_agents, cfg.num_agents


def obs_row_stride(obs_dim: int) -> int:
    """Floats between observation rows: obs_dim for small observations, 128 (zero-padded) for wide ones (csrc/wideobs.hip)."""
    return obs_dim if obs_dim <= 32 else 128


def host_split(key: np.ndarray, num: int = 2) -> np.ndarray:
    """jax.random.split of one key on the host (exact; C ABI magpo_key_split_host)."""
    key = np.ascontiguousarray(key, dtype=np.uint32)
    out = np.empty((num, 2), np.uint32)
    lib().raw("magpo_key_split_host")(key.ctypes.data, num, out.ctypes.data)
    return out


def agent_sample_keys(key: np.ndarray, A: int) -> Tuple[np.ndarray, np.ndarray]:
    """The key chain inside get_actions (decode.py:141): key, sample_key = split(key), once per agent in agent order.
    Returns (the carried key, the A sample keys [A, 2])."""
    k = np.asarray(key, dtype=np.uint32).reshape(2)
    keys = np.zeros((A, 2), np.uint32)
    for i in range(A):
        kk = host_split(k, 2)
        k, keys[i] = kk[0], kk[1]
    return k, keys


def prng_key(seed: int) -> np.ndarray:
    return np.array([(int(seed) >> 32) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFF], np.uint32)


I32, U8, F32 = torch.int32, torch.uint8, torch.float32
TensorSpecs = Dict[str, Tuple[torch.dtype, Tuple[int, ...]]]   # name -> (dtype, shape behind the env axis)


class EnvBatch:
    """Device-resident batch of wrapped envs: the env's own state tensors plus what the wrappers keep for every env -- the env key, the
    RecordEpisodeMetrics key and counters (episode_metrics.py:35-48).  ``reset`` / ``step`` are one kernel launch over the whole batch
    (include/magpo.h: <prefix>_reset / <prefix>_step, whose flat argument lists they assemble).  A subclass declares:

      prefix        entry-point prefix
      state_fields  every state tensor in ABI order (what ``make_env.EnvState`` exposes as the reference's State pytree)
      tensors()     (dtype, per-env shape) of the tensors the base class does not own
      scalars()     the config arguments behind N
      takes_ldo / takes_mask   whether the entry points take the observation row stride / write an action mask"""
    prefix = ""
    state_fields: Tuple[str, ...] = ()
    takes_ldo = takes_mask = False
    has_real_obs = False   # the env has a <prefix>_step_real_obs entry point
    WRAPPER_TENSORS: TensorSpecs = dict(key=(I32, (2,)), metrics_key=(I32, (2,)), run_ret=(F32, ()), run_len=(I32, ()), ep_ret=(F32, ()),
                                        ep_len=(I32, ()))

    def __init__(self, cfg, N: int, device):
        self.cfg, self.N, self.dev, self.L = cfg, N, device, lib()
        self.ldo = obs_row_stride(cfg.obs_dim)
        for name, (dtype, shape) in {**self.tensors(), **self.WRAPPER_TENSORS}.items():
            setattr(self, name, torch.zeros(N, *shape, dtype=dtype, device=device))

    def tensors(self) -> TensorSpecs:
        raise NotImplementedError

    def scalars(self) -> tuple:
        raise NotImplementedError

    def _args(self):
        return (*(getattr(self, f) for f in self.state_fields), self.N, *self.scalars())

    def _obs_args(self, obs, obs_step, mask):
        return (obs, *((self.ldo,) if self.takes_ldo else ()), obs_step, *((mask,) if self.takes_mask else ()))

    def reset(self, env_keys: torch.Tensor, obs, obs_step, mask=None):
        self.L.call(self.prefix + "_reset", *self._args(), env_keys, *self._obs_args(obs, obs_step, mask),
                    torch.cuda.current_stream().cuda_stream)

    def step(self, actions, reward, done, obs, obs_step, m_ret, m_len, m_term, auto_reset=True, mask=None, discount=None, real_obs=None,
             real_mask=None):
        """``real_obs`` / ``real_mask``: extras["real_next_obs"] (auto_reset_wrapper.py:52-83), the stepped state's observation and mask before
        any auto-reset, through the env's ``_step_real_obs`` entry point (CoordSum and LBF have one)."""
        name, real = self.prefix + "_step", ()
        if real_obs is not None or real_mask is not None:
            if not self.has_real_obs:
                raise NotImplementedError(f"{type(self.cfg).__name__}: the env kernel does not write real_next_obs (CoordSum and LBF do)")
            name, real = name + "_real_obs", (real_obs, *((real_mask,) if self.takes_mask else ()))
        self.L.call(name, *self._args(), actions, self.cfg.num_agents, reward, discount, done,
                    *self._obs_args(obs, obs_step, mask), m_ret, m_len, m_term, 1 if auto_reset else 0, *real, torch.cuda.current_stream().cuda_stream)


class CoordSumEnvBatch(EnvBatch):
    """Wrapped CoordSum envs (csrc/coordsum.hip; state surface of coordsum/env.py:17-26)."""
    prefix, has_real_obs = "magpo_coordsum", True
    state_fields = ("step_count", "target", "record", "key", "metrics_key", "run_ret", "run_len", "ep_ret", "ep_len")

    def tensors(self):
        c = self.cfg
        return dict(step_count=(I32, ()), target=(I32, (c.time_limit + 1,)), record=(I32, (c.num_actions, c.time_limit)))

    def scalars(self):
        c = self.cfg
        return (c.num_agents, c.num_actions, c.time_limit, c.maxval)


class LbfEnvBatch(EnvBatch):
    """Wrapped Level-Based Foraging envs (csrc/lbf.hip; UNPINNED dynamics, see oracle/lbf.py)."""
    prefix, takes_mask, has_real_obs = "magpo_lbf", True, True
    state_fields = ("agent_pos", "agent_level", "food_pos", "food_level", "food_eaten", "step_count", "key", "metrics_key",
                    "run_ret", "run_len", "ep_ret", "ep_len")

    def tensors(self):
        A, NF = self.cfg.num_agents, self.cfg.num_food
        return dict(agent_pos=(I32, (A, 2)), agent_level=(I32, (A,)), food_pos=(I32, (NF, 2)), food_level=(I32, (NF,)),
                    food_eaten=(U8, (NF,)), step_count=(I32, ()))

    def scalars(self):
        c = self.cfg
        return (c.num_agents, c.num_food, c.grid_size, c.fov, c.max_agent_level, 1 if c.force_coop else 0, c.time_limit)


class RwareEnvBatch(EnvBatch):
    """Wrapped Robot Warehouse envs (csrc/rware.hip; UNPINNED dynamics, see oracle/rware.py)."""
    prefix, takes_ldo, takes_mask = "magpo_rware", True, True
    state_fields = ("grid_a", "grid_s", "agent_pos", "agent_dir", "agent_carry", "shelf_req", "queue", "step_count", "amask", "key",
                    "metrics_key", "run_ret", "run_len", "ep_ret", "ep_len")

    def __init__(self, cfg: RwareConfig, N: int, device):
        lay = np.zeros(3, np.int32)
        lib().call("magpo_rware_layout", cfg.column_height, cfg.shelf_rows, cfg.shelf_columns, lay.ctypes.data)
        self.H, self.W, self.NS = int(lay[0]), int(lay[1]), int(lay[2])
        super().__init__(cfg, N, device)

    def tensors(self):
        A, H, W = self.cfg.num_agents, self.H, self.W
        return dict(grid_a=(I32, (H, W)), grid_s=(I32, (H, W)), agent_pos=(I32, (A, 2)), agent_dir=(I32, (A,)), agent_carry=(U8, (A,)),
                    shelf_req=(U8, (self.NS,)), queue=(I32, (self.cfg.request_queue_size,)), step_count=(I32, ()), amask=(U8, (A, 5)))

    def scalars(self):
        c = self.cfg
        return (c.num_agents, c.column_height, c.shelf_rows, c.shelf_columns, c.sensor_range, c.request_queue_size, c.time_limit)


class ConnectorEnvBatch(EnvBatch):
    """Wrapped VectorConnector envs (csrc/connector.hip; UNPINNED dynamics, see its header comment)."""
    prefix, takes_ldo, takes_mask = "magpo_connector", True, True
    state_fields = ("grid", "agent_start", "agent_target", "agent_pos", "step_count", "key", "metrics_key", "run_ret", "run_len", "ep_ret",
                    "ep_len")

    def tensors(self):
        A, G = self.cfg.num_agents, self.cfg.grid_size
        return dict(grid=(I32, (G, G)), agent_start=(I32, (A, 2)), agent_target=(I32, (A, 2)), agent_pos=(I32, (A, 2)), step_count=(I32, ()))

    def scalars(self):
        c = self.cfg
        return (c.num_agents, c.grid_size, c.time_limit)


class MpeEnvBatch(EnvBatch):
    """Wrapped MPE simple_spread envs (csrc/mpe.hip; UNPINNED dynamics, see tests/mpe_ref.py)."""
    prefix, takes_ldo = "magpo_mpe", True
    state_fields = ("pos", "vel", "inner_step", "step_count", "key", "metrics_key", "run_ret", "run_len", "ep_ret", "ep_len")

    def tensors(self):
        A, L = self.cfg.num_agents, self.cfg.num_landmarks
        return dict(pos=(F32, (A + L, 2)), vel=(F32, (A, 2)), inner_step=(I32, ()), step_count=(I32, ()))

    def scalars(self):
        c = self.cfg
        return (c.num_agents, c.num_landmarks, c.time_limit, float(c.local_ratio))


ENV_BATCHES = {CoordSumConfig: CoordSumEnvBatch, LbfConfig: LbfEnvBatch, RwareConfig: RwareEnvBatch, VectorConnectorConfig: ConnectorEnvBatch,
               MpeConfig: MpeEnvBatch}


def make_env_batch(cfg, N: int, device) -> EnvBatch:
    return ENV_BATCHES[type(cfg)](cfg, N, device)
