"""VectorConnector + Mava wrapper stack, batched numpy restatement (test infrastructure only; the product never imports it).

Same contract as oracle/rware.py -- ``reset(spec, keys)`` / ``step(spec, state, actions, auto_reset)`` and the same timestep dict -- so
that it plugs into oracle.learner.OracleLearner(..., env=...) and oracle.evaluator.evaluate(..., env=...) unchanged.

Wrapper order (mava/utils/make_env.py:64-75,90-104,107-135):
  RecordEpisodeMetrics (wrappers/episode_metrics.py:60-112)
    -> AutoResetWrapper (wrappers/auto_reset_wrapper.py:60-101)      [train env only]
      -> AgentIDWrapper (wrappers/observation.py:42-54: eye(A) in front of every row)
        -> VectorConnectorWrapper (wrappers/jumanji.py:368-455; aggregate_rewards always on: the factory never passes the flag)
          -> jumanji Connector-v2 with RandomWalkGenerator(grid_size, num_agents), time_limit from the scenario

PINNED by the reference tree (wrappers/jumanji.py:223-241,346-365,368-455):
  * grid values: agent i has path 3i+1, position 3i+2, target 3i+3, empty 0.  switch_perspective shifts agent values by multiples of 3,
    so "position" = v % 3 == 2, "path" = v % 3 == 1, "target" = v % 3 == 0 and v != 0 for every perspective; in agent i's perspective
    its own position reads 2 and its own target 3.
  * features per agent, in order: my_pos (row, col) / G^2 and my_target (row, col) / G^2 (``grid[0].size`` is a whole G x G grid),
    both fp32 true divisions; then the 5 x 5 ``blockers`` window around my_pos (any position 1, any path -1, else 0) and the 5 x 5
    ``targets`` window (own target 1, other targets -1, else 0), both row-major.  Cells outside the grid read 1 in both windows
    (jnp.pad(..., constant_values=True)).
  * _get_location = argmax of a boolean grid: a missing value (a connected agent's target cell holds its position) reads (0, 0).
  * reward: the per-agent rewards summed in agent order in fp32 and repeated for every agent.

UNPINNED DYNAMICS.  Jumanji's Connector environment and RandomWalkGenerator are third-party and absent from the reference tree; they
are restated here from memory of the published algorithm (csrc/connector.hip restates the same rules and agrees bit for bit):
  * actions NOOP, UP, RIGHT, DOWN, LEFT = moves (0, 0), (-1, 0), (0, 1), (1, 0), (0, -1); an action outside 0..4 acts as NOOP.
  * a move is valid if the new cell is on the grid and is EMPTY or the agent's own target, and the agent is not connected
    (connected = position == target).  An invalid move (or NOOP) leaves the agent where it is; a connected agent never moves.
  * all agents step at once, each on the old grid: a mover leaves its path value on the cell it left and puts its position value on
    the new one.  The agents' grids, each keeping that agent's values only, are merged by max, so when several agents enter one cell
    the highest id wins.  Every agent whose position value is gone from the merged grid collided: its old cell (which holds its path
    value) gets its position value back, and its position reverts.
  * action mask, computed on the state after the step: NOOP always legal; a direction is legal iff that move is valid.
  * per-agent reward (DenseRewardFn): 0.1 for an agent that becomes connected this step plus -0.03 for each agent that was not
    connected before it (fp32: 0.1 * newly + (-0.03) * not_connected_before).
  * the episode ends (termination, discount 0) when every agent is connected or blocked (no legal direction), or when
    step_count >= time_limit.  The reset timestep has step_count 0, reward 0 and discount 1.
  * generator: key, board_key = split(key) (the state keeps key); key, step_key = split(board_key); starts = choice(key, G*G, (A,),
    replace=False) with each agent's position value on its start cell.  While some agent has an EMPTY neighbour: cur, step_key =
    split(step_key); keys = split(cur, A); agent i draws one of its neighbours [up, right, down, left] (off-grid cells are -1) with
    choice(keys[i], 4, (), p=neighbour is EMPTY) (replace=True) and moves there under the env's simultaneous-move and merge rules.  An
    agent without an EMPTY neighbour draws index 0 (an all-zero p) whose cell is -1 and stays put.  Each agent's final cell becomes its
    target; the board is then rebuilt empty with every position value written on its start cell and then every target value on its
    final cell.
  * CHOICE (documented here, not recalled): an agent that never moved has its target on its start cell.  The target value, written
    last, then owns the cell and the agent starts connected (position == target): it only has NOOP, earns 0 and counts as connected
    for the ending; its position value is on no cell, so its my_pos reads (0, 0).
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np

from oracle import prng

STEP_FIRST, STEP_MID, STEP_LAST = 0, 1, 2
NOOP, UP, RIGHT, DOWN, LEFT = 0, 1, 2, 3, 4
NUM_ACTIONS = 5
MOVES = np.array([[0, 0], [-1, 0], [0, 1], [1, 0], [0, -1]], np.int32)
FOV = 2
NUM_FEATURES = 4 + 2 * (2 * FOV + 1) ** 2   # 54
CONNECTED_REWARD, TIMESTEP_REWARD = np.float32(0.1), np.float32(-0.03)


def path_value(i):
    return 3 * i + 1


def position_value(i):
    return 3 * i + 2


def target_value(i):
    return 3 * i + 3


class ConnectorSpec:
    def __init__(self, grid_size=10, num_agents=10, time_limit=100):
        self.grid_size, self.num_agents, self.time_limit = int(grid_size), int(num_agents), int(time_limit)
        self.num_actions = NUM_ACTIONS

    @property
    def obs_dim(self) -> int:   # 54 vector features + one-hot agent id (AgentIDWrapper)
        return NUM_FEATURES + self.num_agents


def _valid_moves(spec: ConnectorSpec, grid, pos, target) -> np.ndarray:
    """is_valid_position of every agent's four moves [A][UP, RIGHT, DOWN, LEFT] on ``grid``: on the grid, EMPTY or the agent's own
    target, and the agent not connected."""
    G, A = spec.grid_size, spec.num_agents
    nxt = pos[:, None, :] + MOVES[None, 1:, :]
    inb = (nxt >= 0).all(-1) & (nxt < G).all(-1)
    v = grid[np.clip(nxt[..., 0], 0, G - 1), np.clip(nxt[..., 1], 0, G - 1)]
    connected = (pos == target).all(-1)
    return inb & ((v == 0) | (v == target_value(np.arange(A))[:, None])) & ~connected[:, None]


def _move_all(spec: ConnectorSpec, grid, pos, target, actions):
    """Connector._step_agents: every agent steps on the old grid, the per-agent grids are merged by max, collisions are undone."""
    A = spec.num_agents
    ids = np.arange(A)
    a = np.where((actions >= 0) & (actions < NUM_ACTIONS), actions, NOOP)
    valid = np.concatenate([np.zeros((A, 1), bool), _valid_moves(spec, grid, pos, target)], axis=1)
    moves = valid[ids, a]
    nxt = pos + MOVES[a]
    grids = np.broadcast_to(grid, (A,) + grid.shape).copy()   # every agent's grid after its own move
    for i in np.nonzero(moves)[0]:
        grids[i, pos[i][0], pos[i][1]] = path_value(i)
        grids[i, nxt[i][0], nxt[i][1]] = position_value(i)
    vi = ids[:, None, None]
    own = (grids == path_value(vi)) | (grids == position_value(vi)) | (grids == target_value(vi))   # get_agent_grid
    joined = np.max(np.where(own, grids, 0), axis=0)
    new_pos = np.where(moves[:, None], nxt, pos).astype(np.int32)
    correction = np.zeros_like(joined)
    for i in range(A):
        if not (joined == position_value(i)).any():   # collided: the old cell gets its position value back
            correction += (grid == position_value(i)) * (position_value(i) - path_value(i))
            new_pos[i] = pos[i]
    return joined + correction, new_pos


def _action_mask(spec: ConnectorSpec, st) -> np.ndarray:
    """NOOP always legal; a direction iff its move is valid."""
    valid = _valid_moves(spec, st["grid"], st["agent_pos"], st["agent_target"])
    return np.concatenate([np.ones((spec.num_agents, 1), bool), valid], axis=1)


def _neighbours(G, pos):
    """RandomWalkGenerator._adjacent_cells for every agent: [A][up, right, down, left] flat indices, -1 off the grid."""
    r, c = pos[:, 0:1], pos[:, 1:2]
    rr, cc = r + MOVES[1:, 0][None], c + MOVES[1:, 1][None]
    return np.where((rr >= 0) & (rr < G) & (cc >= 0) & (cc < G), rr * G + cc, -1)


def random_walk(spec: ConnectorSpec, board_key: np.ndarray):
    """RandomWalkGenerator.generate_board's walk: (start cells [A], final cells [A], the walked board [G*G] with every agent's path and
    its head on its final cell)."""
    G, A = spec.grid_size, spec.num_agents
    key_start, step_key = prng.split(board_key, 2)
    starts = prng.choice(key_start, G * G, A, False)
    flat = np.zeros(G * G, np.int32)
    flat[starts] = position_value(np.arange(A))
    cell = starts.astype(np.int64)
    ids = np.arange(A)
    while True:
        nb = _neighbours(G, np.stack(np.divmod(cell, G), axis=1))
        free = (nb >= 0) & (flat[np.maximum(nb, 0)] == 0)
        if not free.any():
            break
        cur, step_key = prng.split(step_key, 2)
        keys = prng.split(cur, A)
        # choice(keys[i], 4, (), p=free[i]) with replace=True: the first neighbour whose cumulative count reaches total * (1 - u)
        cum = np.cumsum(free.astype(np.float32), axis=1, dtype=np.float32)
        r = (cum[:, -1] * (np.float32(1.0) - prng.uniform(keys, 1)[:, 0])).astype(np.float32)
        d = np.argmax(cum >= r[:, None], axis=1)
        pick = np.where(free[ids, d], nb[ids, d], -1)   # available_cells: taken and off-grid neighbours are -1
        # simultaneous moves onto EMPTY cells: of several agents entering one cell the highest id wins (the env's max merge), the others
        # stay (collision correction); a -1 draw never moves
        win = pick >= 0
        for i in range(A):
            if win[i] and (pick[i + 1:] == pick[i]).any():
                win[i] = False
        for i in np.nonzero(win)[0]:
            flat[cell[i]] = path_value(i)
            flat[pick[i]] = position_value(i)
            cell[i] = pick[i]
    return starts, cell, flat


def _generate(spec: ConnectorSpec, key: np.ndarray) -> Dict[str, np.ndarray]:
    G, A = spec.grid_size, spec.num_agents
    key_state, board_key = prng.split(key, 2)
    starts, cell, _ = random_walk(spec, board_key)
    start = np.stack(np.divmod(starts, G), axis=1).astype(np.int32)
    target = np.stack(np.divmod(cell, G), axis=1).astype(np.int32)
    board = np.zeros((G, G), np.int32)
    for i in range(A):
        board[start[i][0], start[i][1]] = position_value(i)
    for i in range(A):
        board[target[i][0], target[i][1]] = target_value(i)
    return dict(grid=board, agent_start=start, agent_target=target, agent_pos=start.copy(), step_count=np.int32(0), key=key_state.copy())


def _location(mask: np.ndarray) -> Tuple[int, int]:
    """_get_location: argmax of a boolean grid (0 when the value is absent)."""
    idx = int(np.argmax(mask))
    return idx // mask.shape[-1], idx % mask.shape[-1]


def _observe(spec: ConnectorSpec, grid: np.ndarray) -> np.ndarray:
    """VectorConnectorWrapper.modify_timestep's agents_view for one env: [A][54] fp32 (create_agents_view vectorised over the agents)."""
    G, A = spec.grid_size, spec.num_agents
    ids = np.arange(A)[:, None, None]
    view = np.where(grid >= 1, (grid[None] - 1 - 3 * ids) % (3 * A) + 1, grid[None])   # switch_perspective, [A][G][G]
    blockers = np.where(view % 3 == 2, 1, np.where(view % 3 == 1, -1, 0))
    targets = np.where(view == 3, 1, np.where((view % 3 == 0) & (view != 0), -1, 0))
    loc = lambda m: np.divmod(np.argmax(m.reshape(A, G * G), axis=1), G)   # _get_location: argmax of a boolean grid
    (pr, pc), (tr, tc) = loc(view == 2), loc(view == 3)
    pad = ((0, 0), (FOV, FOV), (FOV, FOV))
    pb, pt = np.pad(blockers, pad, constant_values=1), np.pad(targets, pad, constant_values=1)
    w = np.arange(2 * FOV + 1)
    rows, cols = (pr[:, None] + w)[:, :, None], (pc[:, None] + w)[:, None, :]   # dynamic_slice at the padded-grid position
    size = np.float32(G * G)
    out = np.zeros((A, NUM_FEATURES), np.float32)
    out[:, 0], out[:, 1] = pr.astype(np.float32) / size, pc.astype(np.float32) / size
    out[:, 2], out[:, 3] = tr.astype(np.float32) / size, tc.astype(np.float32) / size
    out[:, 4:29] = pb[np.arange(A)[:, None, None], rows, cols].reshape(A, -1)
    out[:, 29:54] = pt[np.arange(A)[:, None, None], rows, cols].reshape(A, -1)
    return out


def _step_one(spec: ConnectorSpec, st, actions):
    """Connector.step for one env; returns (new state, per-agent rewards, done)."""
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    A = spec.num_agents
    was = np.all(st["agent_pos"] == st["agent_target"], axis=1)
    st["grid"], st["agent_pos"] = _move_all(spec, st["grid"], st["agent_pos"], st["agent_target"], actions)
    now = np.all(st["agent_pos"] == st["agent_target"], axis=1)
    reward = (CONNECTED_REWARD * (~was & now).astype(np.float32) + TIMESTEP_REWARD * (~was).astype(np.float32)).astype(np.float32)
    st["step_count"] = np.int32(st["step_count"] + 1)
    mask = _action_mask(spec, st)
    finished = all(now[i] or not mask[i, 1:].any() for i in range(A))
    return st, reward, bool(finished or st["step_count"] >= spec.time_limit)


_CORE = ("grid", "agent_start", "agent_target", "agent_pos", "step_count", "key")


def _stack(sts):
    return {f: np.stack([s[f] for s in sts]) for f in _CORE}


def _unstack(st, n):
    return {f: st[f][n] for f in _CORE}


def make_obs(spec: ConnectorSpec, st: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """VectorConnectorWrapper.modify_timestep + AgentIDWrapper (one-hot id in front)."""
    N, A = st["grid"].shape[0], spec.num_agents
    view = np.stack([_observe(spec, st["grid"][n]) for n in range(N)])
    ids = np.broadcast_to(np.eye(A, dtype=np.float32)[None], (N, A, A))
    mask = np.stack([_action_mask(spec, _unstack(st, n)) for n in range(N)])
    return dict(agents_view=np.concatenate([ids, view], axis=-1), action_mask=mask,
                step_count=np.repeat(st["step_count"][:, None], A, axis=1).astype(np.int32))


def reset(spec: ConnectorSpec, env_keys: np.ndarray) -> Tuple[Dict, Dict]:
    ks = prng.split(env_keys, 2)   # key (kept, unused), reset_key  (episode_metrics.py:62)
    core = _stack([_generate(spec, k) for k in ks[:, 1, :]])
    n, a = env_keys.shape[0], spec.num_agents
    state = dict(core, metrics_key=ks[:, 0, :].copy(), running_return=np.zeros(n, np.float32), running_length=np.zeros(n, np.int32),
                 episode_return=np.zeros(n, np.float32), episode_length=np.zeros(n, np.int32))
    timestep = dict(step_type=np.full(n, STEP_FIRST, np.int8), reward=np.zeros((n, a), np.float32), discount=np.ones((n, a), np.float32),
                    observation=make_obs(spec, core),
                    episode_metrics=dict(episode_return=np.zeros(n, np.float32), episode_length=np.zeros(n, np.int32),
                                         is_terminal_step=np.zeros(n, bool)))
    return state, timestep


def step(spec: ConnectorSpec, state: Dict, actions: np.ndarray, auto_reset: bool = True) -> Tuple[Dict, Dict]:
    actions = np.asarray(actions, np.int32)
    N, a = actions.shape[0], spec.num_agents
    res = [_step_one(spec, _unstack(state, n), actions[n]) for n in range(N)]
    core = _stack([r[0] for r in res])
    team = np.zeros(N, np.float32)
    for i in range(a):   # aggregate_rewards: the per-agent rewards summed in agent order
        team = (team + np.array([r[1][i] for r in res], np.float32)).astype(np.float32)
    done = np.array([r[2] for r in res], bool)
    if auto_reset and done.any():   # auto_reset_wrapper.py:60-83: key, _ = split(state.key); reset(key); reward etc. kept
        idx = np.nonzero(done)[0]
        fresh = _stack([_generate(spec, k) for k in prng.split(core["key"][idx], 2)[:, 0, :]])
        for k in _CORE:
            core[k][idx] = fresh[k]
    rewards = np.repeat(team[:, None], a, axis=1)
    discount = np.repeat(np.where(done, 0.0, 1.0).astype(np.float32)[:, None], a, axis=1)
    not_done = (~done).astype(np.float32)
    msum = np.zeros(N, np.float32)
    for i in range(a):
        msum = (msum + rewards[:, i]).astype(np.float32)
    new_ret = (state["running_return"] + msum / np.float32(a)).astype(np.float32)   # episode_metrics.py:91-96
    new_len = state["running_length"] + 1
    ep_ret = (state["episode_return"] * not_done + new_ret * done).astype(np.float32)
    ep_len = np.where(done, new_len, state["episode_length"]).astype(np.int32)
    new_state = dict(core, metrics_key=state["metrics_key"], running_return=(new_ret * not_done).astype(np.float32),
                     running_length=np.where(done, 0, new_len).astype(np.int32), episode_return=ep_ret, episode_length=ep_len)
    timestep = dict(step_type=np.where(done, STEP_LAST, STEP_MID).astype(np.int8), reward=rewards, discount=discount,
                    observation=make_obs(spec, core),
                    episode_metrics=dict(episode_return=ep_ret, episode_length=ep_len, is_terminal_step=done.copy()))
    return new_state, timestep
