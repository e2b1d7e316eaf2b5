"""VectorConnector without a GPU: the env factory (configs/env/vector-connector.yaml + scenario/con-*.yaml) and the numpy restatement
tests/connector_ref.py on hand-built boards (the rules the GPU kernel csrc/connector.hip is checked against bit for bit)."""
import numpy as np
import pytest

from oracle import prng
from tests import connector_ref as C


@pytest.mark.parametrize("scenario,A,F,TL", [("con-5x5x3a", 3, 57, 25), ("con-7x7x5a", 5, 59, 49), ("con-10x10x10a", 10, 64, 100),
                                             ("con-15x15x23a", 23, 77, 225)])
def test_vector_connector_factory(scenario, A, F, TL):
    from magpo_amd.config import compose
    from magpo_amd.learner import VectorConnectorConfig
    from magpo_amd.utils import make_env as environments
    cfg = compose("rec_magpo", ["env=vector-connector", f"env/scenario={scenario}"])
    env, eval_env = environments.make(cfg)
    assert (env.num_agents, env.action_dim, env.obs_dim, env.time_limit) == (A, 5, F, TL)
    assert (eval_env.num_agents, eval_env.action_dim, eval_env.obs_dim, eval_env.time_limit) == (A, 5, F, TL)
    assert env.auto_reset and not eval_env.auto_reset
    assert isinstance(env.unwrapped, VectorConnectorConfig) and env.unwrapped.has_mask and not env.unwrapped.class_tables
    assert env.observation_spec.agents_view.shape == (A, F)
    assert env.observation_spec.action_mask.shape == (A, 5)


def test_vector_connector_factory_rejects():
    from magpo_amd.config import compose
    from magpo_amd.utils import make_env as environments
    with pytest.raises(Exception):   # the grid-observation Connector (ConnectorWrapper) has no config here
        environments.make(compose("rec_magpo", ["env=connector"]))
    cfg = compose("rec_magpo", ["env=vector-connector"])
    cfg.env.env_name = "Connector"
    with pytest.raises(ValueError, match="not a supported environment"):
        environments.make(cfg)
    with pytest.raises(NotImplementedError):
        environments.make(compose("rec_magpo", ["env=vector-connector", "system.add_agent_id=False"]))
    with pytest.raises(NotImplementedError):
        environments.make(compose("rec_magpo", ["env=vector-connector", "+env.kwargs.penalty=1"]))


def _state(spec, grid, start, target, pos, step_count=0):
    """A one-env batch of the restatement's state on a hand-built board."""
    st = dict(grid=np.array(grid, np.int32)[None], agent_start=np.array(start, np.int32)[None], agent_target=np.array(target, np.int32)[None],
              agent_pos=np.array(pos, np.int32)[None], step_count=np.array([step_count], np.int32), key=np.zeros((1, 2), np.uint32))
    n = 1
    st.update(metrics_key=np.zeros((n, 2), np.uint32), running_return=np.zeros(n, np.float32), running_length=np.zeros(n, np.int32),
              episode_return=np.zeros(n, np.float32), episode_length=np.zeros(n, np.int32))
    return st


def test_observation_by_hand():
    """Both perspectives of a 5x5 board: /G^2 coordinates, the blockers and targets windows, padding 1 outside the grid."""
    spec = C.ConnectorSpec(5, 2, 10)
    grid = [[0, 0, 0, 0, 0],
            [0, 2, 1, 0, 0],    # agent 0: head (1, 1), path (1, 2), (2, 2)
            [0, 0, 1, 0, 6],    # agent 1: target (2, 4)
            [3, 0, 5, 4, 0],    # agent 0: target (3, 0); agent 1: head (3, 2), path (3, 3), (4, 3)
            [0, 0, 0, 4, 0]]
    st = _state(spec, grid, [[1, 2], [4, 3]], [[3, 0], [2, 4]], [[1, 1], [3, 2]])
    obs = C.make_obs(spec, st)
    view = obs["agents_view"][0]
    assert view.shape == (2, 56) and view.dtype == np.float32
    g2 = np.float32(25)
    want0 = [1, 0, np.float32(1) / g2, np.float32(1) / g2, np.float32(3) / g2, 0,
             1, 1, 1, 1, 1,
             1, 0, 0, 0, 0,
             1, 0, 1, -1, 0,
             1, 0, 0, -1, 0,
             1, 0, 0, 1, -1,
             1, 1, 1, 1, 1,
             1, 0, 0, 0, 0,
             1, 0, 0, 0, 0,
             1, 0, 0, 0, 0,
             1, 1, 0, 0, 0]
    want1 = [0, 1, np.float32(3) / g2, np.float32(2) / g2, np.float32(2) / g2, np.float32(4) / g2,
             0, 1, -1, 0, 0,
             0, 0, -1, 0, 0,
             0, 0, 1, -1, 0,
             0, 0, 0, -1, 0,
             1, 1, 1, 1, 1,
             0, 0, 0, 0, 0,
             0, 0, 0, 0, 1,
             -1, 0, 0, 0, 0,
             0, 0, 0, 0, 0,
             1, 1, 1, 1, 1]
    assert np.array_equal(view[0], np.array(want0, np.float32))
    assert np.array_equal(view[1], np.array(want1, np.float32))
    assert view[0, 2] == np.float32(0.04) and view[0, 2] != np.float32(1 / 5)   # row / G^2, not row / G
    # masks: agent 0 can go up / left (down is empty too; right is its own path); agent 1 right is its path, up is agent 0's path
    assert obs["action_mask"][0].tolist() == [[True, True, False, True, True], [True, False, False, True, True]]


def test_connection_step_by_hand():
    """Agent 0 steps onto its target: reward 0.1 - 0.03 for it and -0.03 for the other, summed in agent order and repeated; the
    target cell then holds its head, so my_target reads (0, 0) and the agent has only NOOP."""
    spec = C.ConnectorSpec(5, 2, 10)
    grid = [[0, 0, 0, 0, 0],
            [0, 2, 3, 0, 0],
            [0, 0, 0, 0, 0],
            [0, 0, 5, 0, 6],
            [0, 0, 0, 0, 0]]
    st = _state(spec, grid, [[1, 1], [3, 2]], [[1, 2], [3, 4]], [[1, 1], [3, 2]])
    st, ts = C.step(spec, st, np.array([[C.RIGHT, C.UP]]), auto_reset=False)
    assert st["grid"][0].tolist() == [[0, 0, 0, 0, 0],
                                      [0, 1, 2, 0, 0],
                                      [0, 0, 5, 0, 0],
                                      [0, 0, 4, 0, 6],
                                      [0, 0, 0, 0, 0]]
    assert st["agent_pos"][0].tolist() == [[1, 2], [2, 2]]
    per_agent = [np.float32(np.float32(0.1) + np.float32(-0.03)), np.float32(-0.03)]
    team = np.float32(np.float32(np.float32(0.0) + per_agent[0]) + per_agent[1])
    assert ts["reward"][0].tolist() == [team, team] and ts["reward"].dtype == np.float32
    assert ts["discount"][0].tolist() == [1.0, 1.0] and ts["step_type"][0] == C.STEP_MID
    view = ts["observation"]["agents_view"][0]
    assert view[0, 2:6].tolist() == [np.float32(1) / np.float32(25), np.float32(2) / np.float32(25), 0.0, 0.0]
    assert ts["observation"]["action_mask"][0, 0].tolist() == [True, False, False, False, False]
    assert ts["observation"]["step_count"][0].tolist() == [1, 1]
    # the next step gives the connected agent nothing, even for a move it tries
    st, ts = C.step(spec, st, np.array([[C.LEFT, C.NOOP]]), auto_reset=False)
    assert st["agent_pos"][0].tolist() == [[1, 2], [2, 2]]
    assert ts["reward"][0, 0] == np.float32(-0.03)


def test_collision_higher_id_wins():
    spec = C.ConnectorSpec(5, 2, 10)
    grid = [[0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0],
            [0, 2, 0, 5, 0],
            [3, 0, 0, 0, 6],
            [0, 0, 0, 0, 0]]
    st = _state(spec, grid, [[2, 1], [2, 3]], [[3, 0], [3, 4]], [[2, 1], [2, 3]])
    st, ts = C.step(spec, st, np.array([[C.RIGHT, C.LEFT]]), auto_reset=False)
    assert st["grid"][0].tolist() == [[0, 0, 0, 0, 0],
                                      [0, 0, 0, 0, 0],
                                      [0, 2, 5, 4, 0],
                                      [3, 0, 0, 0, 6],
                                      [0, 0, 0, 0, 0]]
    assert st["agent_pos"][0].tolist() == [[2, 1], [2, 2]]
    assert ts["reward"][0].tolist() == [np.float32(np.float32(-0.03) + np.float32(-0.03))] * 2
    # an illegal move (into another agent's path) and an off-grid move leave the agents in place
    grid = [[2, 4, 0, 0, 0],
            [0, 5, 0, 0, 0],
            [0, 0, 0, 0, 0],
            [0, 0, 0, 0, 6],
            [3, 0, 0, 0, 0]]
    st = _state(spec, grid, [[0, 0], [0, 1]], [[4, 0], [3, 4]], [[0, 0], [1, 1]])
    st2, _ = C.step(spec, st, np.array([[C.RIGHT, C.UP]]), auto_reset=False)
    assert np.array_equal(st2["grid"], st["grid"]) and np.array_equal(st2["agent_pos"], st["agent_pos"])
    st2, _ = C.step(spec, st, np.array([[C.UP, 7]]), auto_reset=False)
    assert np.array_equal(st2["grid"], st["grid"]) and np.array_equal(st2["agent_pos"], st["agent_pos"])


def test_termination_blocked_and_time_limit():
    spec = C.ConnectorSpec(5, 2, 10)
    grid = [[2, 4, 0, 0, 0],    # agent 0 in the corner, both neighbours hold agent 1's path
            [4, 5, 6, 0, 0],    # agent 1 one step from its target
            [0, 0, 0, 0, 0],
            [0, 0, 0, 0, 0],
            [0, 0, 0, 0, 3]]
    st = _state(spec, grid, [[0, 0], [0, 1]], [[4, 4], [1, 2]], [[0, 0], [1, 1]], step_count=3)
    st1, ts = C.step(spec, st, np.array([[C.NOOP, C.RIGHT]]), auto_reset=False)
    assert ts["step_type"][0] == C.STEP_LAST and ts["discount"][0].tolist() == [0.0, 0.0]
    assert ts["observation"]["action_mask"][0].tolist() == [[True, False, False, False, False]] * 2
    assert ts["episode_metrics"]["is_terminal_step"][0] and ts["episode_metrics"]["episode_length"][0] == 1
    # without the connection the episode goes on ...
    st1, ts = C.step(spec, st, np.array([[C.NOOP, C.NOOP]]), auto_reset=False)
    assert ts["step_type"][0] == C.STEP_MID and ts["discount"][0].tolist() == [1.0, 1.0]
    # ... until the time limit
    st9 = _state(spec, grid, [[0, 0], [0, 1]], [[4, 4], [1, 2]], [[0, 0], [1, 1]], step_count=9)
    _, ts = C.step(spec, st9, np.array([[C.NOOP, C.NOOP]]), auto_reset=False)
    assert ts["step_type"][0] == C.STEP_LAST and ts["discount"][0].tolist() == [0.0, 0.0]
    assert ts["observation"]["step_count"][0].tolist() == [10, 10]
    # with auto-reset the next observation is a fresh board at step 0; reward and discount stay the ending step's
    st9["key"][0] = prng.prng_key(3)
    st_r, ts = C.step(spec, st9, np.array([[C.NOOP, C.NOOP]]), auto_reset=True)
    assert ts["step_type"][0] == C.STEP_LAST and ts["observation"]["step_count"][0].tolist() == [0, 0]
    fresh = C._generate(spec, prng.split(st9["key"][0], 2)[0])
    assert np.array_equal(st_r["grid"][0], fresh["grid"]) and st_r["step_count"][0] == 0


def _walk_connected(walked, G, i, start, final):
    """BFS from the start over agent i's walked cells (its path and its final head)."""
    mine = {c for c in range(G * G) if walked[c] in (C.path_value(i), C.position_value(i))}
    seen, todo = {int(start)}, [int(start)]
    while todo:
        c = todo.pop()
        r, q = divmod(c, G)
        for dr, dq in ((-1, 0), (0, 1), (1, 0), (0, -1)):
            rr, qq = r + dr, q + dq
            n = rr * G + qq
            if 0 <= rr < G and 0 <= qq < G and n in mine and n not in seen:
                seen.add(n)
                todo.append(n)
    return int(final) in seen


@pytest.mark.parametrize("G,A,n", [(5, 3, 150), (7, 5, 60), (10, 10, 25), (15, 23, 8)])
def test_generator_invariants(G, A, n):
    spec = C.ConnectorSpec(G, A, 4 * G)
    for k in prng.split(prng.prng_key(G * 100 + A), n):
        _, board_key = prng.split(k, 2)
        starts, finals, walked = C.random_walk(spec, board_key)
        assert len(set(starts.tolist())) == A, "distinct starts"
        assert len(set(finals.tolist())) == A
        for i in range(A):
            assert walked[starts[i]] in (C.path_value(i), C.position_value(i))
            assert _walk_connected(walked, G, i, starts[i], finals[i]), "each target is reachable along that agent's walk"
        nbrs = C._neighbours(G, np.stack(np.divmod(finals, G), axis=1))
        assert not ((nbrs >= 0) & (walked[np.maximum(nbrs, 0)] == 0)).any(), "the walk stops only when no head has an empty neighbour"
        st = C._generate(spec, k)
        board = st["grid"].reshape(-1)
        heads, targets = board[board % 3 == 2], board[(board % 3 == 0) & (board != 0)]
        assert len(heads) == len(set(heads.tolist())) and len(targets) == len(set(targets.tolist()))
        assert len(targets) == A and not (board % 3 == 1).any(), "every target on the board, no paths"
        moved = (st["agent_start"] != st["agent_target"]).any(-1)
        assert len(heads) == int(moved.sum()), "one head per agent that walked (a never-moved agent's target owns its start)"
        assert np.array_equal(st["agent_pos"], st["agent_start"]) and st["step_count"] == 0
        assert np.array_equal(st["key"], prng.split(k, 2)[0])


def test_restatement_contract():
    """reset / step have oracle/rware.py's timestep layout (what OracleLearner and oracle.evaluator read)."""
    spec = C.ConnectorSpec(5, 3, 25)
    keys = prng.split(prng.prng_key(0), 6)
    st, ts = C.reset(spec, keys)
    assert ts["observation"]["agents_view"].shape == (6, 3, 57) and ts["observation"]["action_mask"].shape == (6, 3, 5)
    assert ts["step_type"].tolist() == [C.STEP_FIRST] * 6 and (ts["reward"] == 0).all() and (ts["discount"] == 1).all()
    assert (ts["observation"]["step_count"] == 0).all()
    assert np.array_equal(ts["observation"]["agents_view"][:, :, :3], np.broadcast_to(np.eye(3, dtype=np.float32), (6, 3, 3)))
    rng = np.random.default_rng(0)
    ends = 0
    for _ in range(60):
        st, ts = C.step(spec, st, rng.integers(0, 5, (6, 3)), auto_reset=True)
        ends += int((ts["step_type"] == C.STEP_LAST).sum())
        assert ts["reward"].dtype == np.float32 and (ts["reward"] == ts["reward"][:, :1]).all()
    assert ends > 0
