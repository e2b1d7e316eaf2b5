"""ff_mappo system entry point on MI355X -- drop-in for mava/systems/ppo/anakin/ff_mappo.py: a feed-forward actor and a centralised feed-forward critic under PPO.

Same public names and call contract as the reference system file (get_learner_fn, learner_setup, run_experiment, hydra_entry_point); the
implementation is shared with ff_ippo (magpo_amd/systems/ppo/anakin/ff_ppo.py).

    python -m magpo_amd.systems.ppo.anakin.ff_mappo env=coordsum env/scenario=3x30-50 arch.num_envs=64
"""
from magpo_amd.systems.ppo.anakin.ff_ppo import make_system
from magpo_amd.systems.ppo.types import LearnerState, OptStates, Params, PPOTransition  # noqa: F401
from magpo_amd.types import ExperimentOutput  # noqa: F401

_system = make_system("ff_mappo", centralised=True)
get_learner_fn = _system.get_learner_fn
learner_setup = _system.learner_setup
run_experiment = _system.run_experiment
hydra_entry_point = _system.hydra_entry_point

if __name__ == "__main__":
    hydra_entry_point()
