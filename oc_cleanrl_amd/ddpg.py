"""`python -m oc_cleanrl_amd.ddpg [ddpg_continuous_action.py flags]` — Deep Deterministic Policy
Gradient.

The same learner as `python -m oc_cleanrl_amd.td3` (td3.TD3Trainer) with
cleanrl/ddpg_continuous_action.py's Args (:18-65: no policy_noise) and its two differences from
td3_continuous_action.py: one critic (:161-166, :217-221: ops.td3_critic_loss_fwd_bwd with q2 =
None) and no target-policy noise (:216: ops.td3_target_actions with policy_noise 0, which draws
nothing and does not clamp). `noise_clip` is a flag of the script that it never reads. The
checkpoint is (actor, qf1) (:249) and the metrics are the script's three (:241-243). num_envs is
this build's addition: the script is fixed at one env."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

from .td3 import TD3Trainer, main as _main, run_td3


@dataclass
class DDPGArgs:
    """The flags of ddpg_continuous_action.py:18-65 (same names, order and defaults; env_id as
    td3.TD3Args) + this build's additions."""
    exp_name: str = "ddpg_continuous_action"
    seed: int = 1
    torch_deterministic: bool = True
    cuda: bool = True
    track: bool = False
    wandb_project_name: str = "cleanRL"
    wandb_entity: Optional[str] = None
    capture_video: bool = False
    save_model: bool = False
    upload_model: bool = False
    hf_entity: str = ""
    env_id: str = "Pendulum-v1"
    total_timesteps: int = 1000000
    learning_rate: float = 3e-4
    buffer_size: int = int(1e6)
    gamma: float = 0.99
    tau: float = 0.005
    batch_size: int = 256
    exploration_noise: float = 0.1
    learning_starts: float = 25e3  # as td3.TD3Args: int() where compared
    policy_frequency: int = 2
    noise_clip: float = 0.5

    # [oc_cleanrl_amd] additions
    num_envs: int = 1
    backend: str = "Synthetic"
    cuda_graphs: bool = True
    log_dir: str = "runs"
    log_every: int = 100

    # the mode switch and what run_learner / learner_main read (no annotation: not flags)
    obs_mode = "obj"
    twin = False
    policy_noise = 0.0

    @property
    def train_frequency(self) -> int:
        return self.policy_frequency


DDPGTrainer = TD3Trainer  # the mode is the args' (`twin`)
run_ddpg = run_td3


def main(argv=None):
    return _main(argv, DDPGArgs, "oc_cleanrl_amd DDPG (ddpg_continuous_action.py surface)")


if __name__ == "__main__":
    main()
