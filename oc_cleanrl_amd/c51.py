"""C51 (categorical DQN) learner of cleanrl/c51_atari_oc.py on HBM-resident state.

The reference's second off-policy learner runs on the loop of dqn_atari_oc.py: the same SB3
replay, epsilon-greedy coin and schedule, VecNormalize(norm_reward=True) and NatureCNN trunk. It
differs in the head (A * n_atoms logits, a softmax per action over a fixed support `atoms`,
architectures/dqn.py:36-72) and in the train step (c51_atari_oc.py:337-370): the target net's
greedy next action by expected value, the categorical projection of r + gamma * atoms * (1 - d)
onto the support (a Python loop of 2 * B index_add_ calls), the clamped cross entropy against the
taken action's pmf, Adam with eps = 0.01 / batch_size (:275), and a HARD target copy every
`target_network_frequency` steps (:373-374, no tau).

`C51Trainer` is `dqn.DQNTrainer` with those pieces replaced:
  ops.c51_epsilon_greedy  expected Q per action + the epsilon-greedy choice, one launch
  ops.c51_loss_fwd_bwd    :339-359 and its backward w.r.t. the online logits, one launch
everything else (env, store + VecNormalize, replay, FlatAdam, the fill / train chunk hipGraphs) is
the DQN learner's.

`QNetworkC51` is QNetwork_C51 (module layout, init order and state-dict keys equal, the `atoms`
buffer built by torch.linspace on the CPU before .to(device)); `QNetworkC51Obj` is this build's
declared extension for object vectors, as `dqn.QNetworkObj`: the PPObj trunk with an A * n_atoms
head.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .agents import Predictor, fused_trunk, nature_cnn, object_trunk, q_head
from .dqn import DQNTrainer, check_actions, check_atoms, learner_main, run_learner


@dataclass
class C51Args:
    """The flags of c51_atari_oc.py:53-140 (same names and defaults) + this build's additions."""
    exp_name: str = "c51_atari_oc"
    seed: int = 42
    torch_deterministic: bool = True
    cuda: bool = True
    env_id: str = "ALE/Pong-v5"
    obs_mode: str = "dqn"
    feature_func: str = ""
    buffer_window_size: int = 4
    backend: str = "Synthetic"  # reference: OCAtari (ALE not available here)
    modifs: str = ""
    new_rf: str = ""
    frameskip: int = 4
    track: bool = False
    wandb_project_name: str = "OC-Transformer"
    wandb_entity: str = "AIML_OC"
    wandb_dir: Optional[str] = None
    capture_video: bool = False
    ckpt: str = ""
    logging_level: int = 40
    author: str = "JB"
    architecture: str = "C51"
    total_timesteps: int = 20_000_000
    learning_rate: float = 2.5e-4
    num_envs: int = 1
    n_atoms: int = 51
    v_min: float = -10.0
    v_max: float = 10.0
    buffer_size: int = 1_000_000
    gamma: float = 0.99
    target_network_frequency: int = 10000
    batch_size: int = 32
    start_e: float = 1.0
    end_e: float = 0.01
    exploration_fraction: float = 0.10
    learning_starts: int = 80000
    train_frequency: int = 4
    test_modifs: str = ""

    # [oc_cleanrl_amd] additions (as DQNArgs)
    num_features: int = 12      # object-vector width F per frame (synthetic obj env)
    obs_storage: str = "auto"   # replay obs dtype: auto (u8 pixels / bf16 objects) | f32 | bf16 | u8
    encoder_dims: tuple = (256, 512, 1024, 512)  # QNetworkC51Obj (obs_mode obj)
    decoder_dims: tuple = (512,)
    cuda_graphs: bool = True
    gemm_table: bool = False
    vecnorm_reward: bool = True  # VecNormalize(norm_reward=True) of c51_atari_oc.py:260
    log_dir: str = "runs"
    save_model: bool = True
    log_every: int = 100        # the reference logs loss / q_values every 100 steps


class QNetworkC51(Predictor):
    """architectures/dqn.py:36-72: NatureCNN with an A * n_atoms head; class defaults as there."""

    def __init__(self, obs_shape, n_actions, n_atoms=101, v_min=-100, v_max=100):
        super().__init__()
        self.n_atoms = n_atoms
        self.register_buffer("atoms", torch.linspace(v_min, v_max, steps=n_atoms))
        self.n = n_actions
        self.network = nn.Sequential(*nature_cnn(obs_shape[0]), nn.Linear(3136, 512), nn.ReLU(),
                                     nn.Linear(512, self.n * n_atoms))

    def _scale(self, x):
        return x / 255.0

    def forward(self, x):
        return self.network(self._scale(x))

    def logits(self, x):
        """[len(x), A * n_atoms] through the fused Linear / convolution path (same math as
        forward)."""
        return q_head(fused_trunk(self.network[:-1], self._scale(x)), self.network[-1])

    def _pmfs_q(self, x):
        logits = self.logits(x) if x.is_cuda else self.forward(x)
        pmfs = torch.softmax(logits.view(len(x), self.n, self.n_atoms), dim=2)
        return pmfs, (pmfs * self.atoms).sum(2)

    def get_action(self, x, action=None):
        """:57-64 — (greedy or given action, that action's pmf [len(x), n_atoms])."""
        pmfs, q_values = self._pmfs_q(x)
        if action is None:
            action = torch.argmax(q_values, 1)
        return action, pmfs[torch.arange(len(x)), action]

    def get_action_and_value(self, x):
        """:66-72 (greedy action; q_values[:, action] keeps the reference's [B, B] shape)."""
        _, q_values = self._pmfs_q(x)
        action = torch.argmax(q_values, 1)
        return action, q_values[:, action], None, None

    def predict(self, x, states=None, **_):
        with torch.no_grad():
            dev = next(self.parameters()).device
            _, q = self._pmfs_q(torch.as_tensor(np.asarray(x), dtype=torch.float32, device=dev))
            return np.argmax(q.cpu().numpy(), axis=1), states


class QNetworkC51Obj(QNetworkC51):
    """[oc_cleanrl_amd extension] object-vector C51 network: PPObj's trunk + an A * n_atoms head
    (what dqn.QNetworkObj is to QNetwork); inputs are not scaled."""

    def __init__(self, obs_shape, n_actions, n_atoms=101, v_min=-100, v_max=100,
                 encoder_dims=(256, 512, 1024, 512), decoder_dims=(512,)):
        Predictor.__init__(self)
        self.n_atoms = n_atoms
        self.register_buffer("atoms", torch.linspace(v_min, v_max, steps=n_atoms))
        self.n = n_actions
        layers, d = object_trunk(obs_shape, encoder_dims, decoder_dims)
        self.network = nn.Sequential(*layers, nn.Linear(d, self.n * n_atoms))

    def _scale(self, x):
        return x


def make_c51net(args: C51Args, obs_shape, n_actions) -> nn.Module:
    kw = dict(n_atoms=args.n_atoms, v_min=args.v_min, v_max=args.v_max)  # :274
    if args.obs_mode == "obj":
        return QNetworkC51Obj(obs_shape, n_actions, encoder_dims=args.encoder_dims,
                              decoder_dims=args.decoder_dims, **kw)
    return QNetworkC51(obs_shape, n_actions, **kw)


class C51Trainer(DQNTrainer):
    """DQNTrainer's loop (env step, store + VecNormalize, replay, chunk graphs) with the C51
    network, acting rule, train step and hard target copy."""

    def __init__(self, args: C51Args, device, log: bool = True):
        check_atoms(args.n_atoms)
        super().__init__(args, device, log)
        check_actions(self.A, "C51")
        self.fused_act = False  # DQN's Q-head launch does not apply: acting is self._act
        B = args.batch_size
        self.dlogits = torch.zeros((B, self.A * args.n_atoms), dtype=torch.float32,
                                   device=self.dev)

    def _make_net(self) -> nn.Module:
        return make_c51net(self.args, self.obs_shape, self.A)

    def _adam_eps(self) -> float:
        return 0.01 / self.args.batch_size  # :275

    def _act(self, k: int):
        """:303-308 — expected Q per action and the epsilon-greedy choice in one launch."""
        a = self.args
        ops.c51_epsilon_greedy(self.q.logits(self.net_obs), self.q.atoms, a.seed, self.step_dev,
                               a.start_e, a.end_e, self.duration, self.actions, self.epsilon,
                               step_offset=k + 1)

    def _train_step(self):
        """:337-370 — sample, two forwards, projection + loss + d loss / d logits (fused),
        backward, Adam."""
        a = self.args
        d = self.rb.sample(a.batch_size, out=self.batch)
        with torch.no_grad():
            logits_next = self.target.logits(d["next_observations"])
        logits = self.q.logits(d["observations"])
        ops.c51_loss_fwd_bwd(logits.detach(), logits_next, self.target.atoms, d["actions"],
                             d["rewards"], d["dones"], a.gamma, a.v_min, a.v_max,
                             dlogits=self.dlogits, stats=self.td_stats)
        if not self.direct_grads:
            self.opt.zero_grad()
        logits.backward(self.dlogits)
        self.opt.step()

    def _target_update(self):
        """:373-374 — target_network.load_state_dict(q_network.state_dict()) (the atoms buffer is
        constant)."""
        self.t_flat.copy_(self.opt.params)

    LOSS_KEY = "losses/loss"


def run_c51(args: C51Args, device=None) -> C51Trainer:
    return run_learner(C51Trainer, args, device)


def main(argv=None):
    learner_main(C51Args, run_c51, "oc_cleanrl_amd C51 (c51_atari_oc.py surface)", argv)


if __name__ == "__main__":
    main()
