"""`python -m oc_cleanrl_amd.lstm [ppo_atari_lstm.py flags]` — the recurrent (LSTM) PPO agent of
cleanrl/ppo_atari_lstm.py on HBM-resident state.

The script's loop is cleanrl's PPO (GAE, the clipped loss, Adam(eps=1e-5)) with three changes, all
restated here on `trainer.PPOTrainer`:
  * the agent (:117-170) puts a single-layer nn.LSTM between the trunk and the two heads and
    multiplies the state that enters a step by 1 - done (:148-156), one nn.LSTM call per step;
  * the rollout carries (h, c) across steps and iterations and snapshots the state each rollout
    starts from (:234), which every minibatch's recomputation starts from again (:310);
  * minibatches are whole environments: the epoch shuffles ENVIRONMENT indices and a minibatch is
    all T steps of num_envs / num_minibatches of them, time-major (:296-306).

`LSTMAgent` holds the reference's submodules (same construction order, so the same state-dict
keys and seeded init for architecture="PPO" with one stacked frame) and runs the recurrence on
the fused kernels (csrc/ocppo_lstm.hip): `pre = hidden W_ih^T + b_ih` as ONE Linear over all T * B
rows (agents.linear_act), then ops.lstm_seq -- one launch forward, one backward -- in the update,
and ops.lstm_step per env step in the rollout. `FUSED_LSTM = False`, a shape outside
ops.lstm_shape_ok, or tensors that are not GPU f32 select the reference's per-step torch loop.

Declared differences from the script: no ALE here (--backend Synthetic, the package's device
envs); `architecture` / `obs_mode` pick the trunk (the object-vector PPObj encoder / decoder by
default, "PPO" = the script's NatureCNN); the final evaluation (eval_episodes) is not offered
for a stateful agent; one GPU.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .agents import EnvSpec, _ActorCritic, fused_trunk, layer_init, linear_act, object_trunk
from .args import (CORE_FIXED, CORE_SKIP, check_sampling_noise, learner_args,
                   single_gpu_sizes)
from .trainer import PPOTrainer, learner_main, run

# The fused recurrence (ops.lstm_seq / ops.lstm_step); False: the reference's per-step nn.LSTM loop.
FUSED_LSTM = True

ARCHITECTURES = ("PPO_OBJ", "PPO")

# ppo_atari_lstm.py:27-86, same names, order and defaults
_REFERENCE_FIELDS = [
    ("exp_name", str, "ppo_atari_lstm"), ("seed", int, 1), ("torch_deterministic", bool, True),
    ("cuda", bool, True), ("track", bool, False), ("wandb_project_name", str, "cleanRL"),
    ("wandb_entity", Optional[str], None), ("capture_video", bool, False),
    ("env_id", str, "BreakoutNoFrameskip-v4"), ("total_timesteps", int, 10_000_000),
    ("learning_rate", float, 2.5e-4), ("num_envs", int, 8), ("num_steps", int, 128),
    ("anneal_lr", bool, True), ("gamma", float, 0.99), ("gae_lambda", float, 0.95),
    ("num_minibatches", int, 4), ("update_epochs", int, 4), ("norm_adv", bool, True),
    ("clip_coef", float, 0.1), ("clip_vloss", bool, True), ("ent_coef", float, 0.01),
    ("vf_coef", float, 0.5), ("max_grad_norm", float, 0.5), ("target_kl", Optional[float], None),
    ("batch_size", int, 0), ("minibatch_size", int, 0), ("num_iterations", int, 0),
]
# [oc_cleanrl_amd] additions: what PPOTrainer reads beyond the script's flags (args.Args' own
# defaults unless listed), the trunk choice, the observation geometry and the LSTM width
_OWN_DEFAULTS = {"architecture": "PPO_OBJ", "obs_mode": "obj", "backend": "Synthetic",
                 "vecnorm_reward": False,  # the script clips rewards and has no VecNormalize
                 "encoder_dims": (128, 64), "decoder_dims": (128,)}
_OWN_FIELDS = [("lstm_hidden", int, 128)]  # nn.LSTM(trunk_out, 128) at :131

LSTMArgs = learner_args(
    "LSTMArgs", "The flags of ppo_atari_lstm.py:27-86 (same names, order and defaults) + this "
                "build's additions.",
    _REFERENCE_FIELDS, CORE_SKIP, _OWN_DEFAULTS, _OWN_FIELDS, CORE_FIXED)


def finalize(args, world_size: int = 1):
    """Derived sizes (ppo_atari_lstm.py:175-177), the script's assertion at :296 and the checks of
    args.finalize that apply."""
    if args.architecture not in ARCHITECTURES:
        raise NotImplementedError(f"architecture must be one of {ARCHITECTURES}")
    if (args.obs_mode == "obj") != (args.architecture == "PPO_OBJ"):
        raise ValueError('architecture PPO_OBJ reads --obs_mode obj, PPO reads pixels (dqn)')
    if args.num_envs % args.num_minibatches:
        raise ValueError(f"num_envs={args.num_envs} must be divisible by num_minibatches="
                         f"{args.num_minibatches}: a minibatch is whole environments")
    single_gpu_sizes(args, world_size, "the LSTM learner")
    if not ops.lstm_shape_ok(args.num_steps, args.num_envs // args.num_minibatches, 1,
                             args.lstm_hidden):
        raise ValueError(f"lstm_hidden={args.lstm_hidden} with num_steps={args.num_steps}: the "
                         f"LSTM kernels take a hidden size in {ops.LSTM_HIDDEN} and >= 1 step")
    check_sampling_noise(args)
    return args


def epoch_indices(envinds: np.ndarray, rng, num_steps: int, num_minibatches: int) -> np.ndarray:
    """One epoch's sample order (ppo_atari_lstm.py:302-306): shuffle the environment indices IN
    PLACE (they carry over from epoch to epoch of an iteration, as the script's `envinds` does),
    then every minibatch is `flatinds[:, mbenvinds].ravel()` -- all steps of its environments,
    time-major -- and the minibatches follow each other. Returns [num_steps * num_envs] i64."""
    n = envinds.shape[0]
    per = n // num_minibatches
    rng.shuffle(envinds)
    flatinds = np.arange(num_steps * n).reshape(num_steps, n)
    return np.concatenate([flatinds[:, envinds[s:s + per]].ravel() for s in range(0, n, per)])


def lstm_ok(hidden, done, lstm_state, H: int) -> bool:
    """The fused path applies: the module switch, GPU f32 tensors and ops.lstm_shape_ok."""
    h0 = lstm_state[0]
    if not (FUSED_LSTM and hidden.is_cuda and hidden.dtype == torch.float32 and h0.is_cuda and
            h0.dtype == torch.float32 and done.is_cuda and hidden.dim() == 2 and h0.dim() == 3
            and h0.shape[0] == 1 and h0.shape[1] >= 1 and hidden.shape[0] % h0.shape[1] == 0):
        return False
    B = h0.shape[1]
    return ops.lstm_shape_ok(hidden.shape[0] // B, B, hidden.shape[1], H)


class Recurrence:
    """The masked single-layer recurrence (:144-158) of a module that holds `self.lstm`, an
    nn.LSTM: the fused kernels under lstm_ok, else the reference's per-step torch loop. Shared by
    LSTMAgent and the recurrent PQN network (pqn_lstm.PQNLSTMNetwork)."""

    @property
    def _ih(self):
        return SimpleNamespace(weight=self.lstm.weight_ih_l0, bias=self.lstm.bias_ih_l0)

    def recur(self, hidden, lstm_state, done):
        """:144-158 on the trunk output `hidden` [T * B, I] (time-major): (new_hidden [T * B, H],
        (h, c) [1, B, H])."""
        B = lstm_state[0].shape[1]
        H = self.lstm.hidden_size
        if lstm_ok(hidden, done, lstm_state, H):
            T = hidden.shape[0] // B
            pre = linear_act(hidden, self._ih, False)
            out, (hT, cT) = ops.lstm_seq(
                pre.view(T, B, 4 * H), self.lstm.weight_hh_l0, self.lstm.bias_hh_l0,
                done.reshape(T, B).to(torch.float32).contiguous(),
                lstm_state[0][0].contiguous(), lstm_state[1][0].contiguous())
            return out.view(T * B, H), (hT.unsqueeze(0), cT.unsqueeze(0))
        hidden = hidden.reshape((-1, B, self.lstm.input_size))
        done = done.reshape((-1, B))
        new_hidden = []
        for h, d in zip(hidden, done):
            h, lstm_state = self.lstm(h.unsqueeze(0), ((1.0 - d).view(1, -1, 1) * lstm_state[0],
                                                       (1.0 - d).view(1, -1, 1) * lstm_state[1]))
            new_hidden += [h]
        return torch.flatten(torch.cat(new_hidden), 0, 1), lstm_state

    def step_(self, x, done, h, c):
        """One rollout step on the trunk output x [N, I]: h, c [N, H] updated in place; returns h.
        ops.lstm_step (one launch), or one pass of the torch loop."""
        state = (h.unsqueeze(0), c.unsqueeze(0))
        if lstm_ok(x, done, state, self.lstm.hidden_size):
            ops.lstm_step(x, self.lstm.weight_ih_l0, self.lstm.bias_ih_l0, self.lstm.weight_hh_l0,
                          self.lstm.bias_hh_l0, done, h, c)
            return h
        _, (hn, cn) = self.recur(x, state, done)
        h.copy_(hn[0])
        c.copy_(cn[0])
        return h

    def get_states(self, x, lstm_state, done):
        return self.recur(self.trunk(x), lstm_state, done)


def init_lstm(lstm: nn.LSTM) -> nn.LSTM:
    """:132-136: zero biases, orthogonal (gain 1) weights, in named_parameters' order."""
    for name, param in lstm.named_parameters():
        if "bias" in name:
            nn.init.constant_(param, 0)
        elif "weight" in name:
            nn.init.orthogonal_(param, 1.0)
    return lstm


class LSTMAgent(_ActorCritic, Recurrence):
    """Agent of ppo_atari_lstm.py:117-170 on a trunk of this package: architecture "PPO" is the
    script's network (NatureCNN + Linear(3136, 512), x / 255 in get_states) with the script's
    state-dict keys; "PPO_OBJ" is the PPObj encoder / decoder on object vectors."""

    # the torch path's nn.LSTM reaches .grad through AccumulateGrad: the trainer zeroes the flat
    # gradient buffer per minibatch (PPOTrainer.direct_grads)
    grads_in_place = False

    def __init__(self, envs, architecture: str = "PPO", lstm_hidden: int = 128, device=None,
                 encoder_dims=(128, 64), decoder_dims=(128,)):
        super().__init__()
        if architecture not in ARCHITECTURES:
            raise NotImplementedError(architecture)
        self.device = device
        self.pixels = architecture == "PPO"
        dims = tuple(envs.observation_space.shape)
        if self.pixels:
            net = nn.Sequential(
                layer_init(nn.Conv2d(dims[0], 32, 8, stride=4)), nn.ReLU(),
                layer_init(nn.Conv2d(32, 64, 4, stride=2)), nn.ReLU(),
                layer_init(nn.Conv2d(64, 64, 3, stride=1)), nn.ReLU(), nn.Flatten())
            with torch.no_grad():
                feat = net(torch.zeros((1,) + dims)).shape[1]
            net.append(layer_init(nn.Linear(feat, 512)))
            net.append(nn.ReLU())
            self.network, d = net, 512
        else:
            layers, d = object_trunk(dims, tuple(encoder_dims), tuple(decoder_dims), layer_init)
            self.network = nn.Sequential(*layers)
        self.lstm = init_lstm(nn.LSTM(d, lstm_hidden))
        self.actor = layer_init(nn.Linear(lstm_hidden, envs.action_space.n), std=0.01)
        self.critic = layer_init(nn.Linear(lstm_hidden, 1), std=1)

    def trunk(self, x, prescaled: bool = False):
        """The LSTM's input [rows, trunk_out] (:141); pixels are divided by 255 here."""
        if self.pixels and not prescaled:
            x = x / 255.0
        return fused_trunk(self.network, x)

    def get_value(self, x, lstm_state, done):
        hidden, _ = self.get_states(x, lstm_state, done)
        return self._head(self.critic, hidden)

    def get_action_and_value(self, x, lstm_state, done, action=None):
        """(action, log_prob, entropy, value [rows, 1], lstm_state) as :164-170."""
        hidden, lstm_state = self.get_states(x, lstm_state, done)
        logits, value = self.heads(hidden)
        if not logits.is_cuda:
            probs = torch.distributions.Categorical(logits=logits)
            if action is None:
                action = probs.sample()
            return action, probs.log_prob(action), probs.entropy(), value, lstm_state
        if action is None:
            noise = torch.empty_like(logits, dtype=torch.float32).exponential_()
            action, lp, _ = ops.categorical_sample(logits.detach().float().contiguous(), noise)
        lp, ent = ops.categorical_logprob_entropy(logits.float(), action)
        return action, lp, ent, value, lstm_state

    def forward(self, x, lstm_state, done):
        return self.get_states(x, lstm_state, done)

    def predict(self, x, states=None, **_):
        raise NotImplementedError("a recurrent agent needs its state: use get_action_and_value")


class LSTMTrainer(PPOTrainer):
    """PPOTrainer with the recurrent agent: (h, c) [N, H] carried across rollout steps and
    iterations, the state each rollout started from kept for the update, environment-wise
    minibatches, and the LSTM between the trunk and the heads in both phases."""

    def __init__(self, args, device, *a, **k):
        super().__init__(args, device, *a, **k)
        N, H = self.N, self.agent.lstm.hidden_size
        self.envs_per_mb = N // self.nmb
        f32 = torch.float32
        self.lstm_h = torch.zeros((N, H), dtype=f32, device=self.dev)  # next_lstm_state (:228)
        self.lstm_c = torch.zeros((N, H), dtype=f32, device=self.dev)
        self.init_h = torch.zeros_like(self.lstm_h)  # initial_lstm_state (:234)
        self.init_c = torch.zeros_like(self.lstm_c)
        self.boot_h = torch.zeros_like(self.lstm_h)  # the bootstrap's throw-away state (:268)
        self.boot_c = torch.zeros_like(self.lstm_c)

    def _make_agent(self) -> nn.Module:
        a = self.args
        return LSTMAgent(EnvSpec(self.obs_shape, self.A), a.architecture, a.lstm_hidden, None,
                         a.encoder_dims, a.decoder_dims)

    # ---- rollout ---------------------------------------------------------------------------
    def _rollout_begin(self):
        super()._rollout_begin()
        self.init_h.copy_(self.lstm_h)
        self.init_c.copy_(self.lstm_c)

    def _act(self, t: int, env_step: bool = False, hidden=None) -> bool:
        """Step t: trunk -> LSTM step on (the carried state, dones[t] = next_done) -> heads."""
        x = self._policy_hidden(t)
        hidden = self.timer.bracket("lstm_step", lambda: self.agent.step_(
            x, self.dones[t], self.lstm_h, self.lstm_c))
        return super()._act(t, env_step, hidden=hidden)

    def _bootstrap_value(self):
        """:267-272: the value of next_obs through the LSTM with the last state and next_done; the
        state that step returns is dropped, so it runs on a copy."""
        T = self.T
        self.boot_h.copy_(self.lstm_h)
        self.boot_c.copy_(self.lstm_c)
        h = self.agent.step_(self._policy_hidden(T), self.dones[T], self.boot_h, self.boot_c)
        return self.agent._head(self.agent.critic, h)

    # ---- update ----------------------------------------------------------------------------
    def _shuffle(self):
        """np.random.shuffle(envinds) once per epoch (:302), all epochs up front; every
        minibatch's flat indices time-major (epoch_indices) into the usual permutation staging."""
        self.perm_event.synchronize()
        out = self.perm_host.numpy()
        self.staged_rng_state = self.np_rng.get_state()
        envinds = np.arange(self.N)  # envinds = np.arange(num_envs) every iteration (:298)
        for e in range(self.E):
            out[e * self.B:(e + 1) * self.B] = epoch_indices(envinds, self.np_rng, self.T, self.nmb)
        self._stage(out)

    def _rewind_shuffle(self, epochs: int):
        self.np_rng.set_state(self.current_rng_state)
        b = np.arange(self.N)
        for _ in range(epochs):
            self.np_rng.shuffle(b)

    def _minibatch_hidden(self, j: int):
        """Trunk on the minibatch's rows, one Linear for the input projection of all T * B rows,
        the recurrence from that minibatch's slice of the initial state and its dones (:308-313)."""
        idx = self.perm_dev[j * self.M:(j + 1) * self.M]
        x = super()._minibatch_hidden(j)
        envs = idx[:self.envs_per_mb]  # row t = 0 of flatinds[:, mbenvinds]: the env indices
        state = (self.init_h.index_select(0, envs).unsqueeze(0),
                 self.init_c.index_select(0, envs).unsqueeze(0))
        done = self.dones[:self.T].view(-1).index_select(0, idx)
        hidden, _ = self.agent.recur(x, state, done)
        return hidden


def run_lstm(args, device=None) -> LSTMTrainer:
    return run(args, device, trainer_cls=LSTMTrainer)


def main(argv=None):
    return learner_main(LSTMArgs, finalize, run_lstm,
                        "oc_cleanrl_amd recurrent PPO (ppo_atari_lstm.py surface)", argv)


if __name__ == "__main__":
    main()
