"""`python -m oc_cleanrl_amd.pqn [pqn_atari_envpool.py flags]` — PQN (cleanrl/pqn_atari_envpool.py)
on the device rollout of `trainer.PPOTrainer`.

PQN is the value-based learner with the PPO loop's shape: no replay buffer and no target network,
a T-step vectorised rollout with epsilon-greedy acting (:217-232), Q(lambda) targets from a reverse
scan (:248-261), then epochs of shuffled minibatches of an MSE loss on the taken action's Q value
(:269-283) under RAdam with the gradient norm clipped at 10. Restated here on the trainer's HBM
rollout buffer, captured rollout, minibatch staging, flat parameter buffer and hipGraphs:
  * `_act` is the Q head + greedy value + epsilon-greedy action in one launch (ops.pqn_act) into
    actions[t] / values[t] (the log-prob row is unused);
  * the rollout's end evaluates q_network(next_obs) and runs ops.q_lambda into `returns`;
  * a minibatch is trunk -> Q head -> ops.pqn_loss_fwd_bwd -> backward, then ops.FlatRAdam;
  * every `Linear -> LayerNorm -> ReLU` on 2-D rows is agents.linear_act (no ReLU) + ops.ln_relu
    in the rollout; in the update the LayerNorm + ReLU stay on torch unless FUSED_LN_UPDATE (the
    kernel pair measured slower than torch's there).
`FUSED_PQN = False` selects torch's F.layer_norm / relu, torch's argmax for the greedy value,
F.mse_loss and torch.optim.RAdam instead (the exploration draw stays ops.epsilon_greedy: the
package's one stream, so both paths act alike from one seed).

Declared differences from the script: no envpool / ALE here (--backend Synthetic, the package's
device envs); `architecture` / `obs_mode` pick the network ("PQN_OBJ", the default: the PPObj
encoder / decoder on object vectors with a LayerNorm before every ReLU; "PQN": the script's
QNetwork on pixels, whose LayerNorms over [C, H, W] stay on torch); exploration is
ocppo_epsilon_greedy's law (one coin per global step for the whole vector of envs, the
counter-based stream), not torch.rand per env; one GPU.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .agents import EnvSpec, Predictor, layer_init, linear_act, object_trunk
from .args import CORE_FIXED, CORE_SKIP, learner_args, single_gpu_sizes
from .trainer import PPOTrainer, learner_main, run

# The fused kernels (ops.ln_relu, ops.pqn_act, ops.pqn_loss_fwd_bwd, ops.FlatRAdam); False:
# torch's layer_norm / relu, argmax, mse_loss and optim.RAdam.
FUSED_PQN = True
# ops.ln_relu also under autograd (the update's forward + backward). Off: at the update's row
# shapes (128 envs x 128 steps, 4 minibatches) the kernel pair measured slower than torch's
# layer_norm + relu with autograd -- 78.6 vs 73.9 us at [16384, 128], 69.3 vs 66.0 at [16384, 64],
# 42.5 vs 28.5 at [4096, 128] (tools/pqn_rate.py) -- so the update's LayerNorms run on
# torch; the rollout's rows (3.1 vs 5.4 us) run on the kernel
FUSED_LN_UPDATE = False

ARCHITECTURES = ("PQN_OBJ", "PQN")

# pqn_atari_envpool.py:17-73, same names, order and defaults
REFERENCE_FIELDS = [
    ("exp_name", str, "pqn_atari_envpool"), ("seed", int, 1), ("torch_deterministic", bool, True),
    ("cuda", bool, True), ("track", bool, False), ("wandb_project_name", str, "cleanRL"),
    ("wandb_entity", Optional[str], None), ("capture_video", bool, False),
    ("env_id", str, "Breakout-v5"), ("total_timesteps", int, 10_000_000),
    ("learning_rate", float, 2.5e-4), ("num_envs", int, 8), ("num_steps", int, 128),
    ("anneal_lr", bool, True), ("gamma", float, 0.99), ("num_minibatches", int, 4),
    ("update_epochs", int, 4), ("max_grad_norm", float, 10.0), ("start_e", float, 1.0),
    ("end_e", float, 0.01), ("exploration_fraction", float, 0.10), ("q_lambda", float, 0.65),
    ("batch_size", int, 0), ("minibatch_size", int, 0), ("num_iterations", int, 0),
]
# [oc_cleanrl_amd] additions: what PPOTrainer reads beyond the script's flags (args.Args' own
# defaults unless listed), the network choice and the observation geometry
OWN_DEFAULTS = {"architecture": "PQN_OBJ", "obs_mode": "obj", "backend": "Synthetic",
                "vecnorm_reward": False,  # the script clips rewards and has no VecNormalize
                "encoder_dims": (128, 64), "decoder_dims": (128,)}
# fields of args.Args with no meaning here: PPO's loss, the PPObj-only rollout / update features
# (a LayerNorm sits inside every layer those kernels fuse), the sampler's noise, DP
SKIP = CORE_SKIP | {"gae_lambda", "norm_adv", "clip_coef", "clip_vloss", "ent_coef", "vf_coef",
                    "target_kl", "sampling_noise", "fused_heads_loss", "sample_records_min",
                    "conv_channels_last"}
FIXED = CORE_FIXED + (
    ("norm_adv", False), ("target_kl", None),
    ("sampling_noise", "torch"),  # no Exp(1) stream: acting draws from ocppo_epsilon_greedy's
    ("fused_heads_loss", False), ("sample_records_min", -1), ("conv_channels_last", False))

PQNArgs = learner_args(
    "PQNArgs", "The flags of pqn_atari_envpool.py:17-73 (same names, order and defaults) + "
               "this build's additions.",
    REFERENCE_FIELDS, SKIP, OWN_DEFAULTS, fixed=FIXED)


def finalize(args, world_size: int = 1):
    """Derived sizes (pqn_atari_envpool.py:148-150) and the checks of args.finalize that apply."""
    if args.architecture not in ARCHITECTURES:
        raise NotImplementedError(f"architecture must be one of {ARCHITECTURES}")
    if (args.obs_mode == "obj") != (args.architecture == "PQN_OBJ"):
        raise ValueError('architecture PQN_OBJ reads --obs_mode obj, PQN reads pixels (dqn)')
    single_gpu_sizes(args, world_size, "the PQN learner")
    if args.minibatch_size < 1 or args.batch_size % args.num_minibatches:
        raise ValueError(f"batch size {args.batch_size} must be divisible by num_minibatches="
                         f"{args.num_minibatches}")
    if not args.exploration_fraction * args.total_timesteps > 0:
        raise ValueError("exploration_fraction * total_timesteps (the schedule's duration) must "
                         "be positive")
    return args


def linear_schedule(start_e: float, end_e: float, duration: float, t: int) -> float:
    """pqn_atari_envpool.py:141-143."""
    slope = (end_e - start_e) / duration
    return max(slope * t + start_e, end_e)


def _fusable_linear(x, lin) -> bool:
    return (FUSED_PQN and isinstance(lin, nn.Linear) and lin.bias is not None and x.is_cuda and
            x.dtype == torch.float32)


def _fusable_norm(x, ln) -> bool:
    """LayerNorm(width) [-> ReLU] on GPU f32 rows that ops.ln_relu takes: the rollout's rows
    (no autograd), and the update's with FUSED_LN_UPDATE."""
    return (FUSED_PQN and isinstance(ln, nn.LayerNorm) and ln.elementwise_affine and
            ln.bias is not None and tuple(ln.normalized_shape) == (x.shape[-1],) and
            x.shape[-1] <= ops.LN_RELU_MAX_E and x.is_cuda and x.dtype == torch.float32 and
            (FUSED_LN_UPDATE or not torch.is_grad_enabled()))


def trunk_layers(envs, pixels: bool, encoder_dims=(128, 64), decoder_dims=(128,)):
    """(modules, output width) of the network below the Q head, made in the script's order
    (:119-134): the pixel stack, or the PPObj encoder / decoder (agents.object_trunk) with a
    LayerNorm(width) between every Linear and its ReLU. Shared with the recurrent PQN network."""
    dims = tuple(envs.observation_space.shape)
    if pixels:
        convs = [(32, 8, 4), (64, 4, 2), (64, 3, 1)]
        layers, c, hw = [], dims[0], dims[1]
        for cout, k, s in convs:
            hw = (hw - k) // s + 1
            layers += [layer_init(nn.Conv2d(c, cout, k, stride=s)),
                       nn.LayerNorm([cout, hw, hw]), nn.ReLU()]
            c = cout
        layers += [nn.Flatten(), layer_init(nn.Linear(c * hw * hw, 512)), nn.LayerNorm(512),
                   nn.ReLU()]
        return layers, 512
    plain, d = object_trunk(dims, tuple(encoder_dims), tuple(decoder_dims), layer_init)
    layers = []
    for m in plain:  # LayerNorm draws nothing: the seeded init is object_trunk's
        layers.append(m)
        if isinstance(m, nn.Linear):
            layers.append(nn.LayerNorm(m.out_features))
    return layers, d


def run_trunk(mods, x):
    """The modules below the Q head on x: a fusable Linear is agents.linear_act, a fusable
    LayerNorm [-> ReLU] one ops.ln_relu launch, anything else the module itself."""
    i = 0
    while i < len(mods):
        m = mods[i]
        if _fusable_linear(x, m):
            x = linear_act(x, m, False)
        elif _fusable_norm(x, m):
            relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            x = ops.timed("ln_relu", lambda h=x, ln=m, relu=relu: ops.ln_relu(
                h, ln.weight, ln.bias, ln.eps, relu))
            i += 1 if relu else 0
        else:
            x = m(x)
        i += 1
    return x


def q_head(lin, hidden):
    """Q values [rows, A] of the head `lin` on its input rows."""
    if FUSED_PQN and hidden.is_cuda and hidden.dtype == torch.float32:
        return linear_act(hidden, lin, False)
    return lin(hidden)


class PQNetwork(Predictor):
    """QNetwork of pqn_atari_envpool.py:117-138. architecture "PQN": the script's pixel network
    with its state-dict keys (network.0 .. network.13) and seeded init; "PQN_OBJ": the PPObj
    encoder / decoder stack (agents.object_trunk) with a LayerNorm(width) between every Linear and
    its ReLU, then Linear(d, A) with the script's layer_init. The Q head is network[-1]."""

    # PPOTrainer looks for a policy / value head pair: there is none (no fused policy head, no
    # frame cache, autograd's accumulation into the flat gradient buffer)
    actor = critic = None
    grads_in_place = False

    def __init__(self, envs, architecture: str = "PQN_OBJ", device=None, encoder_dims=(128, 64),
                 decoder_dims=(128,)):
        super().__init__()
        if architecture not in ARCHITECTURES:
            raise NotImplementedError(architecture)
        self.device = device
        self.pixels = architecture == "PQN"
        layers, d = trunk_layers(envs, self.pixels, encoder_dims, decoder_dims)
        layers.append(layer_init(nn.Linear(d, envs.action_space.n)))
        self.network = nn.Sequential(*layers)

    @property
    def q_lin(self) -> nn.Linear:
        return self.network[-1]

    def trunk(self, x, prescaled: bool = False):
        """The Q head's input [rows, d] (pixels are divided by 255 here, :138)."""
        if self.pixels and not prescaled:
            x = x / 255.0
        return run_trunk(list(self.network)[:-1], x)

    def q_head(self, hidden):
        """Q values [rows, A] of the trunk output."""
        return q_head(self.q_lin, hidden)

    def forward(self, x):
        return self.q_head(self.trunk(x))

    def predict(self, x, states=None, **_):
        with torch.no_grad():
            dev = next(self.parameters()).device
            q = self(torch.as_tensor(np.asarray(x), dtype=torch.float32, device=dev))
            return np.argmax(q.cpu().numpy(), axis=1), states


class PQNTrainer(PPOTrainer):
    """PPOTrainer's rollout buffer, staging, flat buffers and graphs with PQN's three changes:
    epsilon-greedy acting on the Q head, Q(lambda) returns at the rollout's end, and the MSE loss
    on the taken action under RAdam."""

    def __init__(self, args, device, *a, **k):
        # the torch path's optimizer is torch.optim.RAdam (PPOTrainer's fused_optimizer switch)
        args.fused_optimizer = bool(args.fused_optimizer and FUSED_PQN)
        self.fused = FUSED_PQN
        super().__init__(args, device, *a, **k)
        f32, dev = torch.float32, self.dev
        self.next_q = torch.zeros((self.N, self.A), dtype=f32, device=dev)
        self.dq = torch.zeros((self.M, self.A), dtype=f32, device=dev)
        self.qstats = torch.zeros((self.E * self.nmb, 2), dtype=f32, device=dev)
        # global_step before this rollout (:218); step t's schedule / draw index is this + (t+1) N
        self.eps_step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.epsilon = torch.zeros(1, dtype=f32, device=dev)
        self.eps_duration = float(args.exploration_fraction * args.total_timesteps)

    def _make_agent(self) -> nn.Module:
        a = self.args
        return PQNetwork(EnvSpec(self.obs_shape, self.A), a.architecture, None, a.encoder_dims,
                         a.decoder_dims)

    def _make_optimizer(self):
        a = self.args
        return ops.FlatRAdam(self.agent.parameters(), lr=a.learning_rate,
                             max_grad_norm=a.max_grad_norm)

    def _make_torch_optimizer(self):
        return torch.optim.RAdam(self.params, lr=self.lr, foreach=True, capturable=True)

    # ---- rollout ---------------------------------------------------------------------------
    def _act(self, t: int, env_step: bool = False, hidden=None) -> bool:
        """Step t (:222-232): Q values of the current observation, values[t] = the greedy one,
        actions[t] = the epsilon-greedy choice at global step eps_step + (t + 1) N."""
        a, ag = self.args, self.agent
        if hidden is None:
            hidden = self._policy_hidden(t)
        lin = ag.q_lin
        off = (t + 1) * self.N
        sched = (self.seed, self.eps_step, a.start_e, a.end_e, self.eps_duration)
        if self.fused and ops.pqn_act_ok(hidden, lin.weight):
            self.timer.bracket("pqn_act", lambda: ops.pqn_act(
                hidden, lin.weight, lin.bias, *sched, self.actions[t], self.values[t],
                self.epsilon, step_offset=off))
            return False
        q = ag.q_head(hidden).float().contiguous()
        self.values[t].copy_(q.gather(1, torch.argmax(q, dim=1, keepdim=True)).view(-1))
        ops.epsilon_greedy(q, *sched, self.actions[t], self.epsilon, step_offset=off)
        return False

    def _rollout_end(self):
        """q_network(next_obs) and the Q(lambda) targets (:248-261), then the minibatches' rows."""
        a, T = self.args, self.T
        q = self.agent.q_head(self._policy_hidden(T))
        self.next_q.copy_(q)
        self.timer.bracket("q_lambda", lambda: ops.q_lambda(
            self.rewards, self.values[:T], self.dones[:T], self.next_q, self.dones[T], a.gamma,
            a.q_lambda, self.returns))
        self._prepare_minibatches()

    # ---- update ----------------------------------------------------------------------------
    def _forward_backward_body(self, j: int):
        """Minibatch j (:276-281): trunk -> Q head -> MSE on the taken action -> backward."""
        ag, mb = self.agent, self.mb
        q = ag.q_head(self._minibatch_hidden(j))
        sl = slice(j * self.M, (j + 1) * self.M)
        self.grad_buf.zero_()  # optimizer.zero_grad(): autograd accumulates into the flat buffer
        if self.fused:
            qd = q.detach()
            self.timer.bracket("pqn_loss", lambda: ops.pqn_loss_fwd_bwd(
                qd, mb["actions"][sl], mb["returns"][sl], self.dq, self.qstats[j]))
            torch.autograd.backward(q, self.dq)
            return
        # q.gather(1, a)'s value as a masked row sum: its backward is a multiply, where gather's
        # is a scatter_add that torch_deterministic refuses on the GPU
        old_val = (q * F.one_hot(mb["actions"][sl], self.A).to(q.dtype)).sum(1)
        loss = F.mse_loss(mb["returns"][sl], old_val)
        self.qstats[j, 0].copy_(loss.detach())
        self.qstats[j, 1].copy_(old_val.detach().mean())
        loss.backward()

    # ---- iteration / metrics ---------------------------------------------------------------
    def train_iteration(self, collect_metrics: bool = True, lag: bool = False) -> dict:
        self.eps_step.fill_(self.iteration * self.T * self.N)
        return super().train_iteration(collect_metrics, lag=False)

    def _lag_ok(self) -> bool:
        return False

    def _metrics(self) -> dict:
        """The script's scalars (:285-286) of the last minibatch + epsilon; one host sync."""
        st = self.qstats[:self.executed_mb].cpu().numpy()
        ep_ret, ep_len, ep_n = self.env.pop_episode_stats()
        m = {"charts/learning_rate": float(self.lr), "charts/epsilon": float(self.epsilon),
             "losses/td_loss": float(st[-1, 0]), "losses/q_values": float(st[-1, 1])}
        if ep_n > 0:
            m["charts/episodic_return"] = ep_ret / ep_n
            m["charts/episodic_length"] = ep_len / ep_n
        self.last_metrics = m
        return m


def run_pqn(args, device=None) -> PQNTrainer:
    return run(args, device, trainer_cls=PQNTrainer)


def main(argv=None):
    return learner_main(PQNArgs, finalize, run_pqn,
                        "oc_cleanrl_amd PQN (pqn_atari_envpool.py surface)", argv)


if __name__ == "__main__":
    main()
