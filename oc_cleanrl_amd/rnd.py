"""`python -m oc_cleanrl_amd.rnd [ppo_rnd_envpool.py flags]` — Random Network Distillation
(cleanrl/ppo_rnd_envpool.py) on the device rollout of `trainer.PPOTrainer`.

RND is PPO's loop with a curiosity reward: a frozen random `target` network and a trained
`predictor` both read the newest frame of the observation that follows each env step, and half
their squared distance is the step's intrinsic reward (:365-373). The agent carries two value
heads; the rollout's end filters and normalises the intrinsic rewards (:390-400), runs one GAE
scan per reward stream (:406-430) and mixes the two advantages (:442); the update adds the
intrinsic value loss and the predictor's masked forward loss to PPO's (:463-512). Restated here on
the trainer's HBM rollout buffer, staging, flat buffers, ops.FlatAdam and hipGraphs:
  * `_act` runs actor / extra_layer / both critics on the trunk output (agents.linear_act) and
    ops.categorical_sample; after every `_store(t)` the curiosity step is ops.rnd_normalize on
    the newest frame of obs[t + 1] -> target, predictor -> ops.rnd_curiosity into curiosity[t];
  * the rollout's end is ops.rnd_reward_norm, ops.rnd_gae, the minibatch gather, ops.rms_update
    on the batch's newest frames and ops.rnd_normalize of the whole batch;
  * a minibatch is trunk -> heads, predictor / target on the normalised rows ->
    ops.ppo_loss_fwd_bwd (policy + extrinsic value, on the combined advantage) +
    ops.rnd_aux_loss_fwd_bwd (intrinsic value + masked forward loss) -> one backward, then one
    ops.FlatAdam step over the agent's and the predictor's parameters with one clip.
Both running statistics (gym's RunningMeanStd) live on the device in f64; nothing in an iteration
reads a scalar back to the host except the metrics copy.
`FUSED_RND = False` selects plain torch ops for the six RND kernels (the mask still comes from
ops.rnd_mask, the package's stream, so both paths train alike from one seed).

Declared differences from the script: no envpool / ALE here (--backend Synthetic, the package's
device envs); `architecture` picks the networks ("RND_OBJ", the default: agents.object_trunk on
object vectors, the RND body two Linear + LeakyReLU layers on one frame's object vector; "RND":
the script's pixel networks -- modules, keys and init only, its trainer path is out of scope: the
LeakyReLU convolutions have no kernel here); the observation statistics are per feature of the
newest frame's object vector; the update mask is the library's counter stream keyed by (seed,
minibatch counter, row), not torch.rand; the warm-up's random actions are torch.randint from a
device generator seeded with the run's seed, not np.random.randint, and the first rollout goes on
from the observation the warm-up ended on; the filtered rewards' mean and variance are taken in
f64 (numpy's are f32); one GPU.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import agents, ops
from .agents import EnvSpec, _ActorCritic, layer_init, linear_act, object_trunk
from .args import (CORE_FIXED, CORE_SKIP, check_sampling_noise, learner_args,
                   parse_dataclass, single_gpu_sizes)  # noqa: F401  (parse_dataclass: re-exported)
from .trainer import PPOTrainer, _own_tensors, learner_main, run

# The six RND kernels (ops.rms_update, rnd_normalize, rnd_curiosity, rnd_reward_norm, rnd_gae,
# rnd_aux_loss_fwd_bwd); False: plain torch ops in their place
FUSED_RND = True

ARCHITECTURES = ("RND_OBJ", "RND")

# ppo_rnd_envpool.py:22-94, same names, order and defaults
_REFERENCE_FIELDS = [
    ("exp_name", str, "ppo_rnd_envpool"), ("seed", int, 1), ("torch_deterministic", bool, True),
    ("cuda", bool, True), ("track", bool, False), ("wandb_project_name", str, "cleanRL"),
    ("wandb_entity", Optional[str], None), ("capture_video", bool, False),
    ("env_id", str, "MontezumaRevenge-v5"), ("total_timesteps", int, 2_000_000_000),
    ("learning_rate", float, 1e-4), ("num_envs", int, 128), ("num_steps", int, 128),
    ("anneal_lr", bool, True), ("gamma", float, 0.999), ("gae_lambda", float, 0.95),
    ("num_minibatches", int, 4), ("update_epochs", int, 4), ("norm_adv", bool, True),
    ("clip_coef", float, 0.1), ("clip_vloss", bool, True), ("ent_coef", float, 0.001),
    ("vf_coef", float, 0.5), ("max_grad_norm", float, 0.5), ("target_kl", Optional[float], None),
    ("update_proportion", float, 0.25), ("int_coef", float, 1.0), ("ext_coef", float, 2.0),
    ("int_gamma", float, 0.99), ("num_iterations_obs_norm_init", int, 50),
    ("batch_size", int, 0), ("minibatch_size", int, 0), ("num_iterations", int, 0),
]
# [oc_cleanrl_amd] additions: what PPOTrainer reads beyond the script's flags (args.Args' own
# defaults unless listed), the network choice and the RND body's geometry
_OWN_FIELDS = [("rnd_dims", tuple, (128, 128)), ("rnd_feature_dim", int, 512)]
_OWN_DEFAULTS = {"architecture": "RND_OBJ", "obs_mode": "obj", "backend": "Synthetic",
                 "vecnorm_reward": False,  # the script has no VecNormalize
                 "encoder_dims": (128, 64), "decoder_dims": (128,)}
# fields of args.Args with no meaning here: the PPObj-only rollout / update features (the
# curiosity step needs the stored next observation between two steps; the heads are not one
# Linear each), DP, and the optimizer switch (the flat buffers hold two modules' parameters)
_SKIP = CORE_SKIP | {"fused_heads_loss", "sample_records_min", "conv_channels_last",
                     "fused_optimizer"}
_FIXED = CORE_FIXED + (("fused_heads_loss", False), ("sample_records_min", -1),
                       ("conv_channels_last", False), ("fused_optimizer", True))

RNDArgs = learner_args(
    "RNDArgs", "The flags of ppo_rnd_envpool.py:22-94 (same names, order and defaults) + "
               "this build's additions.",
    _REFERENCE_FIELDS, _SKIP, _OWN_DEFAULTS, _OWN_FIELDS, _FIXED)


def finalize(args, world_size: int = 1, trainer: bool = True):
    """Derived sizes (ppo_rnd_envpool.py:247-249) and the checks of args.finalize that apply.
    trainer: the arguments are for RNDTrainer, which trains RND_OBJ only (False: for building
    the modules)."""
    if args.architecture not in ARCHITECTURES:
        raise NotImplementedError(f"architecture must be one of {ARCHITECTURES}")
    if (args.obs_mode == "obj") != (args.architecture == "RND_OBJ"):
        raise ValueError('architecture RND_OBJ reads --obs_mode obj, RND reads pixels (dqn)')
    if trainer and args.architecture != "RND_OBJ":
        raise NotImplementedError("RNDTrainer trains RND_OBJ; the pixel RND networks' LeakyReLU "
                                  "convolutions have no kernel here (DESIGN 8)")
    if not 0.0 <= args.update_proportion <= 1.0:
        raise ValueError(f"update_proportion {args.update_proportion} outside [0, 1]")
    if args.num_iterations_obs_norm_init < 0:
        raise ValueError("num_iterations_obs_norm_init must be >= 0")
    check_sampling_noise(args)
    single_gpu_sizes(args, world_size, "the RND learner")
    if args.minibatch_size < 1 or args.batch_size % args.num_minibatches:
        raise ValueError(f"batch size {args.batch_size} must be divisible by num_minibatches="
                         f"{args.num_minibatches}")
    return args


def _seq(seq, x):
    """`seq(x)` with every biased Linear (+ a following ReLU) through agents.linear_act on GPU f32
    rows; any other module (LeakyReLU, convolutions, Flatten) is torch's."""
    mods = list(seq) if isinstance(seq, nn.Sequential) else [seq]
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.Linear) and m.bias is not None and x.is_cuda and \
                x.dtype == torch.float32 and x.dim() == 2:
            relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            x = linear_act(x, m, relu)
            i += 2 if relu else 1
        else:
            x = m(x)
            i += 1
    return x


class RNDAgent(_ActorCritic):
    """Agent of ppo_rnd_envpool.py:138-181 with its state-dict keys (network.*, extra_layer.0,
    actor.0, actor.2, critic_ext, critic_int) and seeded init. architecture "RND": the script's
    pixel trunk (d = 448); "RND_OBJ": agents.object_trunk on object vectors (d = the decoder's
    width)."""

    critic = None  # PPOTrainer looks for a one-Linear policy / value head pair: there is none
    grads_in_place = False

    def __init__(self, envs, architecture: str = "RND_OBJ", device=None, encoder_dims=(128, 64),
                 decoder_dims=(128,)):
        super().__init__()
        if architecture not in ARCHITECTURES:
            raise NotImplementedError(architecture)
        self.device = device
        self.pixels = architecture == "RND"
        dims = tuple(envs.observation_space.shape)
        A = envs.action_space.n
        if self.pixels:
            layers = [layer_init(nn.Conv2d(dims[0], 32, 8, stride=4)), nn.ReLU(),
                      layer_init(nn.Conv2d(32, 64, 4, stride=2)), nn.ReLU(),
                      layer_init(nn.Conv2d(64, 64, 3, stride=1)), nn.ReLU(), nn.Flatten()]
            with torch.no_grad():
                feat = nn.Sequential(*layers)(torch.zeros((1,) + dims)).shape[1]
            layers += [layer_init(nn.Linear(feat, 256)), nn.ReLU(),
                       layer_init(nn.Linear(256, 448)), nn.ReLU()]
            d = 448
        else:
            layers, d = object_trunk(dims, tuple(encoder_dims), tuple(decoder_dims), layer_init)
        self.network = nn.Sequential(*layers)
        self.extra_layer = nn.Sequential(layer_init(nn.Linear(d, d), std=0.1), nn.ReLU())
        self.actor = nn.Sequential(layer_init(nn.Linear(d, d), std=0.01), nn.ReLU(),
                                   layer_init(nn.Linear(d, A), std=0.01))
        self.critic_ext = layer_init(nn.Linear(d, 1), std=0.01)
        self.critic_int = layer_init(nn.Linear(d, 1), std=0.01)

    def trunk(self, x, prescaled: bool = False):
        if self.pixels and not prescaled:
            x = x / 255.0
        return super().trunk(x, prescaled)

    def heads3(self, hidden):
        """(logits [rows, A], ext value [rows, 1], int value [rows, 1]) of the trunk output."""
        # the trunk's last layer leaves its ReLU backward to a single consumer (its box): there
        # are three here, so they read a view that carries no box
        h = hidden.view(hidden.shape)
        logits = _seq(self.actor, h)
        s = _seq(self.extra_layer, h) + h
        return logits, _seq(self.critic_ext, s), _seq(self.critic_int, s)

    def get_value(self, x, prescaled: bool = False):
        _, ve, vi = self.heads3(self.trunk(x, prescaled))
        return ve, vi

    def get_action_and_value(self, x, action=None):
        """(action, log_prob, entropy, ext value, int value) like the script (:163-176)."""
        logits, ve, vi = self.heads3(self.trunk(x))
        probs = torch.distributions.Categorical(logits=logits)
        if action is None:
            action = probs.sample()
        return action, probs.log_prob(action), probs.entropy(), ve, vi

    def predict(self, x, states=None, **_):
        with torch.no_grad():
            dev = next(self.parameters()).device
            x = torch.as_tensor(np.asarray(x), dtype=torch.float32, device=dev)
            logits = self.heads3(self.trunk(x))[0]
            return np.argmax(logits.cpu().numpy(), axis=1), states


class RNDModel(nn.Module):
    """RNDModel of ppo_rnd_envpool.py:184-229: a trainable `predictor` and a frozen `target` on
    the normalised newest frame, keys predictor.* / target.*. architecture "RND": the script's
    modules on [rows, 1, 84, 84]; "RND_OBJ": the three convolutions replaced by
    Linear(F, rnd_dims[0]), LeakyReLU, Linear(rnd_dims[0], rnd_dims[1]), LeakyReLU on [rows, F].
    The heads are the script's, into rnd_feature_dim."""

    def __init__(self, architecture: str = "RND_OBJ", frame_features: int = 12,
                 rnd_dims=(128, 128), rnd_feature_dim: int = 512):
        super().__init__()
        if architecture not in ARCHITECTURES:
            raise NotImplementedError(architecture)
        D = int(rnd_feature_dim)

        def body():
            if architecture == "RND":
                return [layer_init(nn.Conv2d(1, 32, 8, stride=4)), nn.LeakyReLU(),
                        layer_init(nn.Conv2d(32, 64, 4, stride=2)), nn.LeakyReLU(),
                        layer_init(nn.Conv2d(64, 64, 3, stride=1)), nn.LeakyReLU(),
                        nn.Flatten()], 7 * 7 * 64
            h1, h2 = (int(v) for v in rnd_dims)
            return [layer_init(nn.Linear(frame_features, h1)), nn.LeakyReLU(),
                    layer_init(nn.Linear(h1, h2)), nn.LeakyReLU()], h2

        layers, w = body()
        self.predictor = nn.Sequential(*layers, layer_init(nn.Linear(w, D)), nn.ReLU(),
                                       layer_init(nn.Linear(D, D)), nn.ReLU(),
                                       layer_init(nn.Linear(D, D)))
        layers, w = body()
        self.target = nn.Sequential(*layers, layer_init(nn.Linear(w, D)))
        for p in self.target.parameters():  # the target network is not trainable (:221-223)
            p.requires_grad = False

    def predict_features(self, x):
        return _seq(self.predictor, x)

    def target_features(self, x):
        with torch.no_grad():
            return _seq(self.target, x)

    def forward(self, x):
        return self.predict_features(x), self.target_features(x)


def combined_parameters(agent, rnd_model):
    """The optimizer's parameters in the script's order (:295)."""
    return list(agent.parameters()) + list(rnd_model.predictor.parameters())


def _merge(state, mean_sl, var_sl, cnt_sl, bm, bv, bc: float):
    """RunningMeanStd.update_from_moments on a device f64 state (torch ops, the law's order)."""
    mean, var, count = state[mean_sl], state[var_sl], state[cnt_sl]
    delta = bm - mean
    tot = count + bc
    new_mean = mean + delta * bc / tot
    m2 = var * count + bv * bc + delta * delta * count * bc / tot
    state[var_sl] = m2 / tot
    state[mean_sl] = new_mean
    state[cnt_sl] = tot


class RNDTrainer(PPOTrainer):
    """PPOTrainer's rollout buffer, staging, flat buffers, FlatAdam and graphs with RND's
    additions: two value heads, the curiosity step after every store, the reward filter and the
    two GAE scans at the rollout's end, the running observation statistics, and the intrinsic
    value + masked forward loss beside PPO's."""

    def __init__(self, args, device, *a, **k):
        if args.architecture != "RND_OBJ":
            raise NotImplementedError("RNDTrainer trains RND_OBJ only (DESIGN 8)")
        self.fused = FUSED_RND
        super().__init__(args, device, *a, **k)
        if self.world != 1 or self.dp:
            raise NotImplementedError("the RND learner runs on one GPU")
        f32, dev = torch.float32, self.dev
        T, N, B, M = self.T, self.N, self.B, self.M
        self.F = self.obs_shape[-1]
        D = args.rnd_feature_dim
        self.ext_values = self.values  # [T + 1, N]: PPOTrainer's value rows are the extrinsic ones
        self.int_values = torch.zeros((T + 1, N), dtype=f32, device=dev)
        self.curiosity = torch.zeros((T, N), dtype=f32, device=dev)
        self.ext_advantages = torch.zeros((T, N), dtype=f32, device=dev)
        self.int_advantages = torch.zeros((T, N), dtype=f32, device=dev)
        self.ext_returns = self.returns  # what minibatch_prepare gathers beside the ext values
        self.int_returns = torch.zeros((T, N), dtype=f32, device=dev)
        self.rnd_in = torch.zeros((N, self.F), dtype=f32, device=dev)
        self.rnd_obs = torch.zeros((B, self.F), dtype=f32, device=dev)
        self.obs_rms = ops.rms_state(self.F, dev)
        self.reward_rms = torch.tensor([0.0, 1.0, 1e-4], dtype=torch.float64, device=dev)
        self.rewems = torch.zeros(T, dtype=f32, device=dev)
        nmbt = self.E * self.nmb
        self.mb_int_returns = torch.zeros(nmbt * M, dtype=f32, device=dev)
        self.mask_counter = ops.rnd_mask_counter(dev)
        self.dpred = torch.zeros((M, D), dtype=f32, device=dev)
        self.dv_int = torch.zeros(M, dtype=f32, device=dev)
        self.rstats = torch.zeros((nmbt, len(ops.RND_STAT_NAMES)), dtype=f32, device=dev)
        self._warm_up()

    def _make_agent(self) -> nn.Module:
        a = self.args
        agent = RNDAgent(EnvSpec(self.obs_shape, self.A), a.architecture, None, a.encoder_dims,
                         a.decoder_dims)
        # the script builds the agent, then the RND model, from one seeded generator (:293-294)
        self.rnd = RNDModel(a.architecture, self.obs_shape[-1], a.rnd_dims, a.rnd_feature_dim)
        return agent

    def _make_optimizer(self):
        a = self.args
        self.rnd.to(self.dev)
        agents.set_update_gemm(self.rnd, a.x6_gemm)
        return ops.FlatAdam(combined_parameters(self.agent, self.rnd), lr=a.learning_rate,
                            eps=1e-5, max_grad_norm=a.max_grad_norm)

    # ---- running statistics / normalisation (kernel or torch) ----------------------------------
    def _newest(self, stacks):
        """The newest frame [rows, F] (strided rows) of observation stacks [..., W, F]."""
        return stacks.reshape((-1,) + self.obs_shape)[:, -1]

    def _rms_update(self, x):
        if self.fused:
            self.timer.bracket("rms_update", lambda: ops.rms_update(x, self.obs_rms))
            return
        C = self.F
        x64 = x.double()
        _merge(self.obs_rms, slice(0, C), slice(C, 2 * C), slice(2 * C, 2 * C + 1), x64.mean(0),
               x64.var(0, unbiased=False), float(x.shape[0]))

    def _normalize(self, x, out):
        if self.fused:
            self.timer.bracket(f"rnd_normalize_{x.shape[0]}",
                               lambda: ops.rnd_normalize(x, self.obs_rms, out))
            return
        C = self.F
        out.copy_(((x.double() - self.obs_rms[:C]) / torch.sqrt(self.obs_rms[C:2 * C]))
                  .clip(-5, 5).float())

    def _warm_up(self):
        """ppo_rnd_envpool.py:324-335: num_iterations_obs_norm_init rounds of num_steps
        random-action env steps, each round's newest frames merged into obs_rms. The actions are
        torch.randint draws of a device generator seeded with the run's seed."""
        a, T = self.args, self.T
        gen = torch.Generator(device=self.dev)
        gen.manual_seed(self.seed)
        with torch.no_grad():
            for _ in range(a.num_iterations_obs_norm_init):
                self.obs[0].copy_(self.obs[T])
                self.dones[0].copy_(self.dones[T])
                self.actions.copy_(torch.randint(0, self.A, (T, self.N), generator=gen,
                                                 device=self.dev))
                for t in range(T):
                    self.env.step(self.actions[t], t)
                    self._store(t)
                self.env.advance(T)
                self._rms_update(self._newest(self.obs[1:T + 1]))
        self.env.pop_episode_stats()  # the warm-up's episodes are not the run's

    # ---- rollout ---------------------------------------------------------------------------
    def _act(self, t: int, env_step: bool = False, hidden=None) -> bool:
        """Step t (:351-359): both values and a Categorical draw from the actor's logits."""
        if self.args.sampling_noise == "torch":
            self.noise[t].exponential_()
        px = self.exp_stream.philox(t) if self.args.sampling_noise == "head" else None
        if hidden is None:
            hidden = self._policy_hidden(t)
        logits, ve, vi = self.agent.heads3(hidden)
        self.int_values[t].copy_(vi.view(-1))
        self.timer.bracket("action_head", lambda: ops.categorical_sample(
            logits.float().contiguous(), self.noise[t], self.actions[t], self.logprobs[t], None,
            ve.reshape(-1), self.ext_values[t], philox=px))
        return False

    def _curiosity_step(self, t: int):
        """curiosity[t] from the newest frame of the observation after step t (:365-373)."""
        self._normalize(self._newest(self.obs[t + 1]), self.rnd_in)
        pf = self.rnd.predict_features(self.rnd_in)
        tf = self.rnd.target_features(self.rnd_in)
        if self.fused:
            self.timer.bracket("rnd_curiosity", lambda: ops.rnd_curiosity(
                pf, tf, self.curiosity[t]))
        else:
            self.curiosity[t].copy_((tf - pf).pow(2).sum(1) / 2)

    def _rollout_step(self, t: int):
        super()._rollout_step(t)
        self._curiosity_step(t)

    def _reward_norm_torch(self):
        """:390-400 in torch ops (the filter walks the env axis; f64 moments)."""
        a, N = self.args, self.N
        g = float(np.float32(a.int_gamma))
        rew, cols = self.rewems, []
        for n in range(N):
            rew = rew * g + self.curiosity[:, n]
            cols.append(rew)
        self.rewems.copy_(rew)
        per_env = torch.stack(cols).double()  # [N, T]
        _merge(self.reward_rms, slice(0, 1), slice(1, 2), slice(2, 3), per_env.mean(),
               per_env.var(unbiased=False), float(N))
        self.curiosity.div_(torch.sqrt(self.reward_rms[1]).float())

    def _gae_torch(self):
        """:406-430, :442: the script's loop."""
        a, T = self.args, self.T
        ext_last = int_last = 0
        for t in reversed(range(T)):
            ext_nnt = 1.0 - self.dones[t + 1]
            ext_delta = self.rewards[t] + a.gamma * self.ext_values[t + 1] * ext_nnt - \
                self.ext_values[t]
            int_delta = self.curiosity[t] + a.int_gamma * self.int_values[t + 1] * 1.0 - \
                self.int_values[t]
            self.ext_advantages[t] = ext_last = ext_delta + a.gamma * a.gae_lambda * ext_nnt * ext_last
            self.int_advantages[t] = int_last = int_delta + a.int_gamma * a.gae_lambda * 1.0 * int_last
        torch.add(self.ext_advantages, self.ext_values[:T], out=self.ext_returns)
        torch.add(self.int_advantages, self.int_values[:T], out=self.int_returns)
        torch.add(self.int_advantages * a.int_coef, self.ext_advantages * a.ext_coef,
                  out=self.advantages)

    def _rollout_end(self):
        """Reward filter + normalisation (:390-400), bootstrap + both GAE scans (:403-430), the
        combined advantage (:442), the minibatches' rows, obs_rms.update and the batch's
        normalised newest frames (:444-454)."""
        a, T = self.args, self.T
        if self.fused:
            self.timer.bracket("rnd_reward_norm", lambda: ops.rnd_reward_norm(
                self.curiosity, self.rewems, self.reward_rms, a.int_gamma))
        else:
            self._reward_norm_torch()
        _, ve, vi = self.agent.heads3(self._policy_hidden(T))
        self.ext_values[T].copy_(ve.view(-1))
        self.int_values[T].copy_(vi.view(-1))
        if self.fused:
            self.timer.bracket("rnd_gae", lambda: ops.rnd_gae(
                self.rewards, self.ext_values[:T], self.dones[:T], self.ext_values[T],
                self.dones[T], self.curiosity, self.int_values[:T], self.int_values[T], a.gamma,
                a.int_gamma, a.gae_lambda, a.int_coef, a.ext_coef, self.ext_advantages,
                self.ext_returns, self.int_advantages, self.int_returns, self.advantages))
        else:
            self._gae_torch()
        # the five-array gather: combined advantage, extrinsic value and return; the intrinsic
        # returns beside it
        self._prepare_minibatches()
        torch.index_select(self.int_returns.view(-1), 0, self.perm_dev, out=self.mb_int_returns)
        newest = self._newest(self.obs[:T])
        self._rms_update(newest)
        self._normalize(newest, self.rnd_obs)

    # ---- update ----------------------------------------------------------------------------
    def _forward_backward_body(self, j: int):
        """Minibatch j (:463-515): PPO's loss on the combined advantage and the extrinsic value
        (ops.ppo_loss_fwd_bwd), the intrinsic value loss and the masked forward loss, one
        backward into the flat gradient buffer."""
        a, mb = self.args, self.mb
        sl = slice(j * self.M, (j + 1) * self.M)
        logits, ve, vi = self.agent.heads3(self._minibatch_hidden(j))
        x = self.rnd_obs.index_select(0, self.perm_dev[sl])
        tf = self.rnd.target_features(x)
        pf = self.rnd.predict_features(x)
        lg, vv = logits.detach(), ve.detach().view(-1)
        self.timer.bracket("ppo_loss", lambda: ops.ppo_loss_fwd_bwd(
            lg, vv, mb["actions"][sl], mb["logprobs"][sl], mb["advantages"][sl],
            mb["returns"][sl], mb["values"][sl], mb_inds=None,
            adv_stats=mb["adv_stats"][j] if a.norm_adv else None, clip_coef=a.clip_coef,
            ent_coef=a.ent_coef, vf_coef=a.vf_coef, norm_adv=a.norm_adv,
            clip_vloss=a.clip_vloss, dlogits=self.dlogits, dvalue=self.dvalue,
            stats=self.stats[j], workspace=self.loss_ws))
        self.grad_buf.zero_()  # optimizer.zero_grad(): autograd accumulates into the flat buffer
        ret = self.mb_int_returns[sl]
        if self.fused:
            pd, vd = pf.detach(), vi.detach().view(-1)
            self.timer.bracket("rnd_aux_loss", lambda: ops.rnd_aux_loss_fwd_bwd(
                pd, tf, vd, ret, self.seed, self.mask_counter, a.update_proportion, a.vf_coef,
                self.dpred, self.dv_int, self.rstats[j]))
            torch.autograd.backward(
                [logits, ve, vi, pf],
                [self.dlogits, self.dvalue.view(-1, 1), self.dv_int.view(-1, 1), self.dpred])
            return
        mask = ops.rnd_mask(self.seed, self.mask_counter, self.M, a.update_proportion)
        self.mask_counter.add_(1)
        fwd = F.mse_loss(pf, tf, reduction="none").mean(-1)
        fwd = (fwd * mask).sum() / torch.clamp(mask.sum(), min=1.0)
        int_v = 0.5 * ((vi.view(-1) - ret) ** 2).mean()
        self.rstats[j].copy_(torch.stack([int_v.detach(), fwd.detach(), mask.sum()]))
        torch.autograd.backward([logits, ve, int_v * a.vf_coef + fwd],
                                [self.dlogits, self.dvalue.view(-1, 1), None])

    # ---- iteration / metrics ---------------------------------------------------------------
    def _lag_ok(self) -> bool:
        return False

    def _metrics(self) -> dict:
        """The script's scalars (:528-534): value_loss = ext + int, fwd_loss of the last
        minibatch."""
        m = super()._metrics()
        rs = self.rstats[self.executed_mb - 1].cpu().numpy()
        m["losses/value_loss"] = m["losses/value_loss"] + float(rs[0])
        m["losses/fwd_loss"] = float(rs[1])
        self.last_metrics = m
        return m

    def state_dict_checkpoint(self) -> dict:
        ck = super().state_dict_checkpoint()
        ck["rnd_weights"] = _own_tensors(self.rnd.state_dict())
        ck["obs_rms"], ck["reward_rms"] = self.obs_rms.clone(), self.reward_rms.clone()
        ck["rewems"] = self.rewems.clone()
        return ck

    def load_checkpoint(self, ck: dict):
        """Both modules and the running statistics of a state_dict_checkpoint payload."""
        self.agent.load_state_dict(ck["model_weights"])
        self.rnd.load_state_dict(ck["rnd_weights"])
        self.obs_rms.copy_(ck["obs_rms"])
        self.reward_rms.copy_(ck["reward_rms"])
        self.rewems.copy_(ck["rewems"])


def run_rnd(args, device=None) -> RNDTrainer:
    return run(args, device, trainer_cls=RNDTrainer)


def main(argv=None):
    return learner_main(RNDArgs, finalize, run_rnd,
                        "oc_cleanrl_amd RND (ppo_rnd_envpool.py surface)", argv)


if __name__ == "__main__":
    main()
