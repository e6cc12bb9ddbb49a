"""`python -m oc_cleanrl_amd.contppo [ppo_continuous_action.py flags]` — continuous-action PPO
(cleanrl/ppo_continuous_action.py) and, with --rpo-alpha > 0, RPO (rpo_continuous_action.py, see
oc_cleanrl_amd.rpo) on the device rollout of `trainer.PPOTrainer`.

ppo.py's loop with a diagonal-Gaussian head (two tanh MLPs and a state-independent logstd):
  * cont_actions [T, N, A] f32 is the action buffer; the rollout's standard normal draws z come
    from one torch.randn per rollout on the trainer's generator, before the captured rollout;
  * `_act` is the two MLPs (torch) + ops.gauss_head_sample; the action rows follow the minibatch
    permutation into mb_actions (ops.gather_rows), the scalars go through ops.minibatch_prepare;
  * a minibatch is the two MLPs -> ops.gauss_ppo_loss_fwd_bwd -> their backward -> ops.FlatAdam;
  * the env is envs.PendulumVecEnv (dynamics + the script's wrapper chain, one launch per step).
`FUSED_CONT = False` selects plain torch instead of the two Gaussian kernels: ContAgent's own
get_action_and_value in the update; in the rollout z * std + mean and the row's log-prob summed
in column order, the kernel's order (torch's sum(1) on the GPU adds in a tree order that differs
in the last bit), so that the two paths' rollouts are bitwise equal.

Declared differences: env_id defaults to Pendulum-v1 (HalfCheetah-v4 needs MuJoCo); reset draws
and RPO's uniform noise are the library's own counter streams (ops.rpo_noise returns the
latter); one randn per rollout instead of Normal.sample's draw per step; one GPU.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
from torch.distributions.normal import Normal

from . import ops
from .agents import EnvSpec, Space, layer_init
from .args import CORE_FIXED, CORE_SKIP, learner_args, single_gpu_sizes
from .envs import make_device_env
from .trainer import PPOTrainer, learner_main, run

# The fused kernels (ops.gauss_head_sample, ops.gauss_ppo_loss_fwd_bwd); False: plain torch.
FUSED_CONT = True

# ppo_continuous_action.py:17-83, same names, order and defaults (env_id: see the module docstring)
# + rpo_continuous_action.py:71's rpo_alpha (0 = PPO)
_REFERENCE_FIELDS = [
    ("exp_name", str, "ppo_continuous_action"), ("seed", int, 1),
    ("torch_deterministic", bool, True), ("cuda", bool, True), ("track", bool, False),
    ("wandb_project_name", str, "cleanRL"), ("wandb_entity", Optional[str], None),
    ("capture_video", bool, False), ("save_model", bool, False), ("upload_model", bool, False),
    ("hf_entity", str, ""), ("env_id", str, "Pendulum-v1"), ("total_timesteps", int, 1_000_000),
    ("learning_rate", float, 3e-4), ("num_envs", int, 1), ("num_steps", int, 2048),
    ("anneal_lr", bool, True), ("gamma", float, 0.99), ("gae_lambda", float, 0.95),
    ("num_minibatches", int, 32), ("update_epochs", int, 10), ("norm_adv", bool, True),
    ("clip_coef", float, 0.2), ("clip_vloss", bool, True), ("ent_coef", float, 0.0),
    ("vf_coef", float, 0.5), ("max_grad_norm", float, 0.5), ("target_kl", Optional[float], None),
    ("rpo_alpha", float, 0.0),
    ("batch_size", int, 0), ("minibatch_size", int, 0), ("num_iterations", int, 0),
]
# [oc_cleanrl_amd] additions: what PPOTrainer reads beyond the script's flags (args.Args' own
# defaults unless listed)
_OWN_DEFAULTS = {"architecture": "CONT_MLP", "obs_mode": "obj", "backend": "Synthetic",
                 "buffer_window_size": 1,
                 "vecnorm_reward": False}  # the env's own chain normalises (:99-100)
# fields of args.Args with no meaning here: the Atari / PPObj / pixel features, the Categorical
# sampler's noise, DP
_SKIP = CORE_SKIP | {"sampling_noise", "fused_heads_loss", "sample_records_min",
                     "conv_channels_last", "conv_benchmark", "encoder_dims", "decoder_dims",
                     "x6_gemm", "gemm_table", "num_features", "modifs", "new_rf", "frameskip"}
_FIXED = CORE_FIXED + (
    ("sampling_noise", "torch"),  # no Exp(1) stream: acting draws are the trainer's randn
    ("fused_heads_loss", False), ("sample_records_min", -1), ("conv_channels_last", False),
    ("x6_gemm", False), ("gemm_table", False))  # 64-wide tanh MLPs: torch's GEMMs

ContPPOArgs = learner_args(
    "ContPPOArgs", "The flags of ppo_continuous_action.py:17-83 (same names, order and "
                   "defaults) + rpo_alpha + this build's additions.",
    _REFERENCE_FIELDS, _SKIP, _OWN_DEFAULTS, fixed=_FIXED)


def finalize(args, world_size: int = 1):
    """Derived sizes (ppo_continuous_action.py:146-148) and the checks that apply."""
    if args.rpo_alpha < 0:
        raise ValueError(f"rpo_alpha = {args.rpo_alpha} must not be negative")
    single_gpu_sizes(args, world_size, "the continuous-action PPO learner")
    if args.minibatch_size < 1 or args.batch_size % args.num_minibatches:
        raise ValueError(f"batch size {args.batch_size} must be divisible by num_minibatches="
                         f"{args.num_minibatches}")
    return args


def cont_spec(obs_shape, action_dim: int) -> EnvSpec:
    """An `envs`-like object with a Box-like action space of `action_dim` dimensions."""
    spec = EnvSpec(tuple(obs_shape), None)
    spec.action_space = spec.single_action_space = Space((int(action_dim),))
    return spec


def gauss_logprob_rows(mean, std, action):
    """Normal(mean, std).log_prob(action) per element as torch writes it, then the row sum in
    column order (ops.gauss_head_sample's order)."""
    var = std ** 2
    e = -((action - mean) ** 2) / (2 * var) - std.log() - math.log(math.sqrt(2 * math.pi))
    lp = e[:, 0]
    for a in range(1, e.shape[1]):
        lp = lp + e[:, a]
    return lp


class ContAgent(nn.Module):
    """Agent of ppo_continuous_action.py:112-141 with its state-dict keys (critic.0/2/4,
    actor_mean.0/2/4, actor_logstd) and seeded layer_init order, in plain torch: the unfused path
    and the f32 reference. Observations [B, ...] are flattened per sample. mean_noise (RPO,
    rpo_continuous_action.py:138-141): added to the mean when an action is given."""

    # PPOTrainer looks for a Linear policy / value head pair and a trunk: there is none (no fused
    # heads, no frame cache, autograd's accumulation into the flat gradient buffer)
    actor = network = None
    grads_in_place = False

    def __init__(self, envs):
        super().__init__()
        n = int(np.array(envs.single_observation_space.shape).prod())
        A = int(np.prod(envs.single_action_space.shape))
        self.critic = nn.Sequential(
            layer_init(nn.Linear(n, 64)), nn.Tanh(), layer_init(nn.Linear(64, 64)), nn.Tanh(),
            layer_init(nn.Linear(64, 1), std=1.0))
        self.actor_mean = nn.Sequential(
            layer_init(nn.Linear(n, 64)), nn.Tanh(), layer_init(nn.Linear(64, 64)), nn.Tanh(),
            layer_init(nn.Linear(64, A), std=0.01))
        self.actor_logstd = nn.Parameter(torch.zeros(1, A))

    def get_value(self, x, prescaled: bool = False):
        return self.critic(x.flatten(1))

    def get_action_and_value(self, x, action=None, *, mean_noise=None):
        x = x.flatten(1)
        action_mean = self.actor_mean(x)
        action_logstd = self.actor_logstd.expand_as(action_mean)
        action_std = torch.exp(action_logstd)
        # (validate_args off: the check is a host sync per call, which a captured update refuses)
        probs = Normal(action_mean, action_std, validate_args=False)
        if action is None:
            action = probs.sample()
        elif mean_noise is not None:
            probs = Normal(action_mean + mean_noise, action_std, validate_args=False)
        return action, probs.log_prob(action).sum(1), probs.entropy().sum(1), self.critic(x)

    def predict(self, x, states=None, **_):
        """A sampled action, as cleanrl_utils/evals/ppo_eval.py acts."""
        with torch.no_grad():
            dev = next(self.parameters()).device
            obs = torch.as_tensor(np.asarray(x), dtype=torch.float32, device=dev)
            return self.get_action_and_value(obs)[0].cpu().numpy(), states


class ContPPOTrainer(PPOTrainer):
    """PPOTrainer's rollout buffer, staging, flat buffers and graphs with a float action buffer,
    the Gaussian head's sample in `_act` and the Gaussian loss in the update. device_env: a
    device-resident vector env (the interface of envs.PendulumVecEnv: frame / reward / done /
    ep_state, reset, step(actions [N, A] f32, step_offset), advance, pop_episode_stats, n_actions =
    the action width) in place of the one env_id names."""

    def __init__(self, args, device, rank: int = 0, world_size: int = 1,
                 kernel_timing: bool = False, log: bool = True, envs=None, comm=None,
                 device_env=None):
        if world_size != 1:
            raise NotImplementedError("the continuous-action PPO learner runs on one GPU")
        if envs is not None:
            raise NotImplementedError("the continuous-action PPO learner steps a device env "
                                      "(host envs carry integer actions here)")
        if device_env is not None and device_env.n_actions > ops.GAUSS_MAX_ACTIONS:
            raise ValueError(f"{device_env.n_actions} action dimensions: the Gaussian kernels "
                             f"take at most {ops.GAUSS_MAX_ACTIONS}")
        self._device_env = device_env
        self.fused = FUSED_CONT
        super().__init__(args, device, rank, world_size, kernel_timing, log)
        f32, dev = torch.float32, self.dev
        T, N, A = self.T, self.N, self.A
        self.cont_actions = torch.zeros((T, N, A), dtype=f32, device=dev)
        self.z = torch.zeros((T, N, A), dtype=f32, device=dev)
        self.mb_actions = torch.zeros((self.E * self.nmb * self.M, A), dtype=f32, device=dev)
        self.dmean = torch.zeros((self.M, A), dtype=f32, device=dev)
        self.dlogstd = torch.zeros(A, dtype=f32, device=dev)
        self.rpo_counter = ops.rpo_counter(dev)
        # the rollout's normal draws: a generator of this trainer's own (two trainers in one
        # process do not share or reseed a stream)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(self.seed)
        self.rpo_z = torch.zeros((self.M, A), dtype=f32, device=dev)

    def _make_env(self):
        a = self.args
        if self._device_env is not None:
            return self._device_env
        if a.env_id != "Pendulum-v1":
            raise NotImplementedError(f"env_id {a.env_id!r}: the device env with a continuous "
                                      "action is Pendulum-v1 (MuJoCo is not available)")
        return make_device_env(a.env_id, a.obs_mode, self.N, a.num_features, self.seed, self.dev,
                               a.buffer_window_size, gamma=a.gamma)

    def _make_agent(self) -> nn.Module:
        return ContAgent(cont_spec(self.obs_shape, self.A))

    # ---- rollout ---------------------------------------------------------------------------
    def _act(self, t: int, env_step: bool = False, hidden=None) -> bool:
        """Step t (:214-220): mean and value of the current observation, cont_actions[t] = z[t] *
        std + mean, logprobs[t], values[t]; with env_step the env steps on that action."""
        ag = self.agent
        x = self.net_obs.flatten(1)
        mean, value = ag.actor_mean(x), ag.critic(x).view(-1)
        if self.fused:
            self.timer.bracket("gauss_head", lambda: ops.gauss_head_sample(
                mean, ag.actor_logstd.view(-1), self.z[t], value, self.cont_actions[t],
                self.logprobs[t], self.values[t]))
        else:
            std = torch.exp(ag.actor_logstd.expand_as(mean))
            action = self.z[t].mul(std).add(mean)
            self.cont_actions[t].copy_(action)
            self.logprobs[t].copy_(gauss_logprob_rows(mean, std, action))
            self.values[t].copy_(value)
        if env_step:
            self.timer.bracket("env_step", lambda: self.env.step(self.cont_actions[t], t))
        return env_step

    def _prepare_minibatches(self, from_records: bool = False):
        """The scalar fields as PPOTrainer gathers them + the action rows by the same
        permutation."""
        super()._prepare_minibatches(from_records)
        self.timer.bracket("gather_actions", lambda: ops.gather_rows(
            self.cont_actions.view(self.B, self.A), self.perm_dev, self.mb_actions))

    # ---- update ----------------------------------------------------------------------------
    def _forward_backward_body(self, j: int):
        """Minibatch j (:265-303): the two MLPs -> the Gaussian PPO loss -> backward."""
        a, ag, mb, M = self.args, self.agent, self.mb, self.M
        sl = slice(j * M, (j + 1) * M)
        self.timer.bracket("gather", lambda: ops.gather_rows(self.b_obs, self.perm_dev[sl],
                                                             self.mb_obs))
        x = self.mb_obs.flatten(1)
        acts = self.mb_actions[sl]
        self.grad_buf.zero_()  # optimizer.zero_grad(): autograd accumulates into the flat buffer
        if self.fused:
            mean, value = ag.actor_mean(x), ag.critic(x)
            md, vd = mean.detach(), value.detach().view(-1)
            self.timer.bracket("gauss_loss", lambda: ops.gauss_ppo_loss_fwd_bwd(
                md, ag.actor_logstd.detach().view(-1), vd, acts, mb["logprobs"][sl],
                mb["advantages"][sl], mb["returns"][sl], mb["values"][sl],
                adv_stats=mb["adv_stats"][j] if a.norm_adv else None, clip_coef=a.clip_coef,
                ent_coef=a.ent_coef, vf_coef=a.vf_coef, norm_adv=a.norm_adv,
                clip_vloss=a.clip_vloss, seed=self.seed, counter=self.rpo_counter, mb=j,
                rpo_alpha=a.rpo_alpha, dmean=self.dmean, dvalue=self.dvalue,
                dlogstd=self.dlogstd, stats=self.stats[j]))
            torch.autograd.backward([mean, value], [self.dmean, self.dvalue.view(-1, 1)])
            ag.actor_logstd.grad.copy_(self.dlogstd.view(1, -1))
            return
        noise = (ops.rpo_noise(self.seed, self.rpo_counter, j, M, self.A, a.rpo_alpha,
                               out=self.rpo_z) if a.rpo_alpha > 0 else None)
        _, newlogprob, entropy, newvalue = ag.get_action_and_value(x, acts, mean_noise=noise)
        logratio = newlogprob - mb["logprobs"][sl]
        ratio = logratio.exp()
        with torch.no_grad():
            old_approx_kl = (-logratio).mean()
            approx_kl = ((ratio - 1) - logratio).mean()
            clipfrac = ((ratio - 1.0).abs() > a.clip_coef).float().mean()
        adv = mb["advantages"][sl]
        adv_mean = adv_std = torch.zeros((), device=self.dev)
        if a.norm_adv:
            adv_mean, adv_std = adv.mean(), adv.std()
            adv = (adv - adv_mean) / (adv_std + 1e-8)
        pg_loss = torch.max(-adv * ratio,
                            -adv * torch.clamp(ratio, 1 - a.clip_coef, 1 + a.clip_coef)).mean()
        newvalue = newvalue.view(-1)
        ret, val = mb["returns"][sl], mb["values"][sl]
        if a.clip_vloss:
            v_clipped = val + torch.clamp(newvalue - val, -a.clip_coef, a.clip_coef)
            v_loss = 0.5 * torch.max((newvalue - ret) ** 2, (v_clipped - ret) ** 2).mean()
        else:
            v_loss = 0.5 * ((newvalue - ret) ** 2).mean()
        entropy_loss = entropy.mean()
        loss = pg_loss - a.ent_coef * entropy_loss + v_loss * a.vf_coef
        self.stats[j].copy_(torch.stack([loss, pg_loss, v_loss, entropy_loss, old_approx_kl,
                                         approx_kl, clipfrac, adv_mean, adv_std]).detach())
        loss.backward()

    # ---- iteration / metrics ---------------------------------------------------------------
    def train_iteration(self, collect_metrics: bool = True, lag: bool = False) -> dict:
        if lag:
            raise NotImplementedError("lagged metrics are not built for this learner")
        # the rollout's draws, before the (captured) rollout reads them
        self.z.normal_(generator=self.gen)
        m = super().train_iteration(collect_metrics, lag=False)
        self.rpo_counter.add_(1)  # a graph replay of the next update draws fresh RPO noise
        return m

    def _lag_ok(self) -> bool:
        return False

    def _metrics(self) -> dict:
        """The script's scalars (:315-322, :229-230)."""
        m = super()._metrics()
        for old, new in (("charts/Episodic_Original_Reward", "charts/episodic_return"),
                         ("charts/Episodic_Length", "charts/episodic_length")):
            if old in m:
                m[new] = m.pop(old)
        self.last_metrics = m
        return m


def run_contppo(args, device=None) -> ContPPOTrainer:
    return run(args, device, trainer_cls=ContPPOTrainer)


def main(argv=None, defaults: dict | None = None,
         description: str = "oc_cleanrl_amd continuous-action PPO (ppo_continuous_action.py "
                            "surface)"):
    return learner_main(ContPPOArgs, finalize, run_contppo, description, argv, defaults)


if __name__ == "__main__":
    main()
