"""`python -m oc_cleanrl_amd.sac_continuous [sac_continuous_action.py flags]` — Soft Actor-Critic
with a tanh-squashed Gaussian policy, on td3.TD3Trainer's loop and HBM-resident state.
(oc_cleanrl_amd.sac is the discrete sac_atari.py.)

The script's loop per global step g (counted from 0): act (uniform while g < learning_starts, else
one draw of the policy, :233-237), env step, rb.add with the terminal observation of a truncated
episode (:252-256), then if g > learning_starts a critic update against the entropy-regularised
twin target (:263-280); every `policy_frequency` steps, `policy_frequency` actor steps each
followed by a temperature step on a fresh draw (:282-304); every `target_network_frequency` steps
the two critics' soft update (:307-311). Here:
  ops.csac_act                  both heads + both acting phases, the branch on the device counter
  envs.PendulumVecEnv(raw)      the env behind RecordEpisodeStatistics only
  ops.ContReplayBuffer          TD3's float-action replay; a sample is the critics' input
  ops.csac_sample_forward       the target's action into next_obs_act and its log-prob; the
                                temperature's fresh log-prob
  ops.csac_critic_loss_fwd_bwd  min - alpha * logp', TD target, both MSEs, dq1 / dq2
  ops.csac_sample               the actor loss's critic input and log-prob, and their backward
  ops.csac_actor_loss_fwd_bwd   mean(alpha * logp - min(q1, q2)), dq1, dq2, dlogp
  ops.csac_alpha_step           alpha_loss, log_alpha's Adam step, alpha on ops.SacTemperature
  ops.polyak_ / ops.FlatAdam    the soft update; Adam over one flat buffer per optimizer
The three 256-wide MLPs are torch's GEMMs. lcm(policy_frequency, target_network_frequency) global
steps are one hipGraph (a fill and a train graph; the chunk around learning_starts runs eagerly).
FUSED_CSAC = False selects plain torch for everything but the replay, on the same draws
(ops.csac_noise).

Declared differences from the script: env_id defaults to Pendulum-v1 (Hopper-v4 needs MuJoCo);
learning_starts keeps the script's float default 5e3 and is compared as int(learning_starts); the
random phase, the policy's draws and the replay indices are the library's counter streams, not
numpy's / torch's generators; log_prob is formed from the draw z (-z^2 / 2 - log_std), which
Normal.log_prob equals up to rounding, and its 1 - tanh(x)^2 from exp(-2 |x|), not from the rounded
tanh; the actor step forms only the actor's gradients (the script
leaves stray ones on the critics and zeroes them before their next use, :278); checkpoint()
returns (actor, qf1, qf2) state dicts and save_model writes them (the script saves nothing).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .dqn import learner_main, run_learner
from .td3 import Critics, QNetwork, TD3Trainer, _flat_target, act_mu, box_spec  # noqa: F401

# The fused kernels (ops.csac_*, polyak_); False: plain torch on the same draws. The replay is
# ops.ContReplayBuffer either way.
FUSED_CSAC = True

LOG_STD_MAX = 2
LOG_STD_MIN = -5
HALF_LOG_2PI = math.log(math.sqrt(2 * math.pi))


@dataclass
class ContSACArgs:
    """The flags of sac_continuous_action.py:18-65 (same names, order and defaults; env_id: see
    the module docstring) + this build's additions."""
    exp_name: str = "sac_continuous_action"
    seed: int = 1
    torch_deterministic: bool = True
    cuda: bool = True
    track: bool = False
    wandb_project_name: str = "cleanRL"
    wandb_entity: Optional[str] = None
    capture_video: bool = False
    env_id: str = "Pendulum-v1"
    total_timesteps: int = 1000000
    num_envs: int = 1
    buffer_size: int = int(1e6)
    gamma: float = 0.99
    tau: float = 0.005
    batch_size: int = 256
    learning_starts: float = 5e3  # the script annotates int and writes 5e3: int() where compared
    policy_lr: float = 3e-4
    q_lr: float = 1e-3
    policy_frequency: int = 2
    target_network_frequency: int = 1
    alpha: float = 0.2
    autotune: bool = True

    # [oc_cleanrl_amd] additions (as TD3Args; save_model: the script saves nothing)
    backend: str = "Synthetic"
    cuda_graphs: bool = True
    log_dir: str = "runs"
    log_every: int = 100  # the script logs its losses every 100 steps
    save_model: bool = False

    # what run_learner / learner_main read under the value-based learners' names (no annotation:
    # not flags)
    obs_mode = "obj"

    @property
    def train_frequency(self) -> int:
        return chunk_length(self.policy_frequency, self.target_network_frequency)


class Actor(nn.Module):
    """sac_continuous_action.py:105-150 (keys fc1, fc2, fc_mean, fc_logstd, the buffers
    action_scale / action_bias)."""

    def __init__(self, env):
        super().__init__()
        sp = env.single_action_space
        n = int(np.prod(sp.shape))
        self.fc1 = nn.Linear(int(np.array(env.single_observation_space.shape).prod()), 256)
        self.fc2 = nn.Linear(256, 256)
        self.fc_mean = nn.Linear(256, n)
        self.fc_logstd = nn.Linear(256, n)
        self.register_buffer("action_scale", torch.tensor((sp.high - sp.low) / 2.0,
                                                          dtype=torch.float32))
        self.register_buffer("action_bias", torch.tensor((sp.high + sp.low) / 2.0,
                                                         dtype=torch.float32))

    def hidden(self, x):
        return F.relu(self.fc2(F.relu(self.fc1(x))))

    def heads(self, x):
        """(mean, r): fc_mean's and fc_logstd's outputs, the latter before tanh."""
        h = self.hidden(x)
        return self.fc_mean(h), self.fc_logstd(h)

    def forward(self, x):
        mean, r = self.heads(x)
        return mean, log_std_of(r)

    def get_action(self, x):
        """The script's get_action (:138-150) on torch's generator."""
        mean, log_std = self(x)
        normal = torch.distributions.Normal(mean, log_std.exp())
        x_t = normal.rsample()
        y_t = torch.tanh(x_t)
        action = y_t * self.action_scale + self.action_bias
        log_prob = normal.log_prob(x_t)
        log_prob = log_prob - torch.log(self.action_scale * (1 - y_t.pow(2)) + 1e-6)
        log_prob = log_prob.sum(1, keepdim=True)
        return action, log_prob, torch.tanh(mean) * self.action_scale + self.action_bias


def log_std_of(r):
    """:133-134."""
    return LOG_STD_MIN + 0.5 * (LOG_STD_MAX - LOG_STD_MIN) * (torch.tanh(r) + 1)


def squash(mean, r, z, action_scale, action_bias):
    """get_action (:138-150) on the heads' outputs and the draw z, in ops.csac_sample's order of
    operations: (action [B, A], log_prob [B, 1]). log_prob's Normal term is -z^2 / 2 - log_std
    (what Normal.log_prob(mean + std * z) is before rounding), summed over columns in order;
    1 - tanh(x)^2 is 4 e / (1 + e)^2 with e = exp(-2 |x|), accurate at any x, where 1 - y * y from
    the rounded y is decided by y's last bit once |x| passes ~3."""
    log_std = log_std_of(r)
    x = mean + torch.exp(log_std) * z
    action = torch.tanh(x) * action_scale + action_bias
    e = torch.exp(-2.0 * torch.abs(x))
    q = 1.0 + e
    t = ((-(z * z) * 0.5 - log_std) - HALF_LOG_2PI) \
        - torch.log(action_scale * ((4.0 * e) / (q * q)) + 1e-6)
    lp = t[:, 0]
    for a in range(1, t.shape[1]):
        lp = lp + t[:, a]
    return action, lp.unsqueeze(1)


class SquashTorch(torch.autograd.Function):
    """squash with its backward spelled out in torch ops, in ops.csac_sample's backward's order of
    operations: what the FUSED_CSAC = False path differentiates, so that both paths take bitwise
    the same steps (autograd's own backward of squash differs from the kernel by rounding; the
    kernel is checked against it under DESIGN 11's rule)."""

    @staticmethod
    def forward(ctx, mean, r, z, action_scale, action_bias):
        with torch.no_grad():
            action, lp = squash(mean, r, z, action_scale, action_bias)
        ctx.save_for_backward(mean, r, z, action_scale)
        return action, lp

    @staticmethod
    def backward(ctx, daction, dlogp):
        mean, r, z, scale = ctx.saved_tensors
        t = torch.tanh(r)
        sigma = torch.exp(LOG_STD_MIN + 0.5 * (LOG_STD_MAX - LOG_STD_MIN) * (t + 1))
        x = mean + sigma * z
        y = torch.tanh(x)
        e = torch.exp(-2.0 * torch.abs(x))
        q = 1.0 + e
        s2 = (4.0 * e) / (q * q)
        u = scale * s2 + 1e-6
        gx = (daction * scale + ((dlogp / u) * scale) * (2.0 * y)) * s2
        dls = (gx * z) * sigma - dlogp
        return gx, (dls * (0.5 * (LOG_STD_MAX - LOG_STD_MIN))) * (1 - t * t), None, None, None


def make_networks(spec):
    """(actor, critics, target critics) constructed in the script's order (:199-205): actor, qf1,
    qf2, then qf1_target and qf2_target, which consume the generator before being overwritten.
    There is no target actor."""
    actor = Actor(spec)
    q = Critics(QNetwork(spec), QNetwork(spec))
    q_target = Critics(QNetwork(spec), QNetwork(spec))
    q_target.load_state_dict(q.state_dict())
    return actor, q, q_target


def chunk_length(policy_frequency: int, target_network_frequency: int) -> int:
    """The period of the train step's schedule: a graph chunk."""
    return math.lcm(int(policy_frequency), int(target_network_frequency))


def train_schedule(g: int, learning_starts: int, policy_frequency: int,
                   target_network_frequency: int):
    """(acts at random, trains, runs the actor / temperature block, soft-updates the targets) at
    global step g (:233, :262, :282, :307)."""
    trains = g > learning_starts
    return (g < learning_starts, trains, trains and g % policy_frequency == 0,
            trains and g % target_network_frequency == 0)


class ContSACTrainer(TD3Trainer):
    """td3.TD3Trainer's loop (acting, env step, replay, chunk graphs) with continuous SAC's
    networks, train step and schedule. device_env: as TD3Trainer."""

    WHO = "continuous SAC"
    CHUNK_NAME = "lcm(policy_frequency, target_network_frequency)"

    def _refuse(self, a, device_env):
        super()._refuse(a, device_env)
        if a.target_network_frequency < 1:
            raise ValueError(f"target_network_frequency = {a.target_network_frequency} must be at "
                             "least 1")

    def _configure(self, a):
        self.twin = True
        self.fused = FUSED_CSAC

    def _build_networks(self, spec):
        a, dev = self.args, self.dev
        actor, q, q_target = make_networks(spec)
        self.actor, self.q, self.target = actor.to(dev), q.to(dev), q_target.to(dev)
        self.q_opt = ops.FlatAdam(self.q.parameters(), lr=a.q_lr)              # :206
        self.actor_opt = ops.FlatAdam(self.actor.parameters(), lr=a.policy_lr)  # :207
        self.tq_flat = _flat_target(self.target, dev)
        # :210-216; a_optimizer is default Adam (eps 1e-8)
        self.temp = ops.SacTemperature(dev, a.autotune, a.alpha, lr=a.q_lr,
                                       target_entropy=-float(self.A), eps=1e-8)

    def _build_policy_buffers(self, B: int):
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.dev)  # noqa: E731
        self.dqa1, self.dqa2, self.dlogp = z(B, 1), z(B, 1), z(B, 1)
        self.pi_loss, self.alpha_loss = z(1), z(1)

    @property
    def chunk_len(self) -> int:
        return chunk_length(self.args.policy_frequency, self.args.target_network_frequency)

    # ---- acting --------------------------------------------------------------------------------
    def _act(self, k: int):
        """:233-237 at global step step_dev + k."""
        a, ac = self.args, self.actor
        h = ac.hidden(self.obs)
        if self.fused:
            ops.csac_act(h, ac.fc_mean.weight, ac.fc_mean.bias, ac.fc_logstd.weight,
                         ac.fc_logstd.bias, ac.action_scale, ac.action_bias, self.low, self.high,
                         a.seed, self.step_dev, self.learning_starts, self.actions, step_offset=k)
            return
        u = ops.csac_noise(a.seed, self.step_dev, self.E, self.A, offset=k, uniform=True)
        z = ops.csac_noise(a.seed, self.step_dev, self.E, self.A, offset=k)
        rand = self.low + (self.high - self.low) * u
        rand = torch.where(rand >= self.high, self.high_below, rand)
        mean = act_mu(h, ac.fc_mean.weight, ac.fc_mean.bias)
        r = act_mu(h, ac.fc_logstd.weight, ac.fc_logstd.bias)
        act = torch.tanh(mean + torch.exp(log_std_of(r)) * z) * ac.action_scale + ac.action_bias
        self.actions.copy_(torch.where(self.step_dev + k < self.learning_starts, rand, act))

    # ---- the train step ------------------------------------------------------------------------
    def _draw(self, draw: int):
        return ops.csac_noise(self.args.seed, self.rb.counter, self.args.batch_size, self.A,
                              draw=draw)

    def update_critics(self, d: dict):
        """:264-280 on the sampled batch d."""
        a, ac, D, alpha = self.args, self.actor, self.D, self.temp.alpha
        xa, nxa = d["obs_act"], d["next_obs_act"]
        rewards, dones = d["rewards"], d["dones"]
        with torch.no_grad():
            mean, r = ac.heads(d["next_observations"])
            if self.fused:
                nlogp = ops.csac_sample_forward(mean, r, ac.action_scale, ac.action_bias, a.seed,
                                                self.rb.counter, ops.CSAC_TARGET_DRAW, xa=nxa)
            else:
                nact, nlogp = squash(mean, r, self._draw(ops.CSAC_TARGET_DRAW), ac.action_scale,
                                     ac.action_bias)
                nxa[:, D:].copy_(nact)
            q1t, q2t = self.target.q_values(nxa)
        q1, q2 = self.q.q_values(xa)
        self.q_opt.zero_grad()
        if self.fused:
            ops.csac_critic_loss_fwd_bwd(q1t, q2t, q1.detach(), q2.detach(), rewards, dones, nlogp,
                                         alpha, a.gamma, dq1=self.dq1, dq2=self.dq2,
                                         stats=self.q_stats)
            torch.autograd.backward([q1, q2], [self.dq1, self.dq2])
        else:
            nq = torch.min(q1t, q2t) - alpha * nlogp
            y = rewards.flatten() + (1 - dones.flatten()) * a.gamma * nq.view(-1)
            q1v, q2v = q1.view(-1), q2.view(-1)
            l1, l2 = F.mse_loss(q1v, y), F.mse_loss(q2v, y)
            (l1 + l2).backward()
            self.q_stats.copy_(torch.stack([l1, l2, q1v.mean(), q2v.mean()]).detach())
        self.q_opt.step()

    def update_policy(self, d: dict, i: int):
        """Iteration i of :283-304: the actor step, then the temperature step on a fresh draw."""
        a, ac, alpha = self.args, self.actor, self.temp.alpha
        mean, r = ac.heads(d["observations"])
        self.actor_opt.zero_grad()
        if self.fused:
            xa, logp = ops.csac_sample(mean, r, d["obs_act"], ac.action_scale, ac.action_bias,
                                       a.seed, self.rb.counter, ops.csac_policy_draw(i))
            q1, q2 = self.q.q_values(xa)
            ops.csac_actor_loss_fwd_bwd(q1.detach(), q2.detach(), logp.detach(), alpha,
                                        dq1=self.dqa1, dq2=self.dqa2, dlogp=self.dlogp,
                                        loss=self.pi_loss)
            # only the actor's gradients: the script's stray ones on the critics are zeroed unread
            torch.autograd.backward([q1, q2, logp], [self.dqa1, self.dqa2, self.dlogp],
                                    inputs=self.actor_params)
        else:
            act, logp = SquashTorch.apply(mean, r, self._draw(ops.csac_policy_draw(i)),
                                          ac.action_scale, ac.action_bias)
            q1, q2 = self.q(d["observations"], act)
            loss = ((alpha * logp) - torch.min(q1, q2)).mean()
            loss.backward()
            self.pi_loss.copy_(loss.detach().view(1))
        self.actor_opt.step()
        if not self.temp.autotune:
            return
        with torch.no_grad():
            mean, r = ac.heads(d["observations"])
            if self.fused:
                logp = ops.csac_sample_forward(mean, r, ac.action_scale, ac.action_bias, a.seed,
                                               self.rb.counter, ops.csac_alpha_draw(i))
                ops.csac_alpha_step(logp, self.temp, loss=self.alpha_loss)
            else:
                _, logp = squash(mean, r, self._draw(ops.csac_alpha_draw(i)), ac.action_scale,
                                 ac.action_bias)
                self._alpha_step_torch(logp)

    def _alpha_step_torch(self, logp):
        """:299-304 in torch ops on the temperature's device buffers (no host value, so it can
        be captured): torch.optim.Adam's single-tensor step with its step scalars in double; the
        batch mean in f64, as the kernel's."""
        t = self.temp
        b1, b2 = t.betas
        ea = t.log_alpha.exp()
        mean = (logp + t.target_entropy).double().mean()
        self.alpha_loss.copy_((-ea.double() * mean).float())
        grad = -ea * mean.float()
        t.step.add_(1)
        n = t.step.double()
        t.exp_avg.lerp_(grad, 1 - b1)
        t.exp_avg_sq.mul_(b2).addcmul_(grad, grad, value=1 - b2)
        step_size = (t.lr / (1 - b1 ** n)).float()
        denom = t.exp_avg_sq.sqrt() / (1 - b2 ** n).sqrt().float() + t.eps
        t.log_alpha.add_((-step_size * t.exp_avg) / denom)
        t.alpha.copy_(t.log_alpha.exp())

    def _target_update(self):
        tau = self.args.tau
        if self.fused:
            ops.polyak_([(self.q_opt.params, self.tq_flat)], tau)
            return
        self.tq_flat.copy_(tau * self.q_opt.params + (1.0 - tau) * self.tq_flat)

    def _train_step(self, policy: bool, target: bool):
        d = self.rb.sample(self.args.batch_size, out=self.batch)
        self.update_critics(d)
        if policy:
            for i in range(self.args.policy_frequency):
                self.update_policy(d, i)
        if target:
            self._target_update()

    def _step(self, k: int, g: int):
        """Global step g = the chunk's first step + k."""
        a = self.args
        _, trains, policy, target = train_schedule(g, self.learning_starts, a.policy_frequency,
                                                   a.target_network_frequency)
        self._env_step(k)
        if trains:
            self._train_step(policy, target)

    # ---- metrics / checkpoint ------------------------------------------------------------------
    def metrics(self) -> dict:
        """The script's scalars (:314-328); one host sync."""
        pf = self.args.policy_frequency
        q1l, q2l, q1v, q2v, pi, al, alpha = torch.cat(
            [self.q_stats, self.pi_loss, self.alpha_loss, self.temp.alpha]).tolist()
        m = {"losses/qf1_values": q1v, "losses/qf2_values": q2v, "losses/qf1_loss": q1l,
             "losses/qf2_loss": q2l, "losses/qf_loss": (q1l + q2l) / 2.0, "losses/alpha": alpha}
        if self.global_step > (self.learning_starts // pf + 1) * pf:  # a policy step has run
            m["losses/actor_loss"] = pi
            if self.temp.autotune:
                m["losses/alpha_loss"] = al
        ep_ret, ep_len, ep_n = self.env.pop_episode_stats()
        if ep_n > 0:
            m["charts/episodic_return"] = ep_ret / ep_n
            m["charts/episodic_length"] = ep_len / ep_n
        return m


def run_sac_continuous(args, device=None) -> ContSACTrainer:
    return run_learner(ContSACTrainer, args, device)


def main(argv=None):
    learner_main(ContSACArgs, run_sac_continuous,
                 "oc_cleanrl_amd continuous SAC (sac_continuous_action.py surface)", argv)


if __name__ == "__main__":
    main()
