"""`python -m oc_cleanrl_amd.td3 [td3_continuous_action.py flags]` — TD3, and through
oc_cleanrl_amd.ddpg the DDPG of ddpg_continuous_action.py (the same loop with one critic and no
target-policy noise), on HBM-resident state.

The scripts' loop per global step g (counted from 0): act (uniform while g < learning_starts,
else actor + exploration noise, :205-211), env step, rb.add with the terminal observation of a
truncated episode (:226-230), then if g > learning_starts a critic update (:237-260) and, every
`policy_frequency` steps, the actor update and the soft target updates (:262-274). Here:
  ops.td3_act                  fc_mu + both acting phases, the branch on the device step counter
  envs.PendulumVecEnv(raw)     the env behind RecordEpisodeStatistics only
  ops.ContReplayBuffer         the float-action replay; a sample is the critics' input
  ops.td3_target_actions       the smoothed target action into next_obs_act's action columns
  ops.td3_critic_loss_fwd_bwd  min, TD target, both MSEs, dq1 / dq2
  ops.td3_policy_actions       the actor loss's critic input and its backward
  ops.polyak_                  all soft target updates of a policy step in one launch
  ops.FlatAdam                 Adam over one flat buffer per optimizer
The three 256-wide MLPs are torch's GEMMs. `policy_frequency` global steps are one hipGraph (a
fill and a train graph; the chunk around learning_starts runs eagerly). FUSED_TD3 = False selects
plain torch for everything but the replay, on the same noise (ops.td3_noise / td3_target_noise).

`TD3Trainer` presents what dqn.run_learner / learner_main drive (steps, metrics, checkpoint,
_graphable, global_step) without subclassing DQNTrainer, whose constructor is the Atari env, the
frame stacks, int64 actions and the memory-optimised replay.

Declared differences from the scripts: env_id defaults to Pendulum-v1 (Hopper-v4 needs MuJoCo);
learning_starts keeps the scripts' float default 25e3 and is compared as int(learning_starts);
the random phase, the exploration noise, the target-policy noise and the replay indices are the
library's counter streams, not numpy's / torch's generators; the actor step does not form the
stray gradients the script leaves on qf1 (it zeroes them before their next use, :258); DDPG takes
num_envs (its script is fixed at one env).
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .dqn import learner_main, run_learner

# The fused kernels (ops.td3_act, td3_target_actions, td3_critic_loss_fwd_bwd, td3_policy_actions,
# polyak_); False: plain torch on the same draws. The replay is ops.ContReplayBuffer either way.
FUSED_TD3 = True


@dataclass
class TD3Args:
    """The flags of td3_continuous_action.py:18-69 (same names, order and defaults; env_id: see
    the module docstring) + this build's additions."""
    exp_name: str = "td3_continuous_action"
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
    num_envs: int = 1
    buffer_size: int = int(1e6)
    gamma: float = 0.99
    tau: float = 0.005
    batch_size: int = 256
    policy_noise: float = 0.2
    exploration_noise: float = 0.1
    learning_starts: float = 25e3  # the script annotates int and writes 25e3: int() where compared
    policy_frequency: int = 2
    noise_clip: float = 0.5

    # [oc_cleanrl_amd] additions (as SACArgs)
    backend: str = "Synthetic"
    cuda_graphs: bool = True
    log_dir: str = "runs"
    log_every: int = 100  # the script logs its losses every 100 steps

    # what run_learner / learner_main read under the value-based learners' names (no annotation:
    # not flags)
    obs_mode = "obj"
    twin = True

    @property
    def train_frequency(self) -> int:
        return self.policy_frequency


def box_spec(obs_dim: int, low, high):
    """An `envs`-like object with a flat observation space and a Box action space."""
    low, high = np.asarray(low, np.float32).reshape(-1), np.asarray(high, np.float32).reshape(-1)
    if low.shape != high.shape or low.size < 1 or not (low < high).all():
        raise ValueError(f"action bounds low={low.tolist()} high={high.tolist()}")
    act = SimpleNamespace(shape=(low.size,), low=low, high=high)
    return SimpleNamespace(single_observation_space=SimpleNamespace(shape=(int(obs_dim),)),
                           single_action_space=act, action_space=act)


class QNetwork(nn.Module):
    """td3_continuous_action.py:87-102 (keys fc1, fc2, fc3, default PyTorch init)."""

    def __init__(self, env):
        super().__init__()
        n = int(np.array(env.single_observation_space.shape).prod()
                + np.prod(env.single_action_space.shape))
        self.fc1 = nn.Linear(n, 256)
        self.fc2 = nn.Linear(256, 256)
        self.fc3 = nn.Linear(256, 1)

    def forward(self, x, a):
        return self.q_values(torch.cat([x, a], 1))

    def q_values(self, xa):
        """forward on the concatenated input [B, D + A] (a replay sample's obs_act)."""
        return self.fc3(F.relu(self.fc2(F.relu(self.fc1(xa)))))


class Actor(nn.Module):
    """td3_continuous_action.py:105-131 (keys fc1, fc2, fc_mu, the buffers action_scale /
    action_bias)."""

    def __init__(self, env):
        super().__init__()
        sp = env.single_action_space
        self.fc1 = nn.Linear(int(np.array(env.single_observation_space.shape).prod()), 256)
        self.fc2 = nn.Linear(256, 256)
        self.fc_mu = nn.Linear(256, int(np.prod(sp.shape)))
        self.register_buffer("action_scale", torch.tensor((sp.high - sp.low) / 2.0,
                                                          dtype=torch.float32))
        self.register_buffer("action_bias", torch.tensor((sp.high + sp.low) / 2.0,
                                                         dtype=torch.float32))

    def hidden(self, x):
        return F.relu(self.fc2(F.relu(self.fc1(x))))

    def pre(self, x):
        """fc_mu's output, before tanh."""
        return self.fc_mu(self.hidden(x))

    def forward(self, x):
        return torch.tanh(self.pre(x)) * self.action_scale + self.action_bias


class Critics(nn.Module):
    """qf1 (and TD3's qf2) as one module, as sac.TwinCritic: its parameters() are the script's
    `list(qf1.parameters()) + list(qf2.parameters())` (:187), so one FlatAdam and one flat target
    buffer cover both."""

    def __init__(self, qf1: nn.Module, qf2: Optional[nn.Module] = None):
        super().__init__()
        self.qf1 = qf1
        if qf2 is not None:
            self.qf2 = qf2
        self.twin = qf2 is not None

    def q_values(self, xa):
        return self.qf1.q_values(xa), (self.qf2.q_values(xa) if self.twin else None)

    def forward(self, x, a):
        return self.q_values(torch.cat([x, a], 1))


def make_networks(spec, twin: bool = True):
    """(actor, critics, target_actor, target critics) constructed in the script's order
    (:178-186): actor, qf1, qf2, then qf1_target, qf2_target and target_actor, which consume the
    generator before being overwritten (DDPG, ddpg_continuous_action.py:160-165: without the
    qf2s)."""
    actor = Actor(spec)
    q = Critics(QNetwork(spec), QNetwork(spec) if twin else None)
    q_target = Critics(QNetwork(spec), QNetwork(spec) if twin else None)
    target_actor = Actor(spec)
    target_actor.load_state_dict(actor.state_dict())
    q_target.load_state_dict(q.state_dict())
    return actor, q, target_actor, q_target


def act_mu(h, w, b):
    """h @ w.T + b in ops.td3_act's summation order (H a multiple of 64): lane l adds its
    products j = l, l + 64, ... in order, the 64 lanes combine by the xor butterfly, then the
    bias. The unfused path uses it so that both paths act bitwise alike."""
    E, H = h.shape
    A = w.shape[0]
    if H % 64:
        raise ValueError(f"act_mu: hidden width {H} is not a multiple of 64")
    p = h.view(E, 1, H // 64, 64) * w.view(1, A, H // 64, 64)
    acc = p[:, :, 0]
    for c in range(1, H // 64):
        acc = acc + p[:, :, c]
    lane = torch.arange(64, device=h.device)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., lane ^ off]
    return acc[..., 0] + b


def train_schedule(g: int, learning_starts: int, policy_frequency: int):
    """(acts at random, trains, updates the policy) at global step g (:205, :236, :262)."""
    trains = g > learning_starts
    return g < learning_starts, trains, trains and g % policy_frequency == 0


def _flat_target(module: nn.Module, dev):
    """The module's parameters as views of one flat buffer laid out as ops.FlatAdam lays out the
    online ones (dqn.DQNTrainer's target construction)."""
    params = list(module.parameters())
    offs, n = ops.flat_offsets(params)
    flat = torch.zeros(n, dtype=torch.float32, device=dev)
    for p, off in zip(params, offs):
        flat[off:off + p.numel()].copy_(p.detach().reshape(-1))
        p.data = flat[off:off + p.numel()].view_as(p)
        p.requires_grad_(False)
    return flat


class TD3Trainer:
    """device_env: a device-resident vector env in place of the one env_id names -- the interface
    of envs.PendulumVecEnv(raw=True): frame [E, D] / reward / done [E] / final_frame [E, D]
    written by step(actions [E, A] f32, step_offset), reset() -> frame, advance(n),
    pop_episode_stats(), n_actions, action_low / action_high, and optionally terminated [E]."""

    def __init__(self, args, device, log: bool = True, device_env=None):
        a = args
        self._refuse(a, device_env)
        self.args = a
        self._configure(a)
        self.learning_starts = int(a.learning_starts)
        self.dev = dev = torch.device(device)
        torch.use_deterministic_algorithms(a.torch_deterministic)
        torch.utils.deterministic.fill_uninitialized_memory = False  # see dqn.DQNTrainer
        torch.backends.cudnn.deterministic = a.torch_deterministic
        torch.manual_seed(a.seed)
        self.E = E = a.num_envs
        if device_env is None:
            from .envs import PendulumVecEnv

            device_env = PendulumVecEnv(E, a.seed, dev, raw=True)
        self.env = env = device_env
        self.A = A = int(env.n_actions)
        self.D = D = int(env.frame.shape[1])
        spec = box_spec(D, env.action_low, env.action_high)
        self._build_networks(spec)
        self.actor_params = list(self.actor.parameters())
        f32 = torch.float32
        sp = spec.single_action_space
        self.low = torch.tensor(sp.low, dtype=f32, device=dev)
        self.high = torch.tensor(sp.high, dtype=f32, device=dev)
        self.high_below = torch.nextafter(self.high, self.low)
        self.low0, self.high0 = float(sp.low[0]), float(sp.high[0])  # :244's scalar bounds
        # SB3 keeps buffer_size // n_envs rows of n_envs transitions
        self.rb = ops.ContReplayBuffer(max(a.buffer_size // E, 1), E, D, A, dev, seed=a.seed)
        B = a.batch_size
        self.batch = self.rb.batch(B)
        self.obs = torch.zeros((E, D), dtype=f32, device=dev)
        self.actions = torch.zeros((E, A), dtype=f32, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=dev)  # the chunk's first step
        self.dq1 = torch.zeros((B, 1), dtype=f32, device=dev)
        self.dq2 = torch.zeros((B, 1), dtype=f32, device=dev) if self.twin else None
        self.q_stats = torch.zeros(4, dtype=f32, device=dev)
        self._build_policy_buffers(B)
        self.global_step = 0  # the next step's index = the steps taken
        self.log_enabled = log
        self.graphs: dict = {}
        self.obs.copy_(env.reset())  # :202

    # ---- what a learner on this loop (sac_continuous.ContSACTrainer) replaces -------------------
    WHO = "TD3"
    CHUNK_NAME = "policy_frequency"  # what chunk_len is, in steps()'s refusal

    def _refuse(self, a, device_env):
        """Every refusal, before any device work."""
        if a.backend != "Synthetic":
            raise NotImplementedError("MuJoCo / gymnasium are not available; use --backend "
                                      "Synthetic")
        if device_env is None and a.env_id != "Pendulum-v1":
            raise NotImplementedError(f"env_id {a.env_id!r}: the device env with a continuous "
                                      "action is Pendulum-v1 (MuJoCo is not available)")
        if device_env is not None and device_env.n_actions > ops.GAUSS_MAX_ACTIONS:
            raise ValueError(f"{device_env.n_actions} action dimensions: the {self.WHO} kernels "
                             f"take at most {ops.GAUSS_MAX_ACTIONS}")
        if a.policy_frequency < 1:
            raise ValueError(f"policy_frequency = {a.policy_frequency} must be at least 1")
        if a.batch_size < 1:
            raise ValueError(f"batch_size = {a.batch_size} must be at least 1")

    def _configure(self, a):
        self.twin = bool(a.twin)
        self.fused = FUSED_TD3
        self.policy_noise = float(a.policy_noise) if self.twin else 0.0

    def _build_networks(self, spec):
        a, dev = self.args, self.dev
        actor, q, target_actor, q_target = make_networks(spec, self.twin)
        self.actor, self.q = actor.to(dev), q.to(dev)
        self.target_actor, self.target = target_actor.to(dev), q_target.to(dev)
        self.q_opt = ops.FlatAdam(self.q.parameters(), lr=a.learning_rate)          # :187
        self.actor_opt = ops.FlatAdam(self.actor.parameters(), lr=a.learning_rate)  # :188
        self.tq_flat = _flat_target(self.target, dev)
        self.ta_flat = _flat_target(self.target_actor, dev)

    def _build_policy_buffers(self, B: int):
        f32, dev = torch.float32, self.dev
        self.dqa = torch.full((B, 1), -(1.0 / B), dtype=f32, device=dev)  # d (-q.mean()) / d q
        self.pi_q = torch.zeros((B, 1), dtype=f32, device=dev)  # qf1(s, actor(s)) of :263

    @property
    def chunk_len(self) -> int:
        """The global steps of one graph chunk: the period of the train step's schedule."""
        return self.args.policy_frequency

    # ---- acting --------------------------------------------------------------------------------
    def _act(self, k: int):
        """:205-211 at global step step_dev + k."""
        a, ac = self.args, self.actor
        h = ac.hidden(self.obs)
        if self.fused:
            ops.td3_act(h, ac.fc_mu.weight, ac.fc_mu.bias, ac.action_scale, ac.action_bias,
                        self.low, self.high, a.seed, self.step_dev, self.learning_starts,
                        a.exploration_noise, self.actions, step_offset=k)
            return
        u = ops.td3_noise(a.seed, self.step_dev, self.E, self.A, k, uniform=True)
        z = ops.td3_noise(a.seed, self.step_dev, self.E, self.A, k)
        rand = self.low + (self.high - self.low) * u
        rand = torch.where(rand >= self.high, self.high_below, rand)
        act = torch.tanh(act_mu(h, ac.fc_mu.weight, ac.fc_mu.bias)) * ac.action_scale \
            + ac.action_bias
        act = torch.clamp(act + (ac.action_scale * a.exploration_noise) * z, self.low, self.high)
        self.actions.copy_(torch.where(self.step_dev + k < self.learning_starts, rand, act))

    def _env_step(self, k: int):
        """One global step up to `obs = next_obs` (:205-233)."""
        env = self.env
        with torch.no_grad():
            self._act(k)
        env.step(self.actions, k)
        self.rb.add(self.obs, env.frame, env.final_frame, env.done, self.actions, env.reward,
                    getattr(env, "terminated", None), carry=True)

    # ---- the train step ------------------------------------------------------------------------
    def update_critics(self, d: dict):
        """:238-260 on the sampled batch d."""
        a, ac, D = self.args, self.actor, self.D
        xa, nxa = d["obs_act"], d["next_obs_act"]
        rewards, dones = d["rewards"], d["dones"]
        with torch.no_grad():
            mu_t = self.target_actor.pre(d["next_observations"])
            if self.fused:
                ops.td3_target_actions(mu_t, ac.action_scale, ac.action_bias, nxa, a.seed,
                                       self.rb.counter, self.policy_noise, a.noise_clip,
                                       self.low0, self.high0)
            else:
                nact = torch.tanh(mu_t) * ac.action_scale + ac.action_bias
                if self.policy_noise != 0:
                    z = ops.td3_target_noise(a.seed, self.rb.counter, mu_t.shape[0], self.A)
                    noise = (z * self.policy_noise).clamp(-a.noise_clip, a.noise_clip) \
                        * ac.action_scale
                    nact = (nact + noise).clamp(self.low0, self.high0)
                nxa[:, D:].copy_(nact)
            q1t, q2t = self.target.q_values(nxa)
        q1, q2 = self.q.q_values(xa)
        self.q_opt.zero_grad()
        if self.fused:
            ops.td3_critic_loss_fwd_bwd(q1t, q2t, q1.detach(), q2.detach() if self.twin else None,
                                        rewards, dones, a.gamma, dq1=self.dq1, dq2=self.dq2,
                                        stats=self.q_stats)
            if self.twin:
                torch.autograd.backward([q1, q2], [self.dq1, self.dq2])
            else:
                q1.backward(self.dq1)
        else:
            nq = torch.min(q1t, q2t) if self.twin else q1t
            y = rewards.flatten() + (1 - dones.flatten()) * a.gamma * nq.view(-1)
            q1v = q1.view(-1)
            l1 = F.mse_loss(q1v, y)
            zero = torch.zeros((), device=self.dev)
            if self.twin:
                q2v = q2.view(-1)
                l2 = F.mse_loss(q2v, y)
                (l1 + l2).backward()
                st = [l1, l2, q1v.mean(), q2v.mean()]
            else:
                l1.backward()
                st = [l1, zero, q1v.mean(), zero]
            self.q_stats.copy_(torch.stack(st).detach())
        self.q_opt.step()

    def update_policy(self, d: dict):
        """:263-274: the actor step against qf1 after its update, then the soft target updates."""
        a, ac = self.args, self.actor
        mu = ac.pre(d["observations"])
        self.actor_opt.zero_grad()
        if self.fused:
            qa = self.q.qf1.q_values(ops.td3_policy_actions(mu, d["obs_act"], ac.action_scale,
                                                            ac.action_bias))
            # only the actor's gradients: the script's stray ones on qf1 are zeroed unread (:258)
            torch.autograd.backward([qa], [self.dqa], inputs=self.actor_params)
        else:
            act = torch.tanh(mu) * ac.action_scale + ac.action_bias
            qa = self.q.qf1(d["observations"], act)
            (-qa.mean()).backward()
        self.pi_q.copy_(qa.detach())
        self.actor_opt.step()
        self._target_update()

    def _target_update(self):
        tau = self.args.tau
        if self.fused:
            ops.polyak_([(self.actor_opt.params, self.ta_flat), (self.q_opt.params, self.tq_flat)],
                        tau)
            return
        self.ta_flat.copy_(tau * self.actor_opt.params + (1.0 - tau) * self.ta_flat)
        self.tq_flat.copy_(tau * self.q_opt.params + (1.0 - tau) * self.tq_flat)

    def _train_step(self, policy: bool):
        d = self.rb.sample(self.args.batch_size, out=self.batch)
        self.update_critics(d)
        if policy:
            self.update_policy(d)

    # ---- the loop ------------------------------------------------------------------------------
    def _step(self, k: int, g: int):
        """Global step g = the chunk's first step + k."""
        _, trains, policy = train_schedule(g, self.learning_starts, self.args.policy_frequency)
        self._env_step(k)
        if trains:
            self._train_step(policy)

    def _chunk(self, base: int):
        n = self.chunk_len
        for k in range(n):
            self._step(k, base + k)
        self.env.advance(n)
        self.step_dev.add_(n)

    def _graphable(self) -> bool:
        return bool(self.args.cuda_graphs)

    def _run_chunk(self, base: int):
        n, ls = self.chunk_len, self.learning_starts
        if base + n - 1 <= ls:
            key = "fill"   # no step of the chunk trains
        elif base > ls:
            key = "train"  # every step trains; the policy step is the chunk's first
        else:
            return self._chunk(base)  # the chunk around learning_starts: once, eagerly
        g = self.graphs.get(key)
        if g is None:
            # warm up eagerly once (creates Adam state / workspaces), then capture
            self._chunk(base)
            torch.cuda.synchronize(self.dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._chunk(base)
            self.graphs[key] = g
            return
        g.replay()

    def steps(self, n: int):
        """Advance `n` global steps; with graphs, n and the steps already taken are multiples of
        policy_frequency (a chunk is policy_frequency steps starting at such a multiple)."""
        c = self.chunk_len
        if self._graphable():
            if n % c or self.global_step % c:
                raise ValueError(f"n={n} (after {self.global_step} steps) must be a multiple of "
                                 f"{self.CHUNK_NAME}={c}")
            for _ in range(n // c):
                self._run_chunk(self.global_step)
                self.global_step += c
            return
        for _ in range(n):  # the script's order step by step
            self._step(0, self.global_step)
            self.env.advance(1)
            self.step_dev.add_(1)
            self.global_step += 1

    # ---- metrics / checkpoint ------------------------------------------------------------------
    def metrics(self) -> dict:
        """The scripts' scalars (:277-282; DDPG :241-243); one host sync."""
        pf = self.args.policy_frequency
        q = self.q_stats.tolist()
        m = {"losses/qf1_values": q[2], "losses/qf1_loss": q[0]}
        if self.twin:
            m.update({"losses/qf2_values": q[3], "losses/qf2_loss": q[1],
                      "losses/qf_loss": (q[0] + q[1]) / 2.0})
        if self.global_step > (self.learning_starts // pf + 1) * pf:  # a policy step has run
            m["losses/actor_loss"] = -float(self.pi_q.mean())
        ep_ret, ep_len, ep_n = self.env.pop_episode_stats()
        if ep_n > 0:
            m["charts/episodic_return"] = ep_ret / ep_n
            m["charts/episodic_length"] = ep_len / ep_n
        return m

    def checkpoint(self):
        """The scripts' payload (:292; DDPG :249): the tuple of state dicts."""
        sd = lambda m: {k: v.detach().clone() for k, v in m.state_dict().items()}  # noqa: E731
        out = (sd(self.actor), sd(self.q.qf1))
        return out + (sd(self.q.qf2),) if self.twin else out


def run_td3(args, device=None) -> TD3Trainer:
    return run_learner(TD3Trainer, args, device)


def main(argv=None, args_cls=TD3Args,
         description: str = "oc_cleanrl_amd TD3 (td3_continuous_action.py surface)"):
    learner_main(args_cls, run_td3, description, argv)


if __name__ == "__main__":
    main()
