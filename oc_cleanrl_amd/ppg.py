"""`python -m oc_cleanrl_amd.ppg [ppg_procgen.py flags]` — Phasic Policy Gradient
(cleanrl/ppg_procgen.py) on the device rollout of `trainer.PPOTrainer`.

PPG is an actor-critic whose value head does not shape the shared trunk while the policy is
trained: `critic` reads `hidden.detach()` (:200). A phase is n_iteration policy iterations
(:288-418), each PPO's rollout, GAE and clipped update, whose rollouts' observations and returns
are kept in a buffer of whole rollouts (:415-418), followed by the auxiliary phase (:420-477): the
policy's logits over the whole buffer are recorded, then for e_auxiliary epochs over minibatches of
num_aux_rollouts whole env columns the trunk is trained on the joint loss aux_value_loss +
beta_clone * KL(old policy || new policy) + real_value_loss. Restated here on the trainer's HBM
rollout buffer, staging, flat buffers and hipGraphs:
  * the policy phase is PPOTrainer's iteration with the unfused tail: ops.ppo_loss_fwd_bwd, then
    autograd through the two heads with `critic` on the detached trunk output; with
    adv_norm_fullbatch the loss kernel gets the whole batch's advantage (mean, unbiased std) of
    ops.minibatch_adv_stats for every minibatch (:345), else no normalisation;
  * after every policy iteration the rollout's stored observations (storage dtype, stacks as
    stored) and f32 returns are copied into columns [N (u - 1), N u) of aux_obs / aux_returns;
  * the auxiliary phase is ops.ppg_aux_gather -> trunk -> three heads ->
    ops.ppg_aux_loss_fwd_bwd -> one backward -> clip + Adam, an epoch's minibatches one hipGraph;
  * the optimizer is ops.FlatAdamSegments: `aux_critic` is a segment of its own that sits the
    policy phase out (torch.optim.Adam skips a parameter whose grad is None, :392-394: its moments
    do not decay and its step count does not advance).
`FUSED_PPG = False` selects plain torch ops for the gather and the auxiliary loss and a masked
torch restatement of the segmented Adam step, in the same loop and the same graphs.

Declared differences from the script: no procgen here (--backend Synthetic, the package's device
envs; the reward normalisation is the package's VecNormalize kernel, not gym's NormalizeReward +
clip); `architecture` picks the networks ("PPG_OBJ", the default: agents.object_trunk on object
vectors + the script's three normed heads; "PPG": the script's IMPALA modules, keys and init only,
its trainer path is out of scope); the auxiliary buffer stays in HBM in the rollout's storage
dtype (the script's round trip through the host and its u8 cast are not reproduced); every
auxiliary minibatch starts from zero gradients (the script's first one of a phase accumulates onto
the last policy minibatch's, its zero_grad following the step); n_aux_grad_accum = 1; one GPU. The
script's anneal_lr takes its fraction from the in-phase update index (:291); so does this.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .agents import EnvSpec, _ActorCritic, layer_init, object_trunk
from .args import (CORE_FIXED, CORE_SKIP, check_sampling_noise, learner_args,
                   single_gpu_sizes)
from .trainer import PPOTrainer, _graph_capture, learner_main, run

# The three PPG pieces (ops.ppg_aux_gather, ops.ppg_aux_loss_fwd_bwd, ops.FlatAdamSegments' step);
# False: plain torch ops in their place
FUSED_PPG = True

ARCHITECTURES = ("PPG_OBJ", "PPG")

# ppg_procgen.py:20-98, same names, order and defaults
_REFERENCE_FIELDS = [
    ("exp_name", str, "ppg_procgen"), ("seed", int, 1), ("torch_deterministic", bool, True),
    ("cuda", bool, True), ("track", bool, False), ("wandb_project_name", str, "cleanRL"),
    ("wandb_entity", Optional[str], None), ("capture_video", bool, False),
    ("env_id", str, "starpilot"), ("total_timesteps", int, 25_000_000),
    ("learning_rate", float, 5e-4), ("num_envs", int, 64), ("num_steps", int, 256),
    ("anneal_lr", bool, False), ("gamma", float, 0.999), ("gae_lambda", float, 0.95),
    ("num_minibatches", int, 8), ("adv_norm_fullbatch", bool, True), ("clip_coef", float, 0.2),
    ("clip_vloss", bool, True), ("ent_coef", float, 0.01), ("vf_coef", float, 0.5),
    ("max_grad_norm", float, 0.5), ("target_kl", Optional[float], None),
    ("n_iteration", int, 32), ("e_policy", int, 1), ("v_value", int, 1), ("e_auxiliary", int, 6),
    ("beta_clone", float, 1.0), ("num_aux_rollouts", int, 4), ("n_aux_grad_accum", int, 1),
    ("batch_size", int, 0), ("minibatch_size", int, 0), ("num_iterations", int, 0),
    ("num_phases", int, 0), ("aux_batch_rollouts", int, 0),
]
# [oc_cleanrl_amd] additions: what PPOTrainer reads beyond the script's flags (args.Args' own
# defaults unless listed) and the network choice
_OWN_DEFAULTS = {"architecture": "PPG_OBJ", "obs_mode": "obj", "backend": "Synthetic",
                 "encoder_dims": (128, 64), "decoder_dims": (256,)}
# fields of args.Args with no meaning here: the PPObj-only rollout / update features, DP, the
# optimizer switch (aux_critic needs the segmented step), and PPO's epoch count and minibatch
# advantage normalisation (e_policy and adv_norm_fullbatch stand in their place)
_SKIP = CORE_SKIP | {"fused_heads_loss", "sample_records_min", "conv_channels_last",
                     "fused_optimizer", "update_epochs", "norm_adv"}
_FIXED = CORE_FIXED + (("fused_heads_loss", False), ("sample_records_min", -1),
                       ("conv_channels_last", False), ("fused_optimizer", True),
                       ("norm_adv", False))

PPGArgs = learner_args(
    "PPGArgs", "The flags of ppg_procgen.py:20-98 (same names, order and defaults) + this "
               "build's additions.",
    _REFERENCE_FIELDS, _SKIP, _OWN_DEFAULTS, fixed=_FIXED)


def finalize(args, world_size: int = 1, trainer: bool = True):
    """Derived sizes (ppg_procgen.py:216-221) and the checks of args.finalize that apply.
    trainer: the arguments are for PPGTrainer, which trains PPG_OBJ only (False: for building the
    modules)."""
    if args.architecture not in ARCHITECTURES:
        raise NotImplementedError(f"architecture must be one of {ARCHITECTURES}")
    if (args.obs_mode == "obj") != (args.architecture == "PPG_OBJ"):
        raise ValueError('architecture PPG_OBJ reads --obs_mode obj, PPG reads pixels (dqn)')
    if trainer and args.architecture != "PPG_OBJ":
        raise NotImplementedError("architecture PPG: PPGTrainer trains PPG_OBJ; the IMPALA "
                                  "network's residual convolutions have no kernel here (DESIGN 8)")
    if args.v_value != 1:  # the script asserts the same (:221)
        raise NotImplementedError("v_value != 1: multiple value epochs are not supported")
    if args.n_aux_grad_accum != 1:
        raise NotImplementedError("n_aux_grad_accum != 1: gradient accumulation over auxiliary "
                                  "minibatches is not built (DESIGN 8)")
    check_sampling_noise(args)
    if min(args.n_iteration, args.e_policy, args.e_auxiliary, args.num_aux_rollouts) < 1:
        raise ValueError("n_iteration, e_policy, e_auxiliary and num_aux_rollouts must be >= 1")
    single_gpu_sizes(args, world_size, "the PPG learner")
    args.num_phases = int(args.num_iterations // args.n_iteration)
    args.aux_batch_rollouts = int(args.num_envs * args.n_iteration)
    args.update_epochs = args.e_policy  # PPOTrainer's name for the policy epochs
    if args.minibatch_size < 1 or args.batch_size % args.num_minibatches:
        raise ValueError(f"batch size {args.batch_size} must be divisible by num_minibatches="
                         f"{args.num_minibatches}")
    if args.aux_batch_rollouts % args.num_aux_rollouts:
        raise ValueError(f"aux_batch_rollouts {args.aux_batch_rollouts} must be divisible by "
                         f"num_aux_rollouts={args.num_aux_rollouts} (the script's last auxiliary "
                         "minibatch would be short)")
    return args


def layer_init_normed(layer, norm_dim, scale=1.0):
    """ppg_procgen.py:101-105: every output unit's weights scaled to L2 norm `scale`, zero bias."""
    with torch.no_grad():
        layer.weight.data *= scale / layer.weight.norm(dim=norm_dim, p=2, keepdim=True)
        layer.bias *= 0
    return layer


class ResidualBlock(nn.Module):
    """ppg_procgen.py:124-140."""

    def __init__(self, channels, scale):
        super().__init__()
        scale = np.sqrt(scale)
        self.conv0 = layer_init_normed(nn.Conv2d(channels, channels, 3, padding=1), (1, 2, 3), scale)
        self.conv1 = layer_init_normed(nn.Conv2d(channels, channels, 3, padding=1), (1, 2, 3), scale)

    def forward(self, x):
        inputs = x
        x = self.conv0(nn.functional.relu(x))
        x = self.conv1(nn.functional.relu(x))
        return x + inputs


class ConvSequence(nn.Module):
    """ppg_procgen.py:143-165."""

    def __init__(self, input_shape, out_channels, scale):
        super().__init__()
        self._input_shape, self._out_channels = input_shape, out_channels
        self.conv = layer_init_normed(nn.Conv2d(input_shape[0], out_channels, 3, padding=1),
                                      (1, 2, 3), 1.0)
        scale = scale / np.sqrt(2)  # two residual blocks
        self.res_block0 = ResidualBlock(out_channels, scale)
        self.res_block1 = ResidualBlock(out_channels, scale)

    def forward(self, x):
        x = nn.functional.max_pool2d(self.conv(x), kernel_size=3, stride=2, padding=1)
        return self.res_block1(self.res_block0(x))

    def get_output_shape(self):
        _c, h, w = self._input_shape
        return (self._out_channels, (h + 1) // 2, (w + 1) // 2)


class PPGAgent(_ActorCritic):
    """Agent of ppg_procgen.py:168-211 with its state-dict keys (network.*, actor, critic,
    aux_critic) and head init. architecture "PPG": the script's IMPALA trunk on channel-first
    pixel stacks (d = 256); "PPG_OBJ": agents.object_trunk on object vectors (d = the decoder's
    width). `critic` reads the detached trunk output wherever the script's does."""

    grads_in_place = False  # three consumers of the trunk output: autograd sums their gradients

    def __init__(self, envs, architecture: str = "PPG_OBJ", device=None, encoder_dims=(128, 64),
                 decoder_dims=(256,)):
        super().__init__()
        if architecture not in ARCHITECTURES:
            raise NotImplementedError(architecture)
        self.device = device
        self.pixels = architecture == "PPG"
        dims = tuple(envs.observation_space.shape)
        if self.pixels:
            shape, seqs, chans = dims, [], [16, 32, 32]
            scale = 1 / np.sqrt(len(chans))
            for c in chans:
                seq = ConvSequence(shape, c, scale=scale)
                shape = seq.get_output_shape()
                seqs.append(seq)
            top = layer_init_normed(nn.Linear(shape[0] * shape[1] * shape[2], 256), 1, 1.4)
            layers, d = seqs + [nn.Flatten(), nn.ReLU(), top, nn.ReLU()], 256
        else:
            layers, d = object_trunk(dims, tuple(encoder_dims), tuple(decoder_dims), layer_init)
        self.network = nn.Sequential(*layers)
        A = envs.action_space.n
        self.actor = layer_init_normed(nn.Linear(d, A), norm_dim=1, scale=0.1)
        self.critic = layer_init_normed(nn.Linear(d, 1), norm_dim=1, scale=0.1)
        self.aux_critic = layer_init_normed(nn.Linear(d, 1), norm_dim=1, scale=0.1)

    def trunk(self, x, prescaled: bool = False):
        if self.pixels and not prescaled:
            x = x / 255.0
        return super().trunk(x, prescaled)

    def heads(self, hidden):
        """(logits, value) of the policy phase (:196-200): the value reads hidden.detach()."""
        # the trunk's last layer leaves its ReLU backward to a single consumer (its box): there
        # are several here, so they read a view that carries no box
        h = hidden.view(hidden.shape)
        return self._head(self.actor, h), self._head(self.critic, h.detach())

    def heads3(self, hidden):
        """(logits, value, aux value) of the auxiliary phase (:206-208)."""
        h = hidden.view(hidden.shape)
        return (self._head(self.actor, h), self._head(self.critic, h.detach()),
                self._head(self.aux_critic, h))

    def get_action_and_value(self, x, action=None):
        """(action, log_prob, entropy, value) like the script (:194-200)."""
        logits, value = self.heads(self.trunk(x))
        probs = torch.distributions.Categorical(logits=logits)
        if action is None:
            action = probs.sample()
        return action, probs.log_prob(action), probs.entropy(), value

    # get_value is _ActorCritic's: critic(network(x)), no detach (:202-203)

    def get_pi_value_and_aux_value(self, x):
        logits, value, aux = self.heads3(self.trunk(x))
        return torch.distributions.Categorical(logits=logits), value, aux

    def get_pi(self, x):
        return torch.distributions.Categorical(logits=self._head(self.actor, self.trunk(x)))

    def head_parameters(self):
        """Everything torch.optim.Adam steps in the policy phase (all but aux_critic)."""
        tail = {id(p) for p in self.aux_critic.parameters()}
        return [p for p in self.parameters() if id(p) not in tail]


class _MaskedAdam:
    """FUSED_PPG = False: ops.FlatAdamSegments' step restated in torch ops on the same flat
    buffers and device scalars (f32 scalars as ocppo_clip_adam_step forms them; capturable)."""

    def __init__(self, opt: ops.FlatAdamSegments):
        self.o = opt
        dev = opt.scalars.device
        self.b1 = torch.tensor(opt.betas[0], dtype=torch.float32, device=dev)
        self.b2 = torch.tensor(opt.betas[1], dtype=torch.float32, device=dev)

    def step(self, tail_active: bool):
        o, b1, b2 = self.o, self.b1, self.b2
        s, sp = o.scalars, o.split
        s[ops.OPT_STEP] += 1.0
        if not tail_active:
            s[ops.OPT_TAIL_SKIPPED] += 1.0
        n = o.numel if tail_active else sp
        total = torch.sqrt((o.grads[:n] * o.grads[:n]).sum())
        clip = torch.clamp(o.max_grad_norm / (total + 1e-6), max=1.0) if o.max_grad_norm > 0 \
            else torch.ones_like(total)
        segs = [(slice(0, sp), s[ops.OPT_STEP])]
        if tail_active:
            segs.append((slice(sp, o.numel), s[ops.OPT_STEP] - s[ops.OPT_TAIL_SKIPPED]))
        for sl, t in segs:
            g = o.grads[sl] * clip
            m, v, p = o.exp_avg[sl], o.exp_avg_sq[sl], o.params[sl]
            m.mul_(b1).add_((1.0 - b1) * g)
            v.mul_(b2).add_((1.0 - b2) * g * g)
            step_size = o.lr / (1.0 - torch.pow(b1, t))
            denom = v.sqrt() / torch.sqrt(1.0 - torch.pow(b2, t)) + o.eps
            p.sub_(step_size * m / denom)
        if tail_active:
            s[ops.OPT_TAIL_STEP] = s[ops.OPT_STEP] - s[ops.OPT_TAIL_SKIPPED]


class PPGTrainer(PPOTrainer):
    """PPOTrainer's rollout buffer, staging, flat buffers and graphs with PPG's additions: the
    value gradient stopped at the head, full-batch advantage normalisation, the auxiliary buffer
    of whole rollouts, the auxiliary phase and an optimizer whose aux_critic segment sits the
    policy phase out."""

    def __init__(self, args, device, *a, **k):
        if args.architecture != "PPG_OBJ":
            raise NotImplementedError("PPGTrainer trains PPG_OBJ only (DESIGN 8)")
        self.fused = FUSED_PPG
        super().__init__(args, device, *a, **k)
        if self.world != 1 or self.dp:
            raise NotImplementedError("the PPG learner runs on one GPU")
        f32, dev, a = torch.float32, self.dev, args
        T, N, A = self.T, self.N, self.A
        self.R, self.K = a.aux_batch_rollouts, a.num_aux_rollouts
        R, K = self.R, self.K
        self.naux = R // K  # auxiliary minibatches per epoch
        self.aux_obs = torch.zeros((T, R) + self.obs_shape, dtype=self.obs_dtype, device=dev)
        self.aux_returns = torch.zeros((T, R), dtype=f32, device=dev)
        self.aux_pi = torch.zeros((T, R, A), dtype=f32, device=dev)
        self.full_stats = torch.zeros((1, 2), dtype=f32, device=dev)
        self.batch_order = torch.arange(self.B, dtype=torch.int64, device=dev)
        # the auxiliary epochs' column shuffles: drawn on the host when the phase begins, the
        # current epoch's in aux_perm_dev (what the graph reads)
        self.aux_perm_host = torch.empty(a.e_auxiliary * R, dtype=torch.int64, pin_memory=True)
        self.aux_perm_all = torch.zeros(a.e_auxiliary * R, dtype=torch.int64, device=dev)
        self.aux_perm_dev = torch.zeros(R, dtype=torch.int64, device=dev)
        self.aux_cols = torch.arange(R, dtype=torch.int64, device=dev)  # the old-policy pass
        self.aux_mb_obs = torch.zeros((T * K,) + self.obs_shape, dtype=f32, device=dev)
        self.aux_mb_pi = torch.zeros((T * K, A), dtype=f32, device=dev)
        self.aux_mb_ret = torch.zeros(T * K, dtype=f32, device=dev)
        self.aux_dlogits = torch.zeros((T * K, A), dtype=f32, device=dev)
        self.aux_dvalue = torch.zeros(T * K, dtype=f32, device=dev)
        self.aux_daux = torch.zeros(T * K, dtype=f32, device=dev)
        self.aux_stats = torch.zeros((self.naux, len(ops.PPG_STAT_NAMES)), dtype=f32, device=dev)
        self.torch_opt = None if self.fused else _MaskedAdam(self.optimizer)
        self.phase, self.update = 0, 0  # phases finished, policy iterations done in this phase
        self.aux_ran = False  # an auxiliary phase has run eagerly (the graphs' warm-up)
        self.g_aux = self.g_aux_pi = None
        self.aux_metrics: dict = {}

    def _make_agent(self) -> nn.Module:
        a = self.args
        return PPGAgent(EnvSpec(self.obs_shape, self.A), a.architecture, None, a.encoder_dims,
                        a.decoder_dims)

    def _make_optimizer(self):
        """optim.Adam(agent.parameters(), lr, eps=1e-8) (:265) with aux_critic a segment of its
        own."""
        a = self.args
        return ops.FlatAdamSegments(self.agent.head_parameters(),
                                    self.agent.aux_critic.parameters(), lr=a.learning_rate,
                                    eps=1e-8, max_grad_norm=a.max_grad_norm)

    def _weight_planes(self):
        # FlatAdamSegments writes no planes and this agent's GEMMs take none: nothing to refresh
        return None

    def _fused_tail(self, j: int, hidden) -> bool:
        return False  # the fused heads + loss kernel sends the value gradient into the trunk

    # ---- policy phase ------------------------------------------------------------------------
    def _rollout_end(self):
        """PPOTrainer's bootstrap, GAE and minibatch gather, then the whole batch's advantage
        (mean, unbiased std) for every minibatch's loss launch (:345)."""
        super()._rollout_end()
        if self.args.adv_norm_fullbatch:
            self.timer.bracket("adv_stats_full", lambda: ops.minibatch_adv_stats(
                self.advantages.view(-1), self.batch_order, self.B, out=self.full_stats))

    def _forward_backward_body(self, j: int):
        """Policy minibatch j (:356-392): PPO's loss on the full-batch-normalised advantage, the
        value's gradient ending at `critic`."""
        a, mb = self.args, self.mb
        sl = slice(j * self.M, (j + 1) * self.M)
        logits, value = self.agent.heads(self._minibatch_hidden(j))
        lg, vv = logits.detach(), value.detach().view(-1)
        norm = a.adv_norm_fullbatch
        self.timer.bracket("ppo_loss", lambda: ops.ppo_loss_fwd_bwd(
            lg, vv, mb["actions"][sl], mb["logprobs"][sl], mb["advantages"][sl],
            mb["returns"][sl], mb["values"][sl], mb_inds=None,
            adv_stats=self.full_stats[0] if norm else None, clip_coef=a.clip_coef,
            ent_coef=a.ent_coef, vf_coef=a.vf_coef, norm_adv=norm, clip_vloss=a.clip_vloss,
            dlogits=self.dlogits, dvalue=self.dvalue, stats=self.stats[j],
            workspace=self.loss_ws))
        self.grad_buf.zero_()  # optimizer.zero_grad() (:391)
        torch.autograd.backward([logits, value], [self.dlogits, self.dvalue.view(-1, 1)])

    def _opt_step(self, tail_active: bool = False):
        """The policy phase's step leaves aux_critic out (its grad is None in the script)."""
        if self.fused:
            self.timer.bracket("adam_seg_tail" if tail_active else "adam_seg",
                               lambda: self.optimizer.step(tail_active))
        else:
            self.torch_opt.step(tail_active)

    # ---- auxiliary phase ---------------------------------------------------------------------
    def _aux_gather(self, cols):
        if self.fused:
            self.timer.bracket("ppg_aux_gather", lambda: ops.ppg_aux_gather(
                self.aux_obs, self.aux_pi, self.aux_returns, cols, self.aux_mb_obs,
                self.aux_mb_pi, self.aux_mb_ret))
            return
        flat = lambda t: t.index_select(1, cols).reshape((-1,) + tuple(t.shape[2:]))  # noqa: E731
        self.aux_mb_obs.copy_(flat(self.aux_obs))  # copy_ converts the storage dtype to f32
        self.aux_mb_pi.copy_(flat(self.aux_pi))
        self.aux_mb_ret.copy_(flat(self.aux_returns))

    def _aux_old_policy(self):
        """aux_pi: the policy's logits over the whole buffer, num_aux_rollouts columns at a time
        (:424-434)."""
        T, K = self.T, self.K
        with torch.no_grad():
            for i in range(self.naux):
                self._aux_gather(self.aux_cols[i * K:(i + 1) * K])
                ag = self.agent
                logits = ag._head(ag.actor, ag.trunk(self.aux_mb_obs))
                self.aux_pi[:, i * K:(i + 1) * K].copy_(logits.view(T, K, self.A))

    def _aux_minibatch(self, i: int):
        """Auxiliary minibatch i of the current epoch (:439-467)."""
        a, K = self.args, self.K
        self._aux_gather(self.aux_perm_dev[i * K:(i + 1) * K])
        logits, value, aux = self.agent.heads3(self.agent.trunk(self.aux_mb_obs))
        st = self.aux_stats[i]
        if self.fused:
            lg, vv, av = logits.detach(), value.detach().view(-1), aux.detach().view(-1)
            self.timer.bracket("ppg_aux_loss", lambda: ops.ppg_aux_loss_fwd_bwd(
                lg, vv, av, self.aux_mb_pi, self.aux_mb_ret, a.beta_clone, self.aux_dlogits,
                self.aux_dvalue, self.aux_daux, st))
            self.grad_buf.zero_()
            torch.autograd.backward(
                [logits, value, aux],
                [self.aux_dlogits, self.aux_dvalue.view(-1, 1), self.aux_daux.view(-1, 1)])
        else:
            kl, avl, rvl = aux_losses_torch(logits, value.view(-1), aux.view(-1), self.aux_mb_pi,
                                            self.aux_mb_ret)
            st.copy_(torch.stack([kl.detach(), avl.detach(), rvl.detach()]))
            self.grad_buf.zero_()
            (avl + a.beta_clone * kl + rvl).backward()
        self._opt_step(tail_active=True)

    def _aux_epoch(self):
        for i in range(self.naux):
            self._aux_minibatch(i)

    def _aux_shuffle(self):
        """np.random.shuffle(aux_inds) once per auxiliary epoch (:438), the indices carried from
        epoch to epoch as the script carries them, all epochs staged before the first replay."""
        a, R = self.args, self.R
        inds = np.arange(R)
        out = self.aux_perm_host.numpy()
        for e in range(a.e_auxiliary):
            self.np_rng.shuffle(inds)
            out[e * R:(e + 1) * R] = inds
        self.aux_perm_all.copy_(self.aux_perm_host, non_blocking=True)

    def _capture_aux(self):
        torch.cuda.synchronize(self.dev)
        pool = self.g_rollout.pool() if self.g_rollout is not None else None
        self.g_aux_pi = torch.cuda.CUDAGraph()
        with _graph_capture(self.g_aux_pi, pool):
            self._aux_old_policy()
        self.g_aux = torch.cuda.CUDAGraph()
        with _graph_capture(self.g_aux, pool if pool is not None else self.g_aux_pi.pool()):
            self._aux_epoch()

    def auxiliary_phase(self) -> dict:
        """:420-477 over the buffer the phase's policy iterations filled."""
        a, R = self.args, self.R
        self._aux_shuffle()
        if a.cuda_graphs and self.aux_ran and self.g_aux is None:
            self._capture_aux()
        replay = self.g_aux is not None
        self.g_aux_pi.replay() if replay else self._aux_old_policy()
        for e in range(a.e_auxiliary):
            self.aux_perm_dev.copy_(self.aux_perm_all[e * R:(e + 1) * R])
            self.g_aux.replay() if replay else self._aux_epoch()
        self.aux_ran = True
        last = self.aux_stats[self.naux - 1].cpu().numpy()  # sync point
        self.aux_metrics = {f"losses/aux/{n}": float(v) for n, v in zip(ops.PPG_STAT_NAMES, last)}
        return self.aux_metrics

    # ---- iteration / metrics -----------------------------------------------------------------
    def run_iterations(self) -> int:
        """Whole phases only (ppg_procgen.py:285-288): num_phases of n_iteration iterations."""
        return self.args.num_phases * self.args.n_iteration

    def train_iteration(self, collect_metrics: bool = True, lag: bool = False) -> dict:
        """One policy iteration; the phase's last one is followed by the auxiliary phase."""
        a = self.args
        last = self.update + 1 == a.n_iteration
        anneal, prefetch = a.anneal_lr, a.prefetch_shuffle
        if anneal:  # the in-phase update index, as the script has it (:291)
            self.lr.fill_((1.0 - float(self.update) / max(a.num_iterations, 1)) * a.learning_rate)
        # the auxiliary epochs' shuffles come before the next policy iteration's in the stream
        a.anneal_lr, a.prefetch_shuffle = False, prefetch and not last
        try:
            m = super().train_iteration(collect_metrics, False)
        finally:
            a.anneal_lr, a.prefetch_shuffle = anneal, prefetch
        sl = slice(self.N * self.update, self.N * (self.update + 1))
        self.aux_obs[:, sl].copy_(self.obs[:self.T])  # :416-418, device to device
        self.aux_returns[:, sl].copy_(self.returns)
        self.update += 1
        if last:
            aux = self.auxiliary_phase()
            self.update, self.phase = 0, self.phase + 1
            if prefetch:
                self._shuffle()
            if collect_metrics:
                m.update(aux)
                self.last_metrics = m
        return m

    def _lag_ok(self) -> bool:
        return False

    def state_dict_checkpoint(self) -> dict:
        ck = super().state_dict_checkpoint()
        o, n = self.optimizer, self.N * self.update
        ck["optimizer"] = {"scalars": o.scalars.clone(), "exp_avg": o.exp_avg.clone(),
                           "exp_avg_sq": o.exp_avg_sq.clone()}
        ck["phase"], ck["update"] = self.phase, self.update
        ck["aux_obs"], ck["aux_returns"] = self.aux_obs[:, :n].clone(), self.aux_returns[:, :n].clone()
        return ck

    def load_checkpoint(self, ck: dict):
        """The agent, the optimizer's moments and both step counts, and the phase position (with
        the part of the auxiliary buffer the phase has filled) of a state_dict_checkpoint
        payload."""
        self.agent.load_state_dict(ck["model_weights"])
        o = self.optimizer
        for k in ("scalars", "exp_avg", "exp_avg_sq"):
            getattr(o, k).copy_(ck["optimizer"][k])
        self.phase, self.update = int(ck["phase"]), int(ck["update"])
        n = self.N * self.update
        self.aux_obs[:, :n].copy_(ck["aux_obs"])
        self.aux_returns[:, :n].copy_(ck["aux_returns"])


def aux_losses_torch(logits, value, aux_value, old_logits, returns):
    """(kl_loss, aux_value_loss, real_value_loss) of ppg_procgen.py:453-458 in plain torch ops
    that a graph can capture: Categorical's normalisation and kl_divergence's two masks written
    out (its boolean-mask assignments read the mask back on the host)."""
    def norm(l):
        ln = l - l.logsumexp(dim=-1, keepdim=True)
        return ln, torch.softmax(ln, dim=-1)

    ln_old, p_old = norm(old_logits)
    ln_new, p_new = norm(logits)
    t = p_old * (ln_old - ln_new)
    t = torch.where(p_new == 0, torch.full_like(t, float("inf")), t)
    t = torch.where(p_old == 0, torch.zeros_like(t), t)
    kl = t.sum(-1).mean()
    real = 0.5 * ((value - returns) ** 2).mean()
    auxl = 0.5 * ((aux_value - returns) ** 2).mean()
    return kl, auxl, real


def run_ppg(args, device=None) -> PPGTrainer:
    """The script body: num_phases phases of n_iteration policy iterations and an auxiliary
    phase each (PPGTrainer.run_iterations / train_iteration), SPS, metrics JSONL, checkpoints."""
    return run(args, device, trainer_cls=PPGTrainer)


def main(argv=None):
    return learner_main(PPGArgs, finalize, run_ppg,
                        "oc_cleanrl_amd PPG (ppg_procgen.py surface)", argv)


if __name__ == "__main__":
    main()
