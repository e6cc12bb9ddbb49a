"""QDagger learner of cleanrl/qdagger_dqn_atari_impalacnn.py on the DQN loop (dqn.py).

The script ("reincarnating RL", Agarwal et al. 2022) trains a student Q-network with the help of
a frozen teacher in three phases:
  teacher fill (:283-297)  the teacher acts epsilon-greedily for `teacher_steps` steps into its
                           own replay buffer
  offline      (:300-329)  `offline_steps` train steps of the student on that buffer
  online       (:367-446)  the DQN loop on a fresh buffer, with `global_step` offset by
                           `offline_steps`
and in both training phases the loss is the TD loss plus a temperature-softmax KL between the
teacher's and the student's Q values (:192-195), weighted by 1 offline and, online, by a
coefficient that decays as the student's last ten episodic returns approach the teacher's
evaluated return (:408-411).

`QDaggerTrainer` is `dqn.DQNTrainer` (env step, store, HBM replay, fused acting, FlatAdam, chunk
hipGraphs) with those pieces added:
  ops.qdagger_loss_fwd_bwd   :303-315 / :412-424 and d loss / d q, one launch
  ops.qdagger_episode_push   the deque(maxlen=10) of :365 / :390 and the coefficient of :408-411
                             on the device, one small launch per env step (the online chunk
                             stays one hipGraph; the loss launch reads the coefficient)
The teacher is `dqn.make_qnet` (the script's TeacherModel is dqn_atari.QNetwork) loaded from a
local file; it acts through DQNTrainer's `_actor` hook, so the fill phase runs on the same fused
launches as the student's acting.

Declared differences from the script: no hub download, `teacher_model_path` names a
local file; a teacher mean return of 0 (or a non-finite one) is refused, the script would divide
by it; the IMPALA student has its modules here but no kernels, the trainer refuses it; more than
one env is allowed (the ring takes finished episodes in ascending env order); steps are counted
as DQNTrainer counts them (the count after the step), with the script's offset added.
"""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import evals, ops
from .args import ACTION_COUNTS
from .dqn import DQNArgs, DQNTrainer, learner_main, make_qnet, run_learner

TEACHER_EVAL_EPSILON = 0.05  # :266


@dataclass
class QDaggerArgs:
    """The flags of qdagger_dqn_atari_impalacnn.py:31-98 (same names and defaults) + DQNArgs's
    additions + this learner's own."""
    exp_name: str = "qdagger_dqn_atari_impalacnn"
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
    env_id: str = "BreakoutNoFrameskip-v4"
    total_timesteps: int = 10_000_000
    learning_rate: float = 1e-4
    num_envs: int = 1
    buffer_size: int = 1_000_000
    gamma: float = 0.99
    tau: float = 1.0
    target_network_frequency: int = 1000
    batch_size: int = 32
    start_e: float = 1.0
    end_e: float = 0.01
    exploration_fraction: float = 0.10
    learning_starts: int = 80_000
    train_frequency: int = 4
    teacher_policy_hf_repo: Optional[str] = None  # inert: there is no hub here
    teacher_model_exp_name: str = "dqn_atari"
    teacher_eval_episodes: int = 10
    teacher_steps: int = 500_000
    offline_steps: int = 500_000
    temperature: float = 1.0

    # [oc_cleanrl_amd] additions (as DQNArgs)
    obs_mode: str = "dqn"
    buffer_window_size: int = 4
    backend: str = "Synthetic"  # ALE is not available here
    num_features: int = 12      # object-vector width F per frame (synthetic obj env)
    obs_storage: str = "auto"   # replay obs dtype: auto (u8 pixels / bf16 objects) | f32 | bf16 | u8
    encoder_dims: tuple = (256, 512, 1024, 512)  # QNetworkObj (obs_mode obj)
    decoder_dims: tuple = (512,)
    cuda_graphs: bool = True
    gemm_table: bool = False
    vecnorm_reward: bool = False  # the script has ClipRewardEnv and no VecNormalize
    log_dir: str = "runs"
    log_every: int = 100        # the script logs its losses every 100 steps

    # [oc_cleanrl_amd] QDagger's own
    teacher_model_path: str = ""  # a .cleanrl_model payload of this package or a bare state dict
    teacher_return: Optional[float] = None  # set: skip the teacher evaluation and use this mean
    student_network: str = "auto"  # auto (dqn.make_qnet) | impala (the script's; no kernels yet)


# ---- the script's own student (:126-184): modules, keys and default init -----------------------
def impala_sequence(input_shape, out_channels: int) -> nn.Module:
    """ConvSequence of :141-160: ppg.ConvSequence's modules (the same layout and forward) with the
    default PyTorch init the script leaves them with, instead of PPG's normed one."""
    from .ppg import ConvSequence

    seq = ConvSequence(input_shape, out_channels, 1.0)
    for m in seq.modules():
        if isinstance(m, nn.Conv2d):
            m.reset_parameters()
    return seq


class QNetworkImpala(nn.Module):
    """QNetwork of :164-184: three ConvSequences (16, 32, 32), Flatten, ReLU, Linear 256, ReLU,
    Linear A; forward = network(x / 255). Modules, state-dict keys and init only: the 3x3 pad-1
    residual convolutions and the max-pool have no HIP kernels, so QDaggerTrainer refuses it."""

    def __init__(self, obs_shape, n_actions):
        super().__init__()
        shape, seqs = tuple(obs_shape), []
        for out_channels in (16, 32, 32):
            seq = impala_sequence(shape, out_channels)
            shape = seq.get_output_shape()
            seqs.append(seq)
        self.network = nn.Sequential(*seqs, nn.Flatten(), nn.ReLU(),
                                     nn.Linear(shape[0] * shape[1] * shape[2], 256), nn.ReLU(),
                                     nn.Linear(256, n_actions))

    def forward(self, x):
        return self.network(x / 255.0)


def linear_schedule(start_e: float, end_e: float, duration: float, t: int) -> float:
    """:187-189."""
    slope = (end_e - start_e) / duration
    return max(slope * t + start_e, end_e)


# ---- the teacher -------------------------------------------------------------------------------
def env_shapes(args) -> tuple:
    """(single observation shape, action count) of the env `args` asks for, without making it."""
    W = args.buffer_window_size
    shape = (W, 84, 84) if args.obs_mode == "dqn" else (W, args.num_features)
    return shape, ACTION_COUNTS.get(args.env_id, 6)


def load_teacher(path: str, args) -> nn.Module:
    """The teacher network on the host from `path`: this package's `.cleanrl_model` payload
    ({"model_weights", "args"}; its encoder_dims / decoder_dims build the network) or a bare
    state dict (what the reference's dqn_atari writes). ValueError when the file's network does
    not fit the env's observation shape or action count."""
    if not path:
        raise ValueError("teacher_model_path is empty: QDagger needs a teacher checkpoint (a "
                         ".cleanrl_model file of `python -m oc_cleanrl_amd.dqn`, or a bare state "
                         "dict); there is no hub download here")
    payload = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(payload, dict) and "model_weights" in payload:
        weights, saved = payload["model_weights"], payload.get("args") or {}
    else:
        weights, saved = payload, {}
    if not isinstance(weights, dict) or not all(isinstance(v, torch.Tensor)
                                                for v in weights.values()):
        raise ValueError(f"{path}: neither a .cleanrl_model payload nor a state dict")
    t_args = DQNArgs(obs_mode=args.obs_mode,
                     encoder_dims=tuple(saved.get("encoder_dims", args.encoder_dims)),
                     decoder_dims=tuple(saved.get("decoder_dims", args.decoder_dims)))
    obs_shape, n_actions = env_shapes(args)
    head = [k for k in weights if k.endswith(".weight")][-1]
    if weights[head].shape[0] != n_actions:
        raise ValueError(f"{path}: the teacher has {weights[head].shape[0]} actions, the env "
                         f"{args.env_id} has {n_actions}")
    net = make_qnet(t_args, obs_shape, n_actions)
    try:
        net.load_state_dict(weights)
    except RuntimeError as e:
        raise ValueError(f"{path}: the teacher does not fit observations of shape {obs_shape} "
                         f"(obs_mode {args.obs_mode}): {e}") from None
    return net


def check_teacher_mean(mean: float) -> float:
    mean = float(mean)
    if mean == 0 or not math.isfinite(mean):
        raise ValueError(f"teacher mean return {mean}: the distillation coefficient divides by "
                         "it; it must be finite and not 0")
    return mean


class QDaggerTrainer(DQNTrainer):
    """DQNTrainer's loop with the teacher, the two extra phases and the distillation loss.
    steps(n) advances the online phase (running the earlier phases first when they have not
    run); run_teacher_fill() and run_offline(n) drive them one by one."""

    def __init__(self, args: QDaggerArgs, device, log: bool = True):
        a = args
        if a.student_network == "impala":
            raise NotImplementedError(
                "student_network impala: the script's IMPALA student has its modules here "
                "(qdagger.QNetworkImpala) but no HIP kernels: the 3x3 pad-1 residual convolutions "
                "and the max-pool are missing; use student_network auto")
        if a.student_network != "auto":
            raise ValueError(f"student_network {a.student_network!r}: auto or impala")
        if a.num_envs < 1 or a.teacher_steps < 1 or a.offline_steps < 0:
            raise ValueError("need num_envs >= 1, teacher_steps >= 1 and offline_steps >= 0")
        if not a.temperature > 0:
            raise ValueError(f"temperature {a.temperature} must be > 0")
        teacher = load_teacher(a.teacher_model_path, a)  # on the host: nothing allocated yet
        self.teacher_mean = None if a.teacher_return is None else check_teacher_mean(a.teacher_return)
        self._acting = None
        super().__init__(a, device, log)
        dev, f32 = self.dev, torch.float32
        # the teacher's parameters as views of one flat no-grad buffer, as the target's
        self.teacher = teacher.to(dev).eval()
        t_params = list(self.teacher.parameters())
        offs, n = ops.flat_offsets(t_params)
        self.teacher_flat = torch.zeros(n, dtype=f32, device=dev)
        for p, off in zip(t_params, offs):
            self.teacher_flat[off:off + p.numel()].copy_(p.detach().reshape(-1))
            p.data = self.teacher_flat[off:off + p.numel()].view_as(p)
            p.requires_grad_(False)
        self.td_stats = torch.zeros(5, dtype=f32, device=dev)       # the online loss launch's
        self.offline_stats = torch.zeros(5, dtype=f32, device=dev)  # the offline one's
        self.ring = ops.EpisodeRing(self.E, dev)
        self.teacher_rb = None
        self.phase = "fill"
        self.fill_step = 0
        self.offline_step = 0
        self.train_steps = 0          # online train steps
        self.target_updates = 0       # online target updates
        self.first_train_step = None  # the online step of the first train step
        self._phase_graphs = {"fill": {}, "offline": {}, "online": {}}
        self.graphs = self._phase_graphs["fill"]
        self.step_record = None  # a list: the eager path appends (env.reward, env.done) per step

    # ---- DQNTrainer's hooks ------------------------------------------------------------------
    def _actor(self) -> nn.Module:
        return self._acting if self._acting is not None else self.q

    def _graphable(self) -> bool:
        a = self.args
        return super()._graphable() and a.offline_steps % a.train_frequency == 0

    def _env_step(self, k: int, advance: int = 0) -> bool:
        moved = super()._env_step(k, advance)
        if self.phase == "online":
            ops.qdagger_episode_push(self.env.reward, self.env.done, self.ring, self.teacher_mean)
        return moved

    def _loss_step(self, d: dict, coeff, stats):
        """:303-319 / :412-439 on the batch `d`: student, target and teacher forwards, the loss
        launch, backward through the Q head and the trunk, Adam."""
        a = self.args
        with torch.no_grad():
            q_next = self.target.q_values(d["next_observations"])
            q_teacher = self.teacher.q_values(d["observations"])
        q = self.q.q_values(d["observations"])
        ops.qdagger_loss_fwd_bwd(q.detach(), q_next, q_teacher, d["actions"], d["rewards"],
                                 d["dones"], a.gamma, a.temperature, coeff, dq=self.dq,
                                 stats=stats)
        if not self.direct_grads:
            self.opt.zero_grad()
        q.backward(self.dq)
        self.opt.step()

    def _train_step(self):
        d = self.rb.sample(self.args.batch_size, out=self.batch)
        self._loss_step(d, self.ring.coeff, self.td_stats)

    # ---- teacher evaluation (:258-269) ----------------------------------------------------------
    def evaluate_teacher(self) -> float:
        a = self.args
        if self.teacher_mean is None:
            returns = evals.evaluate(self.teacher, evals.make_env, a.teacher_eval_episodes,
                                     self.dev, epsilon=TEACHER_EVAL_EPSILON, epsilon_seed=a.seed,
                                     env_id=a.env_id, obs_mode=a.obs_mode,
                                     num_features=a.num_features, seed=a.seed,
                                     window=a.buffer_window_size)
            self.teacher_mean = check_teacher_mean(np.mean(returns))
        return self.teacher_mean

    # ---- teacher fill (:283-297) ----------------------------------------------------------------
    def run_teacher_fill(self):
        """`teacher_steps` env steps of the teacher into teacher_rb; epsilon follows
        linear_schedule(start_e, end_e, teacher_steps, step) with the step counted from 0."""
        if self.phase != "fill" or self.fill_step:
            raise RuntimeError("the teacher fill has run already")
        a = self.args
        tf = a.train_frequency
        self.evaluate_teacher()
        self._acting = self.teacher
        self.fused_act = self._fused_act_ok()
        self.duration = float(a.teacher_steps)
        self.step_dev.fill_(-1)  # _env_step acts at step_dev + k + 1: the fill counts from 0
        n = a.teacher_steps
        chunks = n // tf if self._graphable() else 0
        for _ in range(chunks):
            self._run_chunk(train=False)
        for _ in range(n - chunks * tf):
            self._env_step(0)
            self.env.advance(1)
            self.step_dev.add_(1)
        self.fill_step = n
        self._acting = None
        self.fused_act = self._fused_act_ok()
        self.teacher_rb, self.rb = self.rb, None
        self.phase = "offline"
        self.graphs = self._phase_graphs["offline"]

    # ---- offline phase (:300-329) ---------------------------------------------------------------
    def _offline_step(self):
        d = self.teacher_rb.sample(self.args.batch_size, out=self.batch)
        self._loss_step(d, None, self.offline_stats)

    def run_offline(self, n: Optional[int] = None):
        """`n` (default: all that remain) offline train steps on the teacher's buffer. The step
        is one hipGraph; the target update of step % target_network_frequency == 0 (step 0
        included, as in the script) is applied between replays."""
        if self.phase == "fill":
            self.run_teacher_fill()
        if self.phase != "offline":
            raise RuntimeError("the online phase has started: the teacher's buffer is gone")
        a = self.args
        left = a.offline_steps - self.offline_step
        n = left if n is None else n
        if not 0 <= n <= left:
            raise ValueError(f"n={n}: {left} offline steps remain")
        for _ in range(n):
            g = self.graphs.get("step")
            if not a.cuda_graphs:
                self._offline_step()
            elif g is None:
                # warm up eagerly once (creates Adam state / workspaces), then capture
                self._offline_step()
                torch.cuda.synchronize(self.dev)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._offline_step()
                self.graphs["step"] = g
            else:
                g.replay()
            if self.offline_step % a.target_network_frequency == 0:
                self._target_update()
            self.offline_step += 1

    # ---- online phase (:350-446) ----------------------------------------------------------------
    def start_online(self):
        """A fresh replay buffer (the teacher's is dropped: the script never reads it again), the
        env reset to its first step, the step counter at `offline_steps`."""
        if self.phase == "fill":
            self.run_teacher_fill()
        if self.phase == "offline":
            self.run_offline()
        if self.phase == "online":
            return
        a = self.args
        self.teacher_rb = None
        self._phase_graphs["fill"].clear()  # they hold the dropped buffer's address
        self._phase_graphs["offline"].clear()
        self.rb = self._make_replay(self.obs_dtype)
        self.env.step_base.zero_()
        self.env.ep_state.zero_()
        self.ret_state.zero_()
        self.rms_state.copy_(torch.tensor([0.0, 1.0, 1e-4], dtype=torch.float64))
        self.cur = 0
        ops.obs_reset(self.env.reset(), self.stacks[0], self.net_obs)
        self.step_dev.fill_(a.offline_steps)
        self.duration = a.exploration_fraction * a.total_timesteps
        self.global_step = 0
        self.phase = "online"
        self.graphs = self._phase_graphs["online"]

    def steps(self, n: int):
        """Advance the online phase `n` steps (a multiple of train_frequency when graphs are
        used). DQNTrainer.steps with the script's offset: epsilon, `> learning_starts`,
        `% train_frequency` and `% target_network_frequency` all see global_step +
        offline_steps (:368)."""
        self.start_online()
        a = self.args
        tf, off = a.train_frequency, a.offline_steps
        if self._graphable():
            if n % tf:
                raise ValueError(f"n={n} must be a multiple of train_frequency={tf}")
            for _ in range(n // tf):
                end = self.global_step + tf
                train = end + off > a.learning_starts
                self._run_chunk(train=train)
                self.global_step = end
                if train:
                    self._count_train()
                    if (end + off) % a.target_network_frequency == 0:
                        self._target_update()
                        self.target_updates += 1
            return
        for _ in range(n):  # general path: the script's order step by step
            self.global_step += 1
            self._env_step(0)
            if self.step_record is not None:
                self.step_record.append((self.env.reward.tolist(), self.env.done.tolist()))
            self.env.advance(1)
            self.step_dev.add_(1)
            gs = self.global_step + off
            if gs > a.learning_starts:
                if gs % tf == 0:
                    self._train_step()
                    self._count_train()
                if gs % a.target_network_frequency == 0:
                    self._target_update()
                    self.target_updates += 1

    def _count_train(self):
        self.train_steps += 1
        if self.first_train_step is None:
            self.first_train_step = self.global_step

    # ---- metrics / checkpoint -------------------------------------------------------------------
    LOSS_KEY = "losses/td_loss"
    EPISODE_KEYS = ("charts/episodic_return", "charts/episodic_length")

    def metrics(self) -> dict:
        """The script's scalars (:269, :327-329, :387-389, :427-431); one host sync each."""
        m = {"charts/teacher/avg_episodic_return": self.teacher_mean}
        if self.offline_step:
            o = self.offline_stats.tolist()
            m.update({"charts/offline/loss": o[0], "charts/offline/q_loss": o[1],
                      "charts/offline/distill_loss": o[2]})
        if self.phase == "online":
            st = self.td_stats.tolist()
            ep_ret, ep_len, ep_n = self.env.pop_episode_stats()
            m.update({"losses/loss": st[0], "losses/td_loss": st[1], "losses/distill_loss": st[2],
                      "losses/q_values": st[3], "charts/distill_coeff": float(self.ring.coeff),
                      "charts/epsilon": float(self.epsilon)})
            if ep_n > 0:
                m[self.EPISODE_KEYS[0]] = ep_ret / ep_n
                m[self.EPISODE_KEYS[1]] = ep_len / ep_n
        return m

    def checkpoint(self) -> dict:
        """The student's payload in the DQN format (loads into dqn.make_qnet, and serves as the
        next run's teacher)."""
        return {"model_weights": {k: v.detach().clone() for k, v in self.q.state_dict().items()},
                "args": asdict(self.args)}


def run_qdagger(args: QDaggerArgs, device=None) -> QDaggerTrainer:
    """All phases: the first steps() call of run_learner's loop runs the teacher evaluation, the
    fill and the offline phase."""
    return run_learner(QDaggerTrainer, args, device)


def main(argv=None):
    learner_main(QDaggerArgs, run_qdagger,
                 "oc_cleanrl_amd QDagger (qdagger_dqn_atari_impalacnn.py surface)", argv)


if __name__ == "__main__":
    main()
