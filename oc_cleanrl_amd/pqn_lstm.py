"""`python -m oc_cleanrl_amd.pqn_lstm [pqn_atari_envpool_lstm.py flags]` — the recurrent PQN
learner (cleanrl/pqn_atari_envpool_lstm.py): PQN with a single-layer nn.LSTM between the trunk and
the Q head.

Both halves exist in this package and were written to compose; this module is the composition:
  * `pqn.py`: epsilon-greedy acting on the Q head, Q(lambda) targets, the MSE loss on the taken
    action, RAdam (PQNTrainer; ops.pqn_act, ops.q_lambda, ops.ln_relu, ops.pqn_loss_fwd_bwd,
    ops.FlatRAdam);
  * `lstm.py`: the masked recurrence and the trainer that carries (h, c) across steps and
    iterations, snapshots the state a rollout starts from, draws environment-wise minibatches
    and recurs each from its slice of that state (lstm.Recurrence, LSTMTrainer; ops.lstm_seq,
    ops.lstm_step).
`PQNLSTMTrainer(LSTMTrainer, PQNTrainer)`: LSTMTrainer._act steps the LSTM and hands the new h to
PQNTrainer._act as `hidden=`; LSTMTrainer._minibatch_hidden feeds PQNTrainer's loss. What is this
module's own are the two places where the halves meet, each one fused call
(csrc/ocppo_pqn_lstm.hip):
  * the rollout step -- LSTM step + Q head + greedy value + epsilon-greedy action -- is ONE launch
    (ops.pqn_lstm_act), bitwise ops.lstm_step followed by ops.pqn_act; the bootstrap (:287) is the
    same launch with commit=False (no state copy, no separate step and head);
  * the update's Q head + loss + head backward is ONE call (ops.pqn_head_loss_fwd_bwd) on the
    recurrence's output: one dot product per row instead of a Linear, a loss and two GEMMs.

Switches. FUSED_PQN_LSTM is the master switch of this module's two fused calls;
FUSED_PQN_LSTM_ACT / FUSED_PQN_LSTM_LOSS select each. With any of them off the trainer runs that
part as the composition of the parents' existing kernels (ops.lstm_step + ops.pqn_act;
agents.linear_act + ops.pqn_loss_fwd_bwd + autograd), which is the yardstick of the fused calls.
The parents' own switches still select torch underneath: pqn.FUSED_PQN = False is torch's
layer_norm / argmax / mse_loss / optim.RAdam, lstm.FUSED_LSTM = False the per-step nn.LSTM loop
(either one off also turns this module's fused calls off: they contain both halves).

Declared differences from the script: those of pqn.py and lstm.py (no envpool / ALE: --backend
Synthetic; `architecture` / `obs_mode` pick the trunk: "PQN_LSTM_OBJ", the default, is PQNetwork's
object-vector trunk, "PQN_LSTM" the script's pixel trunk whose LayerNorms over [C, H, W] stay on
torch; exploration is ocppo_epsilon_greedy's law; one GPU; a single LSTM layer).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import lstm as lstm_mod
from . import ops
from . import pqn as pqn_mod
from .agents import EnvSpec, Predictor, layer_init
from .args import learner_args, single_gpu_sizes
from .lstm import LSTMTrainer, Recurrence, epoch_indices, init_lstm  # noqa: F401  (re-exported)
from .pqn import PQNTrainer, linear_schedule  # noqa: F401  (re-exported)
from .trainer import learner_main, run

# This module's two fused calls (ops.pqn_lstm_act, ops.pqn_head_loss_fwd_bwd); False: the
# composition of the parents' kernels.
FUSED_PQN_LSTM = True
# the rollout step and the bootstrap as one launch each (ops.pqn_lstm_act)
FUSED_PQN_LSTM_ACT = True
# the update's Q head + MSE loss + head backward as one call (ops.pqn_head_loss_fwd_bwd)
FUSED_PQN_LSTM_LOSS = True

ARCHITECTURES = ("PQN_LSTM_OBJ", "PQN_LSTM")

# pqn_atari_envpool_lstm.py:20-74: pqn_atari_envpool.py's fields, names and order, with the
# script's own name and its gradient clip
_REFERENCE_DEFAULTS = {"exp_name": "pqn_atari_envpool_lstm", "max_grad_norm": 0.5}
_REFERENCE_FIELDS = [(n, t, _REFERENCE_DEFAULTS.get(n, d)) for n, t, d in pqn_mod.REFERENCE_FIELDS]
# [oc_cleanrl_amd] additions, as pqn.py's, and the LSTM width
_OWN_DEFAULTS = dict(pqn_mod.OWN_DEFAULTS, architecture="PQN_LSTM_OBJ")
_OWN_FIELDS = [("lstm_hidden", int, 128)]  # nn.LSTM(512, 128) at :135

PQNLSTMArgs = learner_args(
    "PQNLSTMArgs", "The flags of pqn_atari_envpool_lstm.py:20-74 (same names, order and "
                   "defaults) + this build's additions.",
    _REFERENCE_FIELDS, pqn_mod.SKIP, _OWN_DEFAULTS, _OWN_FIELDS, pqn_mod.FIXED)


def finalize(args, world_size: int = 1):
    """Derived sizes (pqn_atari_envpool_lstm.py:175-177), the script's assertion at :304 and the
    checks of pqn.finalize / lstm.finalize that apply."""
    if args.architecture not in ARCHITECTURES:
        raise NotImplementedError(f"architecture must be one of {ARCHITECTURES}")
    if (args.obs_mode == "obj") != (args.architecture == "PQN_LSTM_OBJ"):
        raise ValueError('architecture PQN_LSTM_OBJ reads --obs_mode obj, PQN_LSTM reads pixels '
                         '(dqn)')
    if args.num_minibatches < 1 or args.num_envs % args.num_minibatches:
        raise ValueError(f"num_envs={args.num_envs} must be divisible by num_minibatches="
                         f"{args.num_minibatches}: a minibatch is whole environments")
    single_gpu_sizes(args, world_size, "the recurrent PQN learner")
    if not ops.lstm_shape_ok(args.num_steps, args.num_envs // args.num_minibatches, 1,
                             args.lstm_hidden):
        raise ValueError(f"lstm_hidden={args.lstm_hidden} with num_steps={args.num_steps}: the "
                         f"LSTM kernels take a hidden size in {ops.LSTM_HIDDEN} and >= 1 step")
    if not args.exploration_fraction * args.total_timesteps > 0:
        raise ValueError("exploration_fraction * total_timesteps (the schedule's duration) must "
                         "be positive")
    return args


class PQNLSTMNetwork(Predictor, Recurrence):
    """QNetwork of pqn_atari_envpool_lstm.py:117-165 with its state-dict keys (network.*, lstm.*,
    q_func.*), modules made and initialised in the script's order. architecture "PQN_LSTM": the
    script's pixel trunk; "PQN_LSTM_OBJ": PQNetwork's object-vector trunk (both pqn.trunk_layers).
    The recurrence is lstm.Recurrence's (ops.lstm_seq / ops.lstm_step under lstm.lstm_ok, else the
    script's per-step nn.LSTM loop)."""

    # as PQNetwork: no policy / value head pair for PPOTrainer, autograd accumulates into the
    # flat gradient buffer
    actor = critic = None
    grads_in_place = False

    def __init__(self, envs, architecture: str = "PQN_LSTM_OBJ", lstm_hidden: int = 128,
                 device=None, encoder_dims=(128, 64), decoder_dims=(128,)):
        super().__init__()
        if architecture not in ARCHITECTURES:
            raise NotImplementedError(architecture)
        self.device = device
        self.pixels = architecture == "PQN_LSTM"
        layers, d = pqn_mod.trunk_layers(envs, self.pixels, encoder_dims, decoder_dims)
        self.network = nn.Sequential(*layers)
        self.lstm = init_lstm(nn.LSTM(d, lstm_hidden))  # :135-140
        self.q_func = layer_init(nn.Linear(lstm_hidden, envs.action_space.n))  # :141

    @property
    def q_lin(self) -> nn.Linear:
        return self.q_func

    def trunk(self, x, prescaled: bool = False):
        """The LSTM's input [rows, d] (pixels are divided by 255 here, :144)."""
        if self.pixels and not prescaled:
            x = x / 255.0
        return pqn_mod.run_trunk(list(self.network), x)

    def q_head(self, hidden):
        """Q values [rows, A] of the recurrence's output."""
        return pqn_mod.q_head(self.q_func, hidden)

    def forward(self, x, lstm_state, done):
        """(q [rows, A], lstm_state) as :163-165."""
        hidden, lstm_state = self.get_states(x, lstm_state, done)
        return self.q_head(hidden), lstm_state

    def predict(self, x, states=None, **_):
        raise NotImplementedError("a recurrent network needs its state: use forward")


class PQNLSTMTrainer(LSTMTrainer, PQNTrainer):
    """LSTMTrainer's carried state, initial-state snapshot and environment-wise minibatches under
    PQNTrainer's acting, Q(lambda) targets, loss and RAdam (cooperatively: see the module text),
    with the rollout step / bootstrap and the update's head + loss as this module's fused calls."""

    def __init__(self, args, device, *a, **k):
        super().__init__(args, device, *a, **k)
        f32, dev, ag = torch.float32, self.dev, self.agent
        H = ag.lstm.hidden_size
        both = FUSED_PQN_LSTM and self.fused and lstm_mod.FUSED_LSTM
        self.fused_act = bool(both and FUSED_PQN_LSTM_ACT and ops.pqn_lstm_act_ok(
            torch.empty((self.N, ag.lstm.input_size), dtype=f32, device=dev), self.lstm_h,
            ag.q_func.weight))
        self.fused_loss = bool(both and FUSED_PQN_LSTM_LOSS and ops.pqn_head_loss_ok(
            torch.empty((self.M, H), dtype=f32, device=dev), ag.q_func.weight))
        # the bootstrap's greedy value (and, on the composed path, its unused action draw)
        self.boot_values = torch.zeros(self.N, dtype=f32, device=dev)
        self.boot_actions = torch.zeros(self.N, dtype=torch.int64, device=dev)
        self.dh = torch.zeros((self.M, H), dtype=f32, device=dev)
        self.hl_ws = ops.HeadLossWorkspace(self.M, H, self.A, dev) if self.fused_loss else None

    def _make_agent(self) -> nn.Module:
        a = self.args
        return PQNLSTMNetwork(EnvSpec(self.obs_shape, self.A), a.architecture, a.lstm_hidden, None,
                              a.encoder_dims, a.decoder_dims)

    def _sched(self):
        a = self.args
        return (self.seed, self.eps_step, a.start_e, a.end_e, self.eps_duration)

    def _lstm_weights(self):
        m = self.agent.lstm
        return (m.weight_ih_l0, m.bias_ih_l0, m.weight_hh_l0, m.bias_hh_l0)

    # ---- rollout ---------------------------------------------------------------------------
    def _act(self, t: int, env_step: bool = False, hidden=None) -> bool:
        """Step t (:252-267): dones[t] = next_done masks the carried state, values[t] = the
        greedy Q, actions[t] = the epsilon-greedy choice at global step eps_step + (t + 1) N."""
        if not self.fused_act:
            return super()._act(t, env_step)  # lstm_step, then pqn_act on the new h
        x = self._policy_hidden(t)
        q = self.agent.q_func
        self.timer.bracket("pqn_lstm_act", lambda: ops.pqn_lstm_act(
            x, *self._lstm_weights(), self.dones[t], self.lstm_h, self.lstm_c, q.weight, q.bias,
            *self._sched(), self.actions[t], self.values[t], self.epsilon,
            step_offset=(t + 1) * self.N))
        return False

    def _rollout_end(self):
        """max_a Q(next_obs, next_lstm_state, next_done) with the returned state dropped (:287),
        the Q(lambda) targets (:283-296), then the minibatches' rows."""
        a, T, ag = self.args, self.T, self.agent
        x = self._policy_hidden(T)
        q = ag.q_func
        if self.fused_act:
            self.timer.bracket("pqn_lstm_act", lambda: ops.pqn_lstm_act(
                x, *self._lstm_weights(), self.dones[T], self.lstm_h, self.lstm_c, q.weight,
                q.bias, *self._sched(), None, self.boot_values, None, q_out=self.next_q,
                commit=False))
        else:
            self.boot_h.copy_(self.lstm_h)
            self.boot_c.copy_(self.lstm_c)
            h = ag.step_(x, self.dones[T], self.boot_h, self.boot_c)
            if self.fused and ops.pqn_act_ok(h, q.weight):
                # the head as the acting kernel computes it (its q_out; the draw is not used), so
                # the targets are the same bits whichever way the rollout ran
                self.timer.bracket("pqn_act", lambda: ops.pqn_act(
                    h, q.weight, q.bias, *self._sched(), self.boot_actions, self.boot_values,
                    None, q_out=self.next_q))
            else:
                self.next_q.copy_(ag.q_head(h))
        self.timer.bracket("q_lambda", lambda: ops.q_lambda(
            self.rewards, self.values[:T], self.dones[:T], self.next_q, self.dones[T], a.gamma,
            a.q_lambda, self.returns))
        self._prepare_minibatches()

    # ---- update ----------------------------------------------------------------------------
    def _forward_backward_body(self, j: int):
        """Minibatch j (:318-329): trunk -> recurrence from the minibatch's initial state -> Q
        head -> MSE on the taken action -> backward."""
        if not self.fused_loss:
            return super()._forward_backward_body(j)
        mb, q = self.mb, self.agent.q_func
        hidden = self._minibatch_hidden(j)
        sl = slice(j * self.M, (j + 1) * self.M)
        self.grad_buf.zero_()  # optimizer.zero_grad(): autograd accumulates into the flat buffer
        hd = hidden.detach()
        # the head's gradients go straight to its views of the flat gradient buffer
        self.timer.bracket("pqn_head_loss", lambda: ops.pqn_head_loss_fwd_bwd(
            hd, q.weight, q.bias, mb["actions"][sl], mb["returns"][sl], self.dh, q.weight.grad,
            q.bias.grad, self.qstats[j], self.hl_ws))
        torch.autograd.backward(hidden, self.dh)


def run_pqn_lstm(args, device=None) -> PQNLSTMTrainer:
    return run(args, device, trainer_cls=PQNLSTMTrainer)


def main(argv=None):
    return learner_main(PQNLSTMArgs, finalize, run_pqn_lstm,
                        "oc_cleanrl_amd recurrent PQN (pqn_atari_envpool_lstm.py surface)", argv)


if __name__ == "__main__":
    main()
