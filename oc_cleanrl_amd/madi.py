"""`python -m oc_cleanrl_amd.madi [ppo_atari_madi.py flags]` — MaDi (cleanrl/ppo_atari_madi.py):
PPO on pixels behind a small convolutional masker that learns which pixels to show the agent, on
the device rollout of `trainer.PPOTrainer`.

The masker (architectures/madi.py MaskerNet) runs on every frame of a stack on its own:
x / 255 -> Conv3x3(1 -> F) -> ReLU -> Conv3x3(F -> F) -> ReLU -> Conv3x3(F -> 1) -> Sigmoid, and
the agent (PPODefault without NormalizeImg) sees x * mask on the 0-255 scale. Restated here:
  * rollout step t: ops.madi_mask on the u8 stacks of slot t -> the NatureCNN trunk -> the policy
    head launch; the update: ops.madi_mask on b_obs through the minibatch permutation (no f32
    gather of raw stacks), its six parameter gradients by ops.madi_mask_bwd, which recomputes the
    activations per tile (`_MaskFn`);
  * two optimizers as in the script (:378-379, :542-545): the agent's FlatAdam (annealed lr, eps
    1e-5) and the masker's (masker_lr, not annealed, betas (masker_beta, 0.999), eps 1e-8), each
    clipped by its own global norm, both steps inside the captured update graph;
  * the bootstrap value reads the unmasked observation, as the script does (:470).
`FUSED_MADI = False`, a masker outside ops.madi_ok (num_layers != 3, filters not 16 / 32) or CPU
tensors run the torch modules in the same loop; so does any call of more than
ops.MADI_MAX_STACKS stacks, and the update when ops.MADI_FUSED_UPDATE is off.

Declared differences from the script: no ALE here (--backend Synthetic, the package's device
envs); the rollout stores u8 stacks (exact for pixels) where the script stores f32;
`--mask-bootstrap` masks the bootstrap observation too (off: the script's behaviour); the final
evaluation is evals.evaluate on EvalAgent; one GPU.
"""
from __future__ import annotations

from dataclasses import asdict
from pathlib import Path
from typing import Optional

import torch
import torch.nn as nn

from . import ops
from .agents import EnvSpec, NormalizeImg, PPODefault
from .args import CORE_FIXED, CORE_SKIP, check_sampling_noise, learner_args, single_gpu_sizes
from .trainer import PPOTrainer, _own_tensors, learner_main, run

# The fused masker forward / backward (ops.madi_mask, ops.madi_mask_bwd) where ops.madi_ok takes
# the shapes; False: the torch modules
FUSED_MADI = True

# ppo_atari_madi.py:65-193, same names, order and defaults (backend: see the module docstring)
_REFERENCE_FIELDS = [
    ("exp_name", str, "MaDi"), ("seed", int, 42), ("torch_deterministic", bool, True),
    ("cuda", bool, True), ("env_id", str, "ALE/Pong-v5"), ("obs_mode", str, "dqn"),
    ("buffer_window_size", int, 4), ("backend", str, "Synthetic"), ("modifs", str, ""),
    ("new_rf", str, ""), ("frameskip", int, 4), ("track", bool, False),
    ("wandb_project_name", str, "MaskedDQN"), ("wandb_entity", str, "AIML_OC"),
    ("wandb_dir", Optional[str], None), ("capture_video", bool, False), ("ckpt", str, ""),
    ("logging_level", int, 40), ("author", str, "CD"), ("checkpoint_interval", int, 40),
    ("architecture", str, "MaDi"), ("total_timesteps", int, 10_000_000),
    ("learning_rate", float, 2.5e-4), ("num_envs", int, 10), ("num_steps", int, 128),
    ("anneal_lr", bool, True), ("gamma", float, 0.99), ("gae_lambda", float, 0.95),
    ("num_minibatches", int, 4), ("update_epochs", int, 4), ("norm_adv", bool, True),
    ("clip_coef", float, 0.1), ("clip_vloss", bool, True), ("ent_coef", float, 0.01),
    ("vf_coef", float, 0.5), ("max_grad_norm", float, 0.5), ("target_kl", Optional[float], None),
    ("emb_dim", int, 128), ("num_heads", int, 64), ("num_blocks", int, 1), ("patch_size", int, 12),
    ("masker_lr", float, 1e-3), ("masker_beta", float, 0.9), ("masker_num_layers", int, 3),
    ("masker_num_filters", int, 32), ("encoder_dims", tuple, (256, 512, 1024, 512)),
    ("decoder_dims", tuple, (512,)), ("test_modifs", str, ""),
    ("detection_failure_probability", float, 0.0), ("mislabeling_probability", float, 0.0),
    ("noise_std", float, 0.0), ("batch_size", int, 0), ("minibatch_size", int, 0),
    ("num_iterations", int, 0), ("masked_wrapper", Optional[str], None),
    ("add_pixels", bool, False),
]

MaDiArgs = learner_args(
    "MaDiArgs", "The flags of ppo_atari_madi.py:65-193 (same names, order and defaults) + this "
                "build's additions.",
    _REFERENCE_FIELDS, CORE_SKIP, fixed=CORE_FIXED,
    own_fields=[("mask_bootstrap", bool, False)])  # mask the bootstrap observation too


def finalize(args, world_size: int = 1):
    """Derived sizes (ppo_atari_madi.py:309-311) and the checks of args.finalize that apply."""
    if args.architecture != "MaDi":  # the script raises the same (:375-376)
        raise NotImplementedError(f"Architecture {args.architecture} does not exist!")
    if args.obs_mode != "dqn":
        raise ValueError('the MaDi learner reads pixels: --obs_mode dqn')
    if not args.fused_optimizer:
        raise NotImplementedError("the MaDi learner steps both networks with ops.FlatAdam "
                                  "(fused_optimizer)")
    if args.masker_num_layers < 1 or args.masker_num_filters < 1:
        raise ValueError("masker_num_layers and masker_num_filters must be >= 1")
    check_sampling_noise(args)
    single_gpu_sizes(args, world_size, "the MaDi learner")
    if args.minibatch_size < 1 or args.batch_size % args.num_minibatches:
        raise ValueError(f"batch size {args.batch_size} must be divisible by num_minibatches="
                         f"{args.num_minibatches}")
    return args


def weight_init(m):
    """architectures/madi.py:35-49: orthogonal Linear; delta-orthogonal Conv2d (every tap zero
    but the centre, which is orthogonal with gain sqrt(2)); zero biases."""
    if isinstance(m, nn.Linear):
        nn.init.orthogonal_(m.weight.data)
        if hasattr(m.bias, "data"):
            m.bias.data.fill_(0.0)
    elif isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
        assert m.weight.size(2) == m.weight.size(3)
        m.weight.data.fill_(0.0)
        if hasattr(m.bias, "data"):
            m.bias.data.fill_(0.0)
        mid = m.weight.size(2) // 2
        gain = nn.init.calculate_gain("relu")
        nn.init.orthogonal_(m.weight.data[:, :, mid, mid], gain)


def masker_torch(x, weights):
    """MaskerNet.forward in torch ops on f32 stacks x [B, W, H, H] for three layers' tensors
    (w1, b1, w2, b2, w3, b3)."""
    w1, b1, w2, b2, w3, b3 = weights
    H = x.shape[-1]
    h = x.reshape(-1, 1, H, H) / 255.0
    h = torch.relu(nn.functional.conv2d(h, w1, b1, padding=1))
    h = torch.relu(nn.functional.conv2d(h, w2, b2, padding=1))
    m = torch.sigmoid(nn.functional.conv2d(h, w3, b3, padding=1))
    return x * m.view(x.shape)


class _MaskFn(torch.autograd.Function):
    """masked stacks [B, W, H, H] f32 of src[idx] (idx None: all rows) with the gradients of the
    six masker tensors. fused: ops.madi_mask / ops.madi_mask_bwd (the activations are recomputed
    in the backward: nothing of size frames x F x H x H is kept); else torch ops, differentiated
    by a nested autograd pass."""

    @staticmethod
    def forward(ctx, src, idx, fused, channels_last, workspace, *weights):
        ctx.fused, ctx.idx, ctx.src, ctx.workspace = fused, idx, src, workspace
        fmt = torch.channels_last if channels_last else torch.contiguous_format
        ctx.fmt = fmt
        w = tuple(t.detach() for t in weights)
        if fused:
            ctx.w = w
            return ops.timed("madi_mask", lambda: ops.madi_mask(src, idx, w,
                                                                channels_last=channels_last))
        x = (src if idx is None else src.index_select(0, idx)).to(torch.float32)
        with torch.enable_grad():
            ctx.w = tuple(t.requires_grad_() for t in w)
            ctx.y = masker_torch(x, ctx.w)
        return ctx.y.detach().contiguous(memory_format=fmt)

    @staticmethod
    def backward(ctx, g):
        if ctx.fused:
            g = g.contiguous(memory_format=ctx.fmt)
            grads = ops.timed("madi_mask_bwd", lambda: ops.madi_mask_bwd(
                ctx.src, ctx.idx, ctx.w, g, workspace=ctx.workspace))
        else:
            grads = torch.autograd.grad(ctx.y, ctx.w, g)
        return (None, None, None, None, None, *grads)


def _stacks(src, idx) -> int:
    return src.shape[0] if idx is None else idx.numel()


def _differentiated(weights) -> bool:
    return torch.is_grad_enabled() and any(w.requires_grad for w in weights)


def masked_stacks(src, idx, weights, fused: bool = True, channels_last: bool = False,
                  workspace=None):
    """The masker on src[idx]: the fused kernels where `fused` and ops.madi_ok hold, else torch
    ops (same values up to rounding, same gradients)."""
    fused = bool(fused and ops.madi_ok(src, weights, stacks=_stacks(src, idx),
                                       backward=_differentiated(weights)))
    return _MaskFn.apply(src, idx, fused, channels_last, workspace, *weights)


class MaskerNet(nn.Module):
    """architectures/madi.py:6-33 with its state-dict keys (layers.1.*, layers.3.*, ...) and its
    init, drawn from torch's generator in the same order."""

    def __init__(self, obs_shape, num_layers, num_filters):
        super().__init__()
        assert len(obs_shape) == 3
        self.img_size = obs_shape[-1]
        self.num_layers, self.num_filters = num_layers, num_filters
        self.layers = nn.Sequential(NormalizeImg())
        for i in range(num_layers):
            in_filters = 1 if i == 0 else num_filters
            if i > 0:
                self.layers.append(nn.ReLU())
            out_filters = 1 if i == num_layers - 1 else num_filters
            self.layers.append(nn.Conv2d(in_filters, out_filters, 3, stride=1, padding=1,
                                         padding_mode="zeros"))
        self.layers.append(nn.Sigmoid())
        self.apply(weight_init)
        self.workspace = None  # the fused backward's partial rows, made at the first fused call

    def weights(self):
        """(w1, b1, w2, b2, ...) of the convolutions in order."""
        return tuple(t for m in self.layers if isinstance(m, nn.Conv2d)
                     for t in (m.weight, m.bias))

    def torch_forward(self, x):
        s = self.img_size
        return x * self.layers(x.reshape(-1, 1, s, s)).view(x.shape)

    def fused_ok(self, x) -> bool:
        w = self.weights()
        return FUSED_MADI and ops.madi_ok(x, w, self.num_layers, stacks=x.shape[0],
                                          backward=_differentiated(w))

    def forward(self, x):
        if not self.fused_ok(x):
            return self.torch_forward(x)
        if self.workspace is None or self.workspace.device != x.device:
            self.workspace = ops.madi_workspace(self.num_filters, x.device)
        return _MaskFn.apply(x, None, True, False, self.workspace, *self.weights())


class EvalAgent(nn.Module):
    """ppo_atari_madi.py:627-634: the agent behind its masker, for evals.evaluate."""

    def __init__(self, masker, agent):
        super().__init__()
        self.masker, self.agent = masker, agent

    def get_action_and_value(self, x):
        return self.agent.get_action_and_value(self.masker(x))


def masker_path(path) -> Path:
    """`<exp_name>_<tag>.cleanrl_model` -> `<exp_name>_masker_<tag>.cleanrl_model` (:613)."""
    path = Path(path)
    head, _, tag = path.stem.rpartition("_")
    return path.with_name(f"{head}_masker_{tag}{path.suffix}")


class MaDiTrainer(PPOTrainer):
    """PPOTrainer's rollout buffer, staging, flat buffers and graphs with the masker in front of
    the agent and an optimizer of its own."""

    def __init__(self, args, device, *a, **k):
        self.masker = None
        super().__init__(args, device, *a, **k)
        if self.world != 1 or self.dp:
            raise NotImplementedError("the MaDi learner runs on one GPU")
        if not self.pixels or len(self.obs_shape) != 3:
            raise ValueError("the MaDi learner needs pixel stacks [W, H, H]")
        ar, dev = args, self.dev
        self.masker = self.masker.to(dev)
        # masker_optimizer (:379): lr masker_lr (not annealed), eps torch's default, own clip
        self.masker_opt = ops.FlatAdam(self.masker.parameters(), lr=ar.masker_lr,
                                       betas=(ar.masker_beta, 0.999), eps=1e-8,
                                       max_grad_norm=ar.max_grad_norm)
        self.masker_weights = self.masker.weights()
        # the rollout's forward and the update's forward + backward are routed apart (ops.madi_ok)
        ok = lambda n, bwd: bool(FUSED_MADI and ops.madi_ok(  # noqa: E731
            self.obs[0], self.masker_weights, ar.masker_num_layers, stacks=n, backward=bwd))
        self.fused_rollout, self.fused_update = ok(self.N, False), ok(self.M, True)
        self.madi_ws = (ops.madi_workspace(ar.masker_num_filters, dev) if self.fused_update
                        else None)
        self.masked_roll = (torch.empty((self.N,) + self.obs_shape, dtype=torch.float32,
                                        device=dev, memory_format=self.net_format).zero_()
                            if self.fused_rollout else None)
        self.mb_obs = None  # PPOTrainer's f32 minibatch gather: the masker reads b_obs itself

    def _make_agent(self) -> nn.Module:
        """Agent, then masker, from the generator in the script's order (:371-374)."""
        a = self.args
        agent = PPODefault(EnvSpec(self.obs_shape, self.A), None, normalize=False)
        self.masker = MaskerNet(self.obs_shape, a.masker_num_layers, a.masker_num_filters)
        return agent

    # ---- the masker in front of the trunk -----------------------------------------------------
    def _masked_rollout(self, t: int):
        """masker(obs[t]) for the rollout (no autograd), in the trunk's layout."""
        if self.fused_rollout:
            self.timer.bracket("madi_mask_rollout", lambda: ops.madi_mask(
                self.obs[t], None, tuple(w.detach() for w in self.masker_weights),
                out=self.masked_roll))
            return self.masked_roll
        # net_obs holds slot t's stacks in f32 when step t acts
        return self.masker.torch_forward(self.net_obs).contiguous(memory_format=self.net_format)

    def _policy_hidden(self, t: int):
        return self.agent.trunk(self._masked_rollout(t), False)

    def _bootstrap_value(self):
        """agent.get_value(next_obs) on the unmasked observation (:470); --mask-bootstrap: on
        the masked one."""
        if self.args.mask_bootstrap:
            return self.agent._head(self.agent.critic, self._policy_hidden(self.T))
        return self.agent.get_value(self.net_obs, False)

    def _minibatch_hidden(self, j: int):
        idx = self.perm_dev[j * self.M:(j + 1) * self.M]
        self.masker_opt.grads.zero_()  # masker_optimizer.zero_grad() (:540)
        masked = _MaskFn.apply(self.b_obs, idx, self.fused_update, self.channels_last, self.madi_ws,
                               *self.masker_weights)
        return self.agent.trunk(masked, False)

    def _opt_step(self):
        super()._opt_step()
        self.timer.bracket("masker_adam", self.masker_opt.step)

    # ---- checkpoints --------------------------------------------------------------------------
    def masker_checkpoint(self) -> dict:
        return {"model_weights": _own_tensors(self.masker.state_dict()),
                "args": asdict(self.args)}

    def save(self, path):
        """The agent's file as PPOTrainer writes it and the masker's beside it (:607-616)."""
        super().save(path)
        torch.save(self.masker_checkpoint(), masker_path(path))

    def final_extras(self, run_dir, exp_name: str):
        torch.save(self.masker_checkpoint(),
                   Path(run_dir) / f"{exp_name}_masker_final.cleanrl_model")


def _image_size(features: int) -> int:
    """The square input edge whose NatureCNN output (64 channels after 8/4, 4/2 and 3/1
    convolutions) has `features` elements; 84 where it fits, else the smallest."""
    def feats(h):
        h = ((h - 8) // 4 + 1 - 4) // 2 + 1 - 2
        return 64 * h * h if h > 0 else 0

    for h in (84, *range(36, 4096)):
        if feats(h) == features:
            return h
    raise ValueError(f"no square input gives {features} NatureCNN features")


def load_eval_agent(agent_file, masker_file, device, img_size=None) -> EvalAgent:
    """EvalAgent from the two checkpoint files of a run. img_size: the frames' edge (None: from
    the agent's first Linear, several edges can share a feature count: 84 is preferred)."""
    ck, mk = (torch.load(f, map_location=device, weights_only=False)
              for f in (agent_file, masker_file))
    a = mk["args"]
    w1 = ck["model_weights"]["network.0.weight"]
    H = img_size or _image_size(ck["model_weights"]["network.7.weight"].shape[1])
    obs_shape = (w1.shape[1], H, H)
    n_actions = ck["model_weights"]["actor.weight"].shape[0]
    agent = PPODefault(EnvSpec(obs_shape, n_actions), None, normalize=False)
    agent.load_state_dict(ck["model_weights"])
    masker = MaskerNet(obs_shape, a["masker_num_layers"], a["masker_num_filters"])
    masker.load_state_dict(mk["model_weights"])
    return EvalAgent(masker.to(device), agent.to(device))


def run_madi(args, device=None) -> MaDiTrainer:
    return run(args, device, trainer_cls=MaDiTrainer)


def main(argv=None):
    return learner_main(MaDiArgs, finalize, run_madi,
                        "oc_cleanrl_amd MaDi (ppo_atari_madi.py surface)", argv)


if __name__ == "__main__":
    main()
