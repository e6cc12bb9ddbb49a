"""`python -m oc_cleanrl_amd.vit [ppo_atari_vit.py flags]` — the pixel vision-transformer PPO agent
of cleanrl/ppo_atari_vit.py (the `VIT` choice of architectures/transformer.py) on HBM-resident
state.

The script's loop is ppo_atari_oc.py's, so `ViTTrainer` is `trainer.PPOTrainer` with another
agent: `network = nn.Sequential(SimpleViT(...), nn.Flatten())` on the raw 0-255 frame stacks, then
the usual actor and critic heads. `vit_pytorch` is not a dependency of this package: `SimpleViT`
is RESTATED here in plain torch.nn, as the release with the LayerNorms inside the patch embedding
and a bare Linear head (same submodule names, so the same state-dict keys; same construction
order of the Linears, so the same seeded init; dim_head = 64, mlp_dim = emb_dim, exact GELU, the
2-D sincos `pos_embedding` a plain tensor attribute outside the state dict).

The fused path (`FUSED_VIT`, `ViTAgent.fused_ok`) reads the rollout's u8 stacks through the row
indices: ops.vit_patch_ln (patchify + the first LayerNorm, csrc/ocppo_vit_patch.hip), the Linears
on agents.linear_act, the pre-norm LayerNorms on ops.ln_relu(relu=False) (the last LayerNorm on
torch's: FINAL_NORM_HIP), the attention core on
ops.vit_attn (csrc/ocppo_vit_attn.hip, f32 MFMA), the feed-forward half of a block (LayerNorm,
Linear, exact GELU, Linear, residual add) on ops.vit_ffn (`FUSED_FFN`, csrc/ocppo_vit_ffn.hip, f32
MFMA; outside ops.vit_ffn_ok: ops.ln_relu, linear_act and torch's GELU and add); the attention
half of a block (LayerNorm, to_qkv, the attention core, to_out, residual add) on ops.vit_attn_block
(`FUSED_ATTN`, csrc/ocppo_vit_attn_block.hip, f32 MFMA) at the sample counts ops.vit_attn_block_routed
names; the positional add and the token mean are torch ops. Outside that routing (the default: the
routed range is empty) or ops.vit_attn_block_ok the attention half is a chain:
ops.ln_relu, to_qkv, ops.vit_attn, to_out and torch's add, where the two bias-free Linears run
ops.linear_act in the rollout and F.linear under autograd (agents._LinearAct's update GEMM routes
take a bias). Shapes outside either kernel contract (e.g. patch_size 6) and `FUSED_VIT = False` run
the same modules in plain torch.

Declared differences from the script: `--backend Synthetic` (no ALE here) and `obs_mode dqn`, this
package's name for the 84 x 84 x buffer_window_size u8 stacks. `SimpleViT2` and `MobileViT` are out
of scope.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import agents, ops
from .agents import EnvSpec, _ActorCritic, layer_init, linear_act
from .args import CORE_FIXED, CORE_SKIP, check_sampling_noise, learner_args, single_gpu_sizes
from .trainer import PPOTrainer, learner_main, run

# The fused path (ops.vit_patch_ln / ops.vit_attn / ops.ln_relu / linear_act); False: plain torch
FUSED_VIT = True

# The fused path's last LayerNorm (transformer.norm) on ops.ln_relu too. Off: its rows feed the
# token mean, so its bias gradient is a sum of T identical rows per sample, which ops.ln_relu's
# backward adds up in row order; at B = 3, T = 49, dim = 32 that sum sits 2.5e-6 of the largest
# element from the float64 result where torch's pairwise sum sits 6.6e-7, outside
# the project's error rule. The two pre-norms of every block and the patch embedding's norm, whose
# gradient rows differ, stay on ops.ln_relu.
FINAL_NORM_HIP = False

# The feed-forward half of every block (pre-norm LayerNorm, Linear, GELU, Linear and the residual
# add) as ops.vit_ffn: one launch forward, two backward (csrc/ocppo_vit_ffn.hip). A FeedForward
# outside ops.vit_ffn_ok (e.g. mlp_dim 256), a row count outside ops.vit_ffn_routed (the 490-row
# rollout step: measured slower fused) and False run the chain of launches below it.
FUSED_FFN = True

# The attention half of every block (pre-norm LayerNorm, to_qkv, softmax attention, to_out and the
# residual add) as ops.vit_attn_block: one launch forward, three backward
# (csrc/ocppo_vit_attn_block.hip). An Attention outside ops.vit_attn_block_ok, a sample count
# outside ops.vit_attn_block_routed and False run the chain of launches below it.
FUSED_ATTN = True

DIM_HEAD = 64  # vit_pytorch's default, which the script does not override

# ppo_atari_vit.py:45-141, same names, order and defaults (backend / obs_mode: declared differences)
_REFERENCE_FIELDS = [
    ("exp_name", str, "ppo_atari_vit"), ("seed", int, 42), ("torch_deterministic", bool, True),
    ("cuda", bool, True), ("env_id", str, "ALE/Pong-v5"), ("obs_mode", str, "dqn"),
    ("feature_func", str, "xywh"), ("buffer_window_size", int, 4), ("backend", str, "Synthetic"),
    ("modifs", str, ""), ("new_rf", str, ""), ("frameskip", int, -1), ("track", bool, True),
    ("wandb_project_name", str, "OCRL_Transformer"), ("wandb_entity", Optional[str], None),
    ("wandb_dir", Optional[str], None), ("capture_video", bool, True), ("ckpt", str, ""),
    ("logging_level", int, 40), ("total_timesteps", int, 10_000_000),
    ("learning_rate", float, 2.5e-4), ("num_envs", int, 10), ("num_steps", int, 128),
    ("anneal_lr", bool, True), ("gamma", float, 0.99), ("gae_lambda", float, 0.95),
    ("num_minibatches", int, 4), ("update_epochs", int, 4), ("norm_adv", bool, True),
    ("clip_coef", float, 0.1), ("clip_vloss", bool, True), ("ent_coef", float, 0.01),
    ("vf_coef", float, 0.5), ("max_grad_norm", float, 0.5), ("target_kl", Optional[float], None),
    ("emb_dim", int, 128), ("num_heads", int, 8), ("num_blocks", int, 4), ("patch_size", int, 12),
    ("batch_size", int, 0), ("minibatch_size", int, 0), ("num_iterations", int, 0),
]
_ON_THE_COMMAND_LINE = {"emb_dim", "num_heads", "num_blocks", "patch_size"}
_SKIP = CORE_SKIP - _ON_THE_COMMAND_LINE | {"architecture", "encoder_dims", "decoder_dims"}
_FIXED = tuple((n, v) for n, v in CORE_FIXED if n not in _ON_THE_COMMAND_LINE) + (
    ("encoder_dims", ()), ("decoder_dims", ()), ("architecture", "VIT"))

ViTArgs = learner_args(
    "ViTArgs", "The flags of ppo_atari_vit.py:45-141 (same names and defaults) + this build's "
               "additions.", _REFERENCE_FIELDS, _SKIP, fixed=_FIXED)


def finalize(args, world_size: int = 1):
    """Derived sizes (ppo_atari_vit.py's batch_size / minibatch_size / num_iterations) + the checks
    of args.finalize that apply."""
    if args.obs_mode != "dqn":
        raise ValueError("the ViT agent reads pixel stacks: --obs_mode dqn")
    if args.emb_dim % 4:
        raise ValueError("emb_dim must be a multiple of 4 (the 2-D sincos embedding)")
    if args.patch_size < 1 or 84 % args.patch_size:
        raise ValueError("patch_size must divide the 84 x 84 frame")
    check_sampling_noise(args)
    single_gpu_sizes(args, world_size, "the ViT learner")
    if args.minibatch_size < 1 or args.batch_size % args.num_minibatches:
        raise ValueError("batch size must be divisible by num_minibatches")
    return args


def posemb_sincos_2d(h: int, w: int, dim: int, temperature: int = 10000):
    """vit_pytorch.simple_vit.posemb_sincos_2d: [h * w, dim] f32."""
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    if dim % 4:
        raise ValueError("feature dimension must be multiple of 4 for sincos emb")
    omega = torch.arange(dim // 4) / (dim // 4 - 1)
    omega = 1.0 / (temperature ** omega)
    y = y.flatten()[:, None] * omega[None, :]
    x = x.flatten()[:, None] * omega[None, :]
    return torch.cat((x.sin(), x.cos(), y.sin(), y.cos()), dim=1).to(torch.float32)


class Patchify(nn.Module):
    """Rearrange('b c (h p1) (w p2) -> b (h w) (p1 p2 c)') without einops."""

    def __init__(self, patch: int):
        super().__init__()
        self.patch = patch

    def forward(self, x):
        B, C, H, W = x.shape
        p = self.patch
        x = x.reshape(B, C, H // p, p, W // p, p).permute(0, 2, 4, 3, 5, 1)
        return x.reshape(B, (H // p) * (W // p), p * p * C)


class Attention(nn.Module):
    def __init__(self, dim: int, heads: int, dim_head: int = DIM_HEAD):
        super().__init__()
        inner = dim_head * heads
        self.heads, self.scale = heads, dim_head ** -0.5
        self.norm = nn.LayerNorm(dim)
        self.to_qkv = nn.Linear(dim, inner * 3, bias=False)
        self.to_out = nn.Linear(inner, dim, bias=False)

    def forward(self, x):
        B, S, _ = x.shape
        q, k, v = (t.reshape(B, S, self.heads, -1).transpose(1, 2)
                   for t in self.to_qkv(self.norm(x)).chunk(3, dim=-1))
        attn = torch.softmax(q @ k.transpose(-1, -2) * self.scale, dim=-1)
        return self.to_out((attn @ v).transpose(1, 2).reshape(B, S, -1))


class FeedForward(nn.Module):
    def __init__(self, dim: int, hidden: int):
        super().__init__()
        self.net = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, hidden), nn.GELU(),
                                 nn.Linear(hidden, dim))

    def forward(self, x):
        return self.net(x)


class Transformer(nn.Module):
    def __init__(self, dim: int, depth: int, heads: int, dim_head: int, mlp_dim: int):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.layers = nn.ModuleList(
            nn.ModuleList([Attention(dim, heads, dim_head), FeedForward(dim, mlp_dim)])
            for _ in range(depth))

    def forward(self, x):
        for attn, ff in self.layers:
            x = attn(x) + x
            x = ff(x) + x
        return self.norm(x)


class SimpleViT(nn.Module):
    """vit_pytorch.SimpleViT restated (module docstring)."""

    def __init__(self, *, image_size: int, patch_size: int, num_classes: int, dim: int, depth: int,
                 heads: int, mlp_dim: int, channels: int = 3, dim_head: int = DIM_HEAD):
        super().__init__()
        if image_size % patch_size:
            raise ValueError("Image dimensions must be divisible by the patch size.")
        patch_dim = channels * patch_size * patch_size
        self.patch_size, self.heads = patch_size, heads
        self.to_patch_embedding = nn.Sequential(
            Patchify(patch_size), nn.LayerNorm(patch_dim), nn.Linear(patch_dim, dim),
            nn.LayerNorm(dim))
        side = image_size // patch_size
        self.pos_embedding = posemb_sincos_2d(side, side, dim)
        self.transformer = Transformer(dim, depth, heads, dim_head, mlp_dim)
        self.linear_head = nn.Linear(dim, num_classes)

    def _apply(self, fn, *a, **k):
        """pos_embedding is neither a parameter nor a buffer; it follows the module's moves."""
        super()._apply(fn, *a, **k)
        self.pos_embedding = fn(self.pos_embedding)
        return self

    def forward(self, img):
        x = self.to_patch_embedding(img)
        x = x + self.pos_embedding.to(x.device, dtype=x.dtype)
        x = self.transformer(x)
        return self.linear_head(x.mean(dim=1))


def _linear_nobias(x2, lin: nn.Linear):
    """A bias-free Linear on rows x2: the rollout's HIP Linear kernel where it applies, F.linear
    under autograd (agents._LinearAct's update routes take a bias)."""
    if agents._hip_linear_ok(x2, lin):
        return ops.linear_act(x2, lin.weight, None, False)
    return F.linear(x2, lin.weight)


def _norm(x2, ln: nn.LayerNorm):
    return ops.ln_relu(x2, ln.weight, ln.bias, ln.eps, False)


class ViTAgent(_ActorCritic):
    """The `VIT` agent of architectures/transformer.py (ppo_atari_oc.py:417-433): SimpleViT with
    num_classes = emb_dim behind nn.Flatten, actor and critic heads on it."""

    # LayerNorm / bias-free Linear gradients reach .grad through AccumulateGrad: the trainer zeroes
    # the flat gradient buffer per minibatch (PPOTrainer.direct_grads)
    grads_in_place = False

    def __init__(self, envs, emb_dim=128, num_heads=8, num_blocks=4, patch_size=12, device=None):
        super().__init__()
        self.device = device
        dims = tuple(envs.observation_space.shape)  # [C, H, H]
        self.network = nn.Sequential(
            SimpleViT(image_size=dims[-1], patch_size=patch_size, num_classes=emb_dim, dim=emb_dim,
                      depth=num_blocks, heads=num_heads, mlp_dim=emb_dim, channels=dims[0]),
            nn.Flatten())
        self.actor = layer_init(nn.Linear(emb_dim, envs.action_space.n), std=0.01)
        self.critic = layer_init(nn.Linear(emb_dim, 1), std=1)

    def fused_ok(self, src) -> bool:
        """The fused path applies to the u8 stacks src [N, C, 84, 84]: the module switch and both
        kernel contracts (ops.vit_patch_ok, ops.vit_attn_shape_ok), LayerNorm widths within
        ops.ln_relu's."""
        v = self.network[0]
        pe = v.to_patch_embedding
        dim = pe[2].out_features
        return bool(FUSED_VIT and pe[2].weight.is_cuda and ops.vit_patch_ok(src, pe[1], v.patch_size)
                    and dim <= ops.LN_RELU_MAX_E and
                    ops.vit_attn_shape_ok((ops.VIT_PATCH_H // v.patch_size) ** 2,
                                          v.heads * DIM_HEAD, v.heads))

    def trunk(self, x, prescaled: bool = False):
        """Plain torch on stacks x [B, C, H, H] holding 0-255 values (any dtype)."""
        return self.network(x.to(self.actor.weight.dtype))

    def trunk_stacks(self, src, idx):
        """trunk(src[idx]) (idx None: every row) on the fused path; fused_ok(src) must hold."""
        v = self.network[0]
        pe, heads = v.to_patch_embedding, v.heads
        y = ops.vit_patch_ln(src, idx, pe[1], v.patch_size)
        R, T, E = y.shape
        x = _norm(linear_act(y.view(R * T, E), pe[2], False), pe[3])
        D = x.shape[1]
        x = (x.view(R, T, D) + v.pos_embedding).view(R * T, D)
        for attn, ff in v.transformer.layers:
            if FUSED_ATTN and ops.vit_attn_block_routed(R) and ops.vit_attn_block_ok(x, attn, T):
                x = ops.vit_attn_block(x, attn, T)
            else:
                qkv = _linear_nobias(_norm(x, attn.norm), attn.to_qkv)
                a = ops.vit_attn(qkv.view(R, T, qkv.shape[1]), heads)
                x = _linear_nobias(a.view(R * T, -1), attn.to_out) + x
            if FUSED_FFN and ops.vit_ffn_routed(x.shape[0]) and ops.vit_ffn_ok(x, ff):
                x = ops.vit_ffn(x, ff)
                continue
            h = F.gelu(linear_act(_norm(x, ff.net[0]), ff.net[1], False))
            x = linear_act(h, ff.net[3], False) + x
        x = _norm(x, v.transformer.norm) if FINAL_NORM_HIP else v.transformer.norm(x)
        x = x.view(R, T, D).mean(dim=1)
        return linear_act(x, v.linear_head, False)

    def forward(self, x):
        return self.trunk(x)


class ViTTrainer(PPOTrainer):
    """PPOTrainer with the ViT agent; the fused path reads slot t of the u8 rollout buffer (the
    rollout) or the buffer through the minibatch's indices (the update): no f32 stack copy."""

    def __init__(self, args, device, *a, **k):
        super().__init__(args, device, *a, **k)
        if not self.pixels or len(self.obs_shape) != 3:
            raise ValueError("the ViT learner needs pixel stacks [W, H, H]")

    def _make_agent(self) -> nn.Module:
        a = self.args
        return ViTAgent(EnvSpec(self.obs_shape, self.A), a.emb_dim, a.num_heads, a.num_blocks,
                        a.patch_size)

    def _policy_hidden(self, t: int):
        if self.agent.fused_ok(self.obs[t]):
            return self.agent.trunk_stacks(self.obs[t], None)
        return self.agent.trunk(self.net_obs)  # holds slot t's stacks in f32 when step t acts

    def _bootstrap_value(self):
        return self.agent._head(self.agent.critic, self._policy_hidden(self.T))

    def _minibatch_hidden(self, j: int):
        idx = self.perm_dev[j * self.M:(j + 1) * self.M]
        if self.agent.fused_ok(self.b_obs):
            return self.agent.trunk_stacks(self.b_obs, idx)
        self.timer.bracket("gather", lambda: ops.gather_rows(self.b_obs, idx, self.mb_obs))
        return self.agent.trunk(self.mb_obs)


def run_vit(args, device=None) -> ViTTrainer:
    return run(args, device, trainer_cls=ViTTrainer)


def main(argv=None):
    return learner_main(ViTArgs, finalize, run_vit,
                        "oc_cleanrl_amd ViT PPO (ppo_atari_vit.py surface)", argv)


if __name__ == "__main__":
    main()
