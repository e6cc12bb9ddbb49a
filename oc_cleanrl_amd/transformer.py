"""`python -m oc_cleanrl_amd.transformer [ppo_atari_oc_transformer.py flags]` — the object-set
transformer PPO agent of cleanrl/ppo_atari_oc_transformer.py on HBM-resident state.

The script's loop is ppo_atari_oc.py's (VecNormalize rewards, GAE, the clipped loss,
Adam(eps=1e-5)), so `TransformerTrainer` is `trainer.PPOTrainer` with another agent. Its
`PPOAgent` (:215-277) reads an observation as a SET of objects [S, F]: a per-object Linear makes
tokens, `num_blocks` post-norm torch TransformerEncoderLayers (dim_feedforward = emb_dim, ReLU)
mix them under a key-padding mask derived from the first `num_obj` (object type) columns,
`num_post_layers` Linear+ReLU follow, a masked max / mean / first pooling gives the hidden vector
of the usual actor and critic heads.

`OCTransformerAgent` holds the same submodules (torch's own TransformerEncoderLayer /
TransformerEncoder, same construction order, so the same state-dict keys and seeded init) and
runs a block as
    in-proj -> ops.mha -> out-proj -> add + LayerNorm -> linear1+ReLU -> linear2 -> add + LayerNorm
with the four Linears on agents.linear_act (rows = B * S: x6 / hipBLASLt / the rows kernel) and
the attention core one HIP launch per direction (csrc/ocppo_attn.hip); the residual add +
LayerNorm has a HIP kernel too (ops.add_layernorm), routed to torch's ops where it measured
slower (ADD_LAYERNORM_HIP). By default that path needs `dropout == 0`: with the reference's
default dropout = 0.1 every block runs torch's own layer modules. `--dropout 0` selects the fused
path; `FUSED_ATTN = False` turns it off (tests, tools/bench_transformer.py).

`--fused-dropout` puts `dropout > 0` on the fused path too: the four dropout sites of a layer
(attention probabilities inside ops.mha; dropout1, the FFN's inner dropout and dropout2 on
ops.dropout) draw counter-based masks from the agent's own generator state `rng` = device i64
(seed, offset) -- a documented Philox stream, NOT torch's dropout stream. One
forward snapshots the state, every site of that forward and of its backward reads the snapshot,
and the forward ends by advancing the live state by one; all of it is graph-capturable. As with
torch's modules (and the reference, which never calls eval()), dropout is active iff
`self.training`.

The trainer's `(buffer_window_size, num_features)` observation is read as (S objects, F
features); `num_obj` stands in for the reference's `envs.get_attr("num_obj")`. Host envs
delivering whole object sets (OCAtari's OCWrapper) are out of scope.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn
from torch.nn import TransformerEncoder, TransformerEncoderLayer

from . import ops
from .agents import EnvSpec, _ActorCritic, layer_init, linear_act
from .args import CORE_FIXED, CORE_SKIP, learner_args, single_gpu_sizes
from .trainer import PPOTrainer, learner_main, run

# The fused block path (ops.mha / ops.add_layernorm); False: torch's layer modules everywhere.
FUSED_ATTN = True

# The fused path's residual add + LayerNorm on ops.add_layernorm. Off: measured slower than
# torch's add + layer_norm at both measured shapes (forward + backward, 2560 x 128: 38.4 us against
# 24.2; 65536 x 128: 216.7 against 185.2), so the fused path takes torch's two ops
# there and keeps the HIP attention core. The kernel stays tested (tests/test_attn_gpu.py).
ADD_LAYERNORM_HIP = False

POOLING_TYPES = ("max", "mean", "first")

# ppo_atari_oc_transformer.py:55-160, same names, order and defaults (backend / obs_mode: declared
# differences -- no ALE here, and "obj" is this package's name of the object-vector observation)
_REFERENCE_FIELDS = [
    ("exp_name", str, "ppo_atari_oc_transformer"), ("seed", int, 42),
    ("torch_deterministic", bool, True), ("cuda", bool, True),
    ("env_id", str, "ALE/Pong-v5"), ("obs_mode", str, "obj"), ("backend", str, "Synthetic"),
    ("modifs", str, ""), ("new_rf", str, ""), ("frameskip", int, -1),
    ("track", bool, True), ("wandb_project_name", str, "OCRL_Transformer"),
    ("wandb_entity", str, "AIML_OC"), ("wandb_dir", str, "../../wandb"),
    ("capture_video", bool, True), ("ckpt", str, ""), ("logging_level", int, 40),
    ("total_timesteps", int, 10_000_000), ("learning_rate", float, 2.5e-4),
    ("num_envs", int, 10), ("num_steps", int, 128), ("anneal_lr", bool, True),
    ("gamma", float, 0.99), ("gae_lambda", float, 0.95), ("num_minibatches", int, 4),
    ("update_epochs", int, 4), ("norm_adv", bool, True), ("clip_coef", float, 0.1),
    ("clip_vloss", bool, True), ("ent_coef", float, 0.01), ("vf_coef", float, 0.5),
    ("max_grad_norm", float, 0.5), ("target_kl", Optional[float], None),
    ("emb_dim", int, 128), ("num_heads", int, 8), ("num_blocks", int, 3),
    ("pooling_type", str, "max"), ("num_post_layers", int, 1), ("masking", bool, True),
    ("dropout", float, 0.1),
    ("player_name", str, "Player"), ("use_polar_coordinates", bool, False),
    ("relative_velocity", bool, True),
    ("batch_size", int, 0), ("minibatch_size", int, 0), ("num_iterations", int, 0),
]
# [oc_cleanrl_amd] additions: what PPOTrainer reads beyond the script's flags (args.Args' own
# defaults), the observation geometry, and num_obj
_OWN_DEFAULTS = {"buffer_window_size": 8,  # S: objects per observation
                 "num_features": 8}        # F: features per object
_OWN_FIELDS = [
    ("num_obj", int, 3),  # leading object-type columns (envs.get_attr("num_obj"))
    # dropout > 0 on the fused block path with counter-based masks (off: torch's layer modules)
    ("fused_dropout", bool, False)]
# Where this learner differs from args.CORE_SKIP / CORE_FIXED: the transformer's sizes are the
# script's flags, the final evaluation and the DP switches stay on its command line, and the
# network choice is fixed instead
_ON_THE_COMMAND_LINE = {"emb_dim", "num_heads", "num_blocks", "eval_episodes", "dp_overlap",
                        "dp_exchange"}
_SKIP = CORE_SKIP - _ON_THE_COMMAND_LINE | {"architecture", "encoder_dims", "decoder_dims"}
_FIXED = tuple((n, v) for n, v in CORE_FIXED if n not in _ON_THE_COMMAND_LINE) + (
    ("encoder_dims", ()), ("decoder_dims", ()), ("architecture", "OC_TRANSFORMER"))

TransformerArgs = learner_args(
    "TransformerArgs", "The flags of ppo_atari_oc_transformer.py:55-160 (same names and "
                       "defaults) + this build's additions.",
    _REFERENCE_FIELDS, _SKIP, _OWN_DEFAULTS, _OWN_FIELDS, _FIXED)


def finalize(args, world_size: int = 1):
    """Derived sizes (ppo_atari_oc_transformer.py:282-284) + the checks of args.finalize that
    apply."""
    if args.pooling_type not in POOLING_TYPES:
        raise NotImplementedError(f"pooling_type must be one of {POOLING_TYPES}")
    if args.obs_mode != "obj":
        raise ValueError('the transformer agent reads object sets: --obs_mode obj')
    single_gpu_sizes(args, world_size, "the transformer learner")
    if args.batch_size % args.num_minibatches:
        raise ValueError("batch size must be divisible by num_minibatches")
    if not 1 <= args.num_obj <= args.num_features:
        raise ValueError("num_obj must be in [1, num_features]")
    return args


def attn_shape_ok(S: int, E: int, num_heads: int, dropout: float,
                  fused_dropout: bool = False) -> bool:
    """The kernel contract (1 <= S <= 64, head dim in {8, 16, 32, 64}, E <= 512) and no dropout;
    with fused_dropout, 0 < dropout < 1 too, within the dropout kernels' contract."""
    if dropout == 0:
        return ops.mha_shape_ok(S, E, num_heads)
    return bool(fused_dropout) and 0 < dropout < 1 and ops.mha_dropout_shape_ok(S, E, num_heads)


def attn_ok(x, emb_dim: int, num_heads: int, dropout: float, fused_dropout: bool = False) -> bool:
    """The fused block path applies to the object sets x [B, S, F]: a GPU f32 contiguous input,
    attn_shape_ok for its tokens [B, S, emb_dim], and the module switch."""
    return (FUSED_ATTN and isinstance(x, torch.Tensor) and x.dim() == 3 and x.is_cuda and
            x.dtype == torch.float32 and x.is_contiguous() and x.shape[0] >= 1 and
            attn_shape_ok(x.shape[1], emb_dim, num_heads, dropout, fused_dropout))


def pool(h, mask, pooling_type: str):
    """PPOAgent's pooling (:226-244) as it is. mask [B, S] bool: mean pooling sums ALL rows and
    divides by the number of valid ones, max pooling multiplies by the mask first; mask None
    (masking off): torch.max / torch.mean / the first row."""
    if pooling_type == "first":
        return h[:, 0, :]
    if mask is None:
        return torch.max(h, dim=1)[0] if pooling_type == "max" else torch.mean(h, dim=1)
    if pooling_type == "max":
        return torch.max(h * mask.unsqueeze(-1), dim=1)[0]
    return torch.sum(h, dim=1) / torch.sum(mask, dim=1, keepdim=True)


def _add_norm(x, res, norm: nn.LayerNorm):
    """norm(x + res): ops.add_layernorm, or torch's two ops (ADD_LAYERNORM_HIP)."""
    if ADD_LAYERNORM_HIP:
        return ops.add_layernorm(x, res, norm.weight, norm.bias, norm.eps)
    return norm(x + res)


class OCTransformerAgent(_ActorCritic):
    """PPOAgent of ppo_atari_oc_transformer.py:215-277; its options are constructor arguments
    instead of the script's global `args`."""

    # LayerNorm / in-proj gradients of the torch path reach .grad through AccumulateGrad: the
    # trainer zeroes the flat gradient buffer per minibatch (PPOTrainer.direct_grads)
    grads_in_place = False

    def __init__(self, envs, emb_dim, num_heads, num_blocks, masking, num_obj, device=None,
                 pooling_type="max", num_post_layers=1, dropout=0.1, fused_dropout=False, seed=0):
        super().__init__()
        if pooling_type not in POOLING_TYPES:
            raise NotImplementedError(pooling_type)
        self.device = device
        dims = envs.observation_space.shape
        self.num_obj, self.masking, self.pooling_type = num_obj, bool(masking), pooling_type
        self.num_heads, self.dropout = num_heads, float(dropout)
        # fused_dropout: dropout > 0 on the fused path. rng = device i64 (seed, offset), made on
        # the first input's device; a plain attribute (the state-dict keys stay the reference's)
        self.fused_dropout, self.seed, self.rng = bool(fused_dropout), int(seed), None
        encoder_layer = TransformerEncoderLayer(emb_dim, num_heads, emb_dim, device=device,
                                                dropout=dropout, batch_first=True)
        self.encoder = nn.Linear(dims[1], emb_dim, device=device)
        self.transformer = TransformerEncoder(encoder_layer, num_blocks)
        self.network = nn.Sequential()
        for _ in range(num_post_layers):
            self.network.append(nn.Linear(emb_dim, emb_dim, device=device))
            self.network.append(nn.ReLU())
        self.actor = layer_init(nn.Linear(emb_dim, envs.action_space.n, device=device), std=0.01)
        self.critic = layer_init(nn.Linear(emb_dim, 1, device=device), std=1)

    def valid_mask(self, x):
        """:258 -- an object is present when any of its type columns is set."""
        return x[..., :self.num_obj].sum(dim=-1, dtype=bool)

    @staticmethod
    def _block(layer, x2, B: int, S: int, key_valid, rng=None, site0: int = 0, p: float = 0.0):
        """One TransformerEncoderLayer (post-norm, ReLU) on tokens x2 [B * S, E]. p > 0: dropout
        at its four sites, masks of (rng, site0 + {0 attention probabilities, 1 dropout1, 2 the
        FFN's inner dropout, 3 dropout2})."""
        sa = layer.self_attn
        E = x2.shape[1]
        in_proj = SimpleNamespace(weight=sa.in_proj_weight, bias=sa.in_proj_bias)
        qkv = linear_act(x2, in_proj, False)
        if p == 0:
            a = ops.mha(qkv.view(B, S, 3 * E), key_valid, sa.num_heads)
        else:
            a = ops.mha(qkv.view(B, S, 3 * E), key_valid, sa.num_heads, rng, site0, p)
        a = linear_act(a.view(B * S, E), sa.out_proj, False)
        x2 = _add_norm(x2, ops.dropout(a, rng, site0 + 1, p), layer.norm1)
        f = ops.dropout(linear_act(x2, layer.linear1, True), rng, site0 + 2, p)
        f = linear_act(f, layer.linear2, False)
        return _add_norm(x2, ops.dropout(f, rng, site0 + 3, p), layer.norm2)

    def tokens(self, x, mask):
        """transformer(encoder(x)) [B, S, E] (:260 / :238-242): the fused block path when attn_ok,
        else torch's modules. With fused_dropout and dropout > 0 in train(): one snapshot of the
        generator state serves every site of this forward and of its backward, and the live state
        moves on by one at the end (a backward that runs after later forwards still regenerates
        its own forward's masks)."""
        B, S, _ = x.shape
        E = self.encoder.out_features
        if not attn_ok(x, E, self.num_heads, self.dropout, self.fused_dropout):
            pad = None if mask is None else ~mask
            return self.transformer(self.encoder(x), src_key_padding_mask=pad), False
        p = self.dropout if self.training else 0.0
        snap = None
        if p > 0:
            if 4 * len(self.transformer.layers) > ops.DROPOUT_SITES:
                raise ValueError("fused dropout numbers its sites 4 * layer + k < 256")
            if self.rng is None or self.rng.device != x.device:
                self.rng = ops.philox_state(self.seed, x.device)
            snap = self.rng.clone()
        kv = None if mask is None else mask.to(torch.uint8).contiguous()
        h = linear_act(x.reshape(B * S, x.shape[2]), self.encoder, False)
        for i, layer in enumerate(self.transformer.layers):
            h = self._block(layer, h, B, S, kv, snap, 4 * i, p)
        if p > 0:
            ops.philox_advance(self.rng)
        return h.view(B, S, E), True

    def trunk(self, x, prescaled: bool = False):
        """The pooled hidden [B, E] (PPOAgent.forward). As the reference, the post layers run only
        on the masking path."""
        if not self.masking:
            h, _ = self.tokens(x, None)
            return pool(h, None, self.pooling_type)
        mask = self.valid_mask(x)
        h, fused = self.tokens(x, mask)
        if fused:
            for i in range(0, len(self.network), 2):
                h = linear_act(h, self.network[i], True)
        else:
            h = self.network(h)
        return pool(h, mask, self.pooling_type)

    def forward(self, x):
        return self.trunk(x)


class TransformerTrainer(PPOTrainer):
    """PPOTrainer with the object-set transformer agent; observations [S = buffer_window_size,
    F = num_features] of the synthetic object env."""

    def _make_agent(self) -> nn.Module:
        a = self.args
        if len(self.obs_shape) != 2:
            raise ValueError(f"object-set observations are [S, F], got {self.obs_shape}")
        return OCTransformerAgent(EnvSpec(self.obs_shape, self.A), a.emb_dim, a.num_heads,
                                  a.num_blocks, a.masking, a.num_obj, None,
                                  pooling_type=a.pooling_type, num_post_layers=a.num_post_layers,
                                  dropout=a.dropout, fused_dropout=a.fused_dropout, seed=a.seed)


def run_transformer(args, device=None) -> TransformerTrainer:
    return run(args, device, trainer_cls=TransformerTrainer)


def main(argv=None):
    return learner_main(TransformerArgs, finalize, run_transformer,
                        "oc_cleanrl_amd transformer PPO (ppo_atari_oc_transformer.py surface)",
                        argv)


if __name__ == "__main__":
    main()
