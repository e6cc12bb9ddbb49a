"""One post-norm transformer encoder block (torch.nn.TransformerEncoderLayer, batch_first, ReLU,
no dropout) and the object-set agent around it, restated in plain torch ops on a dict of
parameters. Dtype-generic: run on float64 copies of f32 inputs and weights it is the float64 twin
for shapes the fixtures do not cover (tests/test_transformer_cpu.py checks it against them).

The error rule of DESIGN.md 11: a tensor's error against the f64 twin, relative to the twin's
largest element, is at most max(3 x the f32 torch computation's own error, 4 * 2^-23).
"""
from __future__ import annotations

import math

import torch

FLOOR = 4 * 2.0 ** -23


def rel_err(a, twin) -> float:
    """max |a - twin| / max |twin| (in float64)."""
    a, twin = torch.as_tensor(a).double().cpu(), torch.as_tensor(twin).double().cpu()
    m = float(twin.abs().max())
    return float((a - twin).abs().max()) / (m if m > 0 else 1.0)


def bound(own: float) -> float:
    return max(3 * own, FLOOR)


def check(name, got, f32, twin):
    """Assert the rule for one tensor; prints the (measured, reference's-own) pair first."""
    e, own = rel_err(got, twin), rel_err(f32, twin)
    print(f"{name}: {e:.3g} / {own:.3g}")
    assert e <= bound(own), (name, e, own)
    return e, own


def mha_ref(qkv, key_valid, heads: int):
    """nn.MultiheadAttention's math on the in-proj output qkv [B, S, 3E] (q | k | v): per head
    softmax(q k^T / sqrt(dh) + mask) v with -inf at excluded keys, heads concatenated."""
    B, S, E3 = qkv.shape
    E = E3 // 3
    dh = E // heads
    q, k, v = (t.reshape(B, S, heads, dh).transpose(1, 2) for t in qkv.split(E, dim=2))
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    if key_valid is not None:
        s = s.masked_fill(~key_valid.bool()[:, None, None, :], float("-inf"))
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, S, E)


def add_layernorm_ref(x, res, weight, bias, eps: float = 1e-5):
    z = x + res
    mu = z.mean(-1, keepdim=True)
    var = ((z - mu) ** 2).mean(-1, keepdim=True)
    return (z - mu) / torch.sqrt(var + eps) * weight + bias


def block_ref(x, p: dict, prefix: str, heads: int, key_valid, eps: float = 1e-5):
    """x [B, S, E] through the layer whose parameters are p[prefix + ...]."""
    g = lambda k: p[prefix + k]  # noqa: E731
    qkv = x @ g("self_attn.in_proj_weight").T + g("self_attn.in_proj_bias")
    a = mha_ref(qkv, key_valid, heads) @ g("self_attn.out_proj.weight").T + \
        g("self_attn.out_proj.bias")
    x = add_layernorm_ref(x, a, g("norm1.weight"), g("norm1.bias"), eps)
    f = torch.relu(x @ g("linear1.weight").T + g("linear1.bias")) @ g("linear2.weight").T + \
        g("linear2.bias")
    return add_layernorm_ref(x, f, g("norm2.weight"), g("norm2.bias"), eps)


def pool_ref(h, mask, pooling_type: str):
    """The reference's pooling variants (mask None: masking off)."""
    if pooling_type == "first":
        return h[:, 0, :]
    if mask is None:
        return h.max(1)[0] if pooling_type == "max" else h.mean(1)
    if pooling_type == "max":
        return (h * mask.unsqueeze(-1)).max(1)[0]
    return h.sum(1) / mask.sum(1, keepdim=True)


def agent_ref(x, p: dict, *, heads: int, blocks: int, post: int, num_obj: int, masking: bool,
              pooling_type: str):
    """(hidden, logits, value, [encoder output, block outputs...]) of the agent on x [B, S, F]."""
    mask = (x[..., :num_obj] != 0).any(-1) if masking else None
    h = x @ p["encoder.weight"].T + p["encoder.bias"]
    steps = [h]
    for i in range(blocks):
        h = block_ref(h, p, f"transformer.layers.{i}.", heads, mask)
        steps.append(h)
    if masking:
        for i in range(post):
            h = torch.relu(h @ p[f"network.{2 * i}.weight"].T + p[f"network.{2 * i}.bias"])
    hidden = pool_ref(h, mask, pooling_type)
    logits = hidden @ p["actor.weight"].T + p["actor.bias"]
    value = hidden @ p["critic.weight"].T + p["critic.bias"]
    return hidden, logits, value, steps


def fixture_params(z: dict, dtype=torch.float32, device="cpu", grad: bool = False) -> dict:
    return {k[2:]: torch.from_numpy(v).to(device, dtype).requires_grad_(grad)
            for k, v in z.items() if k.startswith("p:")}


def fixture_cfg(z: dict) -> dict:
    return dict(heads=int(z["num_heads"]), blocks=int(z["num_blocks"]),
                post=int(z["num_post_layers"]), num_obj=int(z["num_obj"]),
                masking=bool(z["masking"]), pooling_type=str(z["pooling_type"]))


def make_masks(kind: str, B: int, S: int, gen: torch.Generator):
    """key_valid [B, S] bool for a mask kind: none | tail (ragged tail padding per sample) | hole
    (one excluded key in the middle) | one (exactly one valid key)."""
    if kind == "none":
        return None
    m = torch.ones(B, S, dtype=torch.bool)
    if kind == "tail":
        n = torch.randint(1, S + 1, (B,), generator=gen)
        m = torch.arange(S)[None, :] < n[:, None]
    elif kind == "hole":
        if S > 1:
            m[:, S // 2] = False
    elif kind == "one":
        m[:] = False
        m[torch.arange(B), torch.randint(0, S, (B,), generator=gen)] = True
    return m
