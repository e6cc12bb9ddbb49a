"""Shared inputs of the MaDi masker tests: the case recipe (random weights on every tap with std
sqrt(2 / fan_in), biases uniform in +-0.5 so that an out-of-image halo error shows, u8 pixels), the
f64 twin and the torch f32 reference. tests/golden/gen_golden_madi.py uses the same recipe."""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as Fn

# (B stacks, W frames per stack, H, F filters) -> seed: the first seed in [0, 100) for which no
# ReLU pre-activation of the f64 twin satisfies |z| < 1e-5 (gen_golden_madi.py --search)
Z_MIN = 1e-5
CASE_SEEDS = {
    (1, 1, 1, 32): 0, (1, 1, 3, 16): 0, (1, 1, 9, 32): 0, (1, 1, 10, 16): 0,
    (1, 1, 11, 32): 0, (1, 1, 13, 16): 0, (1, 1, 14, 32): 0, (1, 1, 15, 32): 0,
    (1, 1, 29, 32): 1, (1, 1, 84, 32): 44, (1, 4, 17, 32): 1, (1, 4, 33, 16): 8,
    (2, 1, 17, 32): 1, (5, 1, 3, 32): 0, (5, 1, 17, 16): 1, (5, 1, 33, 32): 74,
}
CASES = sorted(CASE_SEEDS)


def make_case(B: int, W: int, H: int, F: int, seed: int) -> dict:
    """x u8 [B, W, H, H], weights (w1, b1, w2, b2, w3, b3) f32, g f32 [B, W, H, H]; CPU tensors
    drawn in this order from one generator."""
    gen = torch.Generator().manual_seed(seed)
    ws = []
    for cout, cin in ((F, 1), (F, F), (1, F)):
        ws.append(torch.randn((cout, cin, 3, 3), generator=gen) * math.sqrt(2.0 / (9 * cin)))
        ws.append(torch.rand(cout, generator=gen) - 0.5)
    x = torch.randint(0, 256, (B, W, H, H), generator=gen, dtype=torch.int64).to(torch.uint8)
    g = torch.randn((B, W, H, H), generator=gen)
    return {"x": x, "weights": tuple(ws), "g": g, "shape": (B, W, H, F), "seed": seed}


def masker(x, weights, pre=None):
    """MaskerNet.forward in torch ops at the dtype of its arguments; pre: a list that receives the
    two ReLU pre-activations."""
    w1, b1, w2, b2, w3, b3 = weights
    H = x.shape[-1]
    z1 = Fn.conv2d(x.reshape(-1, 1, H, H) / 255.0, w1, b1, padding=1)
    z2 = Fn.conv2d(torch.relu(z1), w2, b2, padding=1)
    m = torch.sigmoid(Fn.conv2d(torch.relu(z2), w3, b3, padding=1))
    if pre is not None:
        pre += [z1, z2]
    return x * m.view(x.shape)


def reference(case: dict, dtype, device="cpu"):
    """(y, six gradients, min |ReLU pre-activation|) of the torch ops at `dtype` on `device`."""
    x = case["x"].to(device=device, dtype=dtype)
    ws = tuple(w.to(device=device, dtype=dtype).requires_grad_() for w in case["weights"])
    pre: list = []
    y = masker(x, ws, pre)
    grads = torch.autograd.grad(y, ws, case["g"].to(device=device, dtype=dtype))
    zmin = min(float(z.detach().abs().min()) for z in pre)
    return y.detach(), tuple(grads), zmin


@functools.lru_cache(maxsize=None)
def case_and_twin(shape):
    """The committed-seed case of `shape` with its f64 twin (computed once per process)."""
    seed = CASE_SEEDS[shape]
    case = make_case(*shape, seed)
    y64, g64, zmin = reference(case, torch.float64)
    return case, y64, g64, zmin


def find_seed(shape, limit: int = 100):
    for seed in range(limit):
        if reference(make_case(*shape, seed), torch.float64)[2] >= Z_MIN:
            return seed
    return None
