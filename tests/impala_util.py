"""The IMPALA units restated in plain torch (dtype-generic: float64 on the CPU is the twin, float32
on the GPU is torch's own computation whose error sets the bound), the kernel tests' cases, and
the bound they share.

Inputs of a case come from torch.manual_seed(seed) in float64, drawn in the order x, weights
(randn / sqrt(9 Cin)) and biases (0.1 randn) as the functions take them, then the upstream
gradient. Every case's seed keeps the twin's ReLU inputs (|x| and the mid pre-activation) and the
top-2 gap of every pool window at >= MARGIN (asserted), so no unit or argmax can flip in f32.
"""
from __future__ import annotations

import functools
import math

import torch
import torch.nn.functional as F

MARGIN = 1e-5
FLOOR = 2.0 ** -20
T = 14  # the kernels' tile edge (pooled outputs: 7, i.e. 13 / 14 and 15 / 16 input rows)

# (C, B, H, W, seed)
RES_CASES = [(16, 1, 1, 1, 0), (16, 2, 2, 3, 0), (32, 2, 2, 3, 0), (16, 1, 11, 11, 0),
             (32, 1, 11, 11, 0), (16, 3, 21, 21, 1), (32, 3, 21, 21, 0), (16, 1, 17, 23, 0),
             (32, 1, 17, 23, 0), (16, 2, 42, 42, 0), (32, 1, 32, 32, 0),
             (32, 1, T - 1, T - 1, 0), (16, 1, T, T, 0), (32, 1, T + 1, T + 1, 0),
             (16, 520, 2, 3, 0)]  # 520 tiles on 256 workgroups: accumulators kept across tiles
# (B, Cin, Cout, H, W, seed)
CP_CASES = [(1, 4, 16, 1, 1, 0), (2, 3, 16, 2, 3, 0), (2, 4, 16, 12, 9, 0), (1, 16, 32, 17, 23, 0),
            (1, 32, 32, 11, 11, 0), (3, 32, 32, 21, 21, 0), (2, 16, 32, 42, 42, 0),
            (1, 4, 16, 84, 84, 0), (1, 3, 16, 64, 64, 2),
            (1, 16, 32, T - 1, T - 1, 0), (1, 32, 32, T, T, 0), (1, 4, 16, T + 1, T + 1, 0)]


def res_block(x, w0, b0, w1, b1):
    """(y, mid pre-activation) of ppg.ResidualBlock."""
    z0 = F.conv2d(F.relu(x), w0, b0, padding=1)
    return x + F.conv2d(F.relu(z0), w1, b1, padding=1), z0


def conv_pool(x, w, b):
    """(p, conv output) of ConvSequence's first two lines."""
    z = F.conv2d(x, w, b, padding=1)
    return F.max_pool2d(z, kernel_size=3, stride=2, padding=1), z


def _draw(seed, x_shape, w_shapes):
    torch.manual_seed(seed)
    t = [torch.randn(x_shape, dtype=torch.float64)]
    for s in w_shapes:
        t.append(torch.randn(s, dtype=torch.float64) / math.sqrt(9 * s[1]))
        t.append(0.1 * torch.randn(s[0], dtype=torch.float64))
    return t


def run(fn, inputs, g, dtype, dev, no_dx=False):
    """(y, [gradients of the inputs]) of fn under autograd in dtype on dev."""
    leaves = [t.detach().to(dev, dtype).clone().requires_grad_(not (no_dx and i == 0))
              for i, t in enumerate(inputs)]
    y = fn(*leaves)[0]
    y.backward(g.to(dev, dtype))
    return y.detach(), [t.grad for t in leaves if t.requires_grad]


@functools.lru_cache(maxsize=None)
def res_case(case):
    """(inputs, g, y64, grads64) of a residual-block case; the margins asserted."""
    C, B, H, W, seed = case
    inputs = _draw(seed, (B, C, H, W), [(C, C, 3, 3)] * 2)
    g = torch.randn(B, C, H, W, dtype=torch.float64)
    z0 = res_block(*inputs)[1]
    assert float(inputs[0].abs().min()) >= MARGIN and float(z0.abs().min()) >= MARGIN, case
    return (inputs, g) + run(res_block, inputs, g, torch.float64, "cpu")


@functools.lru_cache(maxsize=None)
def cp_case(case):
    """(inputs, g, p64, grads64 incl. dx) of a conv + pool case; the window gaps asserted."""
    B, cin, cout, H, W, seed = case
    inputs = _draw(seed, (B, cin, H, W), [(cout, cin, 3, 3)])
    g = torch.randn(B, cout, (H + 1) // 2, (W + 1) // 2, dtype=torch.float64)
    z = F.pad(conv_pool(*inputs)[1], (1, 1, 1, 1), value=-math.inf)
    win = F.unfold(z, 3, stride=2).reshape(B, cout, 9, -1)
    top = win.topk(2, dim=2).values
    assert float((top[:, :, 0] - top[:, :, 1]).min()) >= MARGIN, case
    return (inputs, g) + run(conv_pool, inputs, g, torch.float64, "cpu")


def rel(a, twin) -> float:
    m = float(twin.abs().max())
    return float((a.double().cpu() - twin).abs().max()) / (m if m > 0 else 1.0)


def check(name, got, f32, twin):
    """|got - twin|_inf / |twin|_inf <= max(4 x torch f32's, 2^-20); 4 x: another summation order."""
    e, own = rel(got, twin), rel(f32, twin)
    print(f"{name}: kernel {e:.3e} torch {own:.3e}")
    assert e <= max(4 * own, FLOOR), (name, e, own)
