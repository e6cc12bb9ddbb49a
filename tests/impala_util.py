"""The IMPALA units restated in plain torch (dtype-generic: float64 on the CPU is the twin, float32
on the GPU is torch's own computation whose error sets the bound), the kernel tests' cases, and
the bound they share.

Inputs of a case come from torch.manual_seed(seed) in float64, drawn in the order x, weights
(randn / sqrt(9 Cin)) and biases (0.1 randn) as the functions take them, then the upstream
gradient. Every case's seed keeps the twin's ReLU inputs (|x| and the mid pre-activation) and the
top-2 gap of every pool window at >= MARGIN (asserted), so no unit or argmax can flip in f32.
The exact (lattice) cases further down are the opposite: small integers, full of ties and zeros,
compared bit for bit.
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


def run(fn, inputs, g, dtype, dev, no_dx=False, channels_last=False):
    """(y, [gradients of the inputs]) of fn under autograd in dtype on dev; x (the first input) in
    NCHW order, or channels_last."""
    leaves = [t.detach().to(dev, dtype).clone() for t in inputs]
    if channels_last:
        leaves[0] = leaves[0].contiguous(memory_format=torch.channels_last)
    for i, t in enumerate(leaves):
        t.requires_grad_(not (no_dx and i == 0))
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


# ---- the exact (lattice) cases ------------------------------------------------------------------
# Small-integer inputs: every product, bias add, ReLU, max, skip add and power-of-two scale of the
# two units is then exact in f32 in any summation order, so a kernel equals the f64 twin element by
# element, bit for bit -- at pool ties, at x == 0 and at a pre-activation of exactly 0, which the
# margin cases above exclude. Inputs come from torch.manual_seed(seed) in float64 in the order x,
# (weight, bias) per convolution, upstream gradient:
#   x       integers constant over 3 x 3 pixel blocks (blocky frames cropped to H x W): [-3, 3] for
#           the residual block, [0, 8] for conv + pool
#   weights integers in [-2, 2] times a Bernoulli keep-mask (0.3 for <= 4 input channels, else 0.15)
#   biases, upstream gradient: integers in [-2, 2]
# Every case asserts on the CPU (a case that breaks one is a broken test):
#   exactness  the same graph on |x|, |w|, |b|, |g| with the ReLUs and the pool's selection removed
#              (plain sums) stays below 2^24 units (unit: min(scale, 1)) in every output,
#              pre-activation and gradient, so every partial sum of every ordering is an integer
#              number of units that f32 holds exactly
#   edges      residual block: >= 5 % of x and >= 1 % of the mid pre-activations are exactly 0, one
#              of each on the image border and, where the image has one, on a 14-pixel tile seam
#              conv + pool: >= 5 % of the pool windows hold their maximum twice or more (first and
#              last maximal position differ), one such window over the border (it holds padding)
#              and, where there is one, over a tile seam (conv rows or columns 14 k - 1 and 14 k);
#              a 1 x 1 image has one position per window, so no tie: only exactness is asserted
EXACT_LIMIT = 2.0 ** 24
ZERO_X_FRAC, ZERO_MID_FRAC, TIE_FRAC = 0.05, 0.01, 0.05

_RES_SHAPES = [(3, 1, 1), (2, 2, 3), (1, T - 1, T - 1), (1, T, T), (1, T + 1, T + 1), (1, 17, 23),
               (1, 29, 29)]
# (C, B, H, W, seed); 520 tiles on 256 workgroups: accumulators kept across tiles
LATTICE_RES_CASES = [(C, B, H, W, 0) for C in (16, 32) for B, H, W in _RES_SHAPES] + [
    (16, 520, 2, 3, 0)]

_CP_PAIRS = [(ci, co) for ci in (1, 2, 3, 4, 16, 32) for co in (16, 32)]
# even and odd H and W; 17 x 23 and 29 x 30: 2 x 2 / 3 x 3 tiles forward (7 x 7 pooled) and backward
_CP_SHAPES = [(2, 12, 9), (1, 17, 23), (1, 29, 30)]
# below the halo, and one whole tile beside a one-column tile: once per kernel instantiation
_CP_SMALL = [(3, 1, 1), (2, 2, 3), (1, T, T + 1)]
_CP_SMALL_PAIRS = [(1, 16), (3, 32), (16, 16), (16, 32), (32, 16), (32, 32)]
# seeds other than 0: the first seed whose draw holds every edge the case asserts
_CP_SEEDS = {(2, 16, 16, 2, 3, 1.0): 2, (2, 16, 32, 2, 3, 1.0): 3, (2, 32, 16, 12, 9, 1.0): 1,
             (1, 32, 16, 17, 23, 1.0): 7, (1, 32, 16, 29, 30, 1.0): 2, (2, 32, 16, 2, 3, 1.0): 7,
             (2, 32, 32, 12, 9, 1.0): 6, (1, 32, 32, 29, 30, 1.0): 2, (2, 32, 32, 2, 3, 1.0): 13,
             (1, 32, 32, T, T + 1, 1.0): 5}


def _cp_cases():
    out = []
    for ci, co in _CP_PAIRS:
        shapes = _CP_SHAPES + (_CP_SMALL if (ci, co) in _CP_SMALL_PAIRS else [])
        for B, H, W in shapes:
            for scale in (1.0, 0.25) if ci <= 4 else (1.0,):
                out.append((B, ci, co, H, W, scale))
    out.append((520, 2, 16, 2, 3, 1.0))  # more tiles than workgroups
    return [c + (_CP_SEEDS.get(c, 0),) for c in out]


# (B, Cin, Cout, H, W, scale, seed)
LATTICE_CP_CASES = _cp_cases()


def res_id(case):
    C, B, H, W, _ = case
    return f"C{C}-{B}x{H}x{W}"


def cp_id(case):
    B, ci, co, H, W, scale, _ = case
    return f"cin{ci}-cout{co}-{B}x{H}x{W}-scale{scale:g}"


def lattice(seed, x_shape, x_lo, x_hi, w_shapes):
    """[x, w, b, ...] of a lattice case (float64)."""
    torch.manual_seed(seed)
    B, C, H, W = x_shape
    blocks = torch.randint(x_lo, x_hi + 1, (B, C, (H + 2) // 3, (W + 2) // 3), dtype=torch.float64)
    x = blocks.repeat_interleave(3, dim=2).repeat_interleave(3, dim=3)[:, :, :H, :W].contiguous()
    t = [x]
    for s in w_shapes:
        keep = torch.rand(s, dtype=torch.float64) < (0.3 if s[1] <= 4 else 0.15)
        t.append(torch.randint(-2, 3, s, dtype=torch.float64) * keep)
        t.append(torch.randint(-2, 3, (s[0],), dtype=torch.float64))
    return t


def res_block_sums(x, w0, b0, w1, b1):
    """res_block without its ReLUs."""
    z0 = F.conv2d(x, w0, b0, padding=1)
    return x + F.conv2d(z0, w1, b1, padding=1), z0


def conv_pool_sums(x, w, b):
    """conv_pool with the window's sum for its maximum."""
    z = F.conv2d(x, w, b, padding=1)
    return F.avg_pool2d(z, 3, stride=2, padding=1, divisor_override=1), z


def abs_bound(fn, inputs, g) -> float:
    """Largest output, pre-activation or gradient (of either) of fn, a graph of plain sums, on the
    absolute values: no partial sum of the real graph, in any order, exceeds it."""
    leaves = [t.detach().abs().requires_grad_() for t in inputs]
    y, z = fn(*leaves)
    z.retain_grad()
    y.backward(g.abs())
    return max(float(t.detach().max()) for t in (y, z, z.grad, *(t.grad for t in leaves)))


def _seams(n, period):
    """[n] bool: index i is the first of a tile of `period` other than tile 0."""
    i = torch.arange(n)
    return (i > 0) & (i % period == 0)


def _outer_or(rows, cols):
    return rows[:, None] | cols[None, :]


@functools.lru_cache(maxsize=None)
def lattice_res_case(case):
    """(inputs, g, y64, grads64, stats) of an exact residual-block case; exactness and the zeros
    asserted. stats: the bound and the fractions, for the record."""
    C, B, H, W, seed = case
    inputs = lattice(seed, (B, C, H, W), -3, 3, [(C, C, 3, 3)] * 2)
    g = torch.randint(-2, 3, (B, C, H, W), dtype=torch.float64)
    bound = abs_bound(res_block_sums, inputs, g)
    assert bound < EXACT_LIMIT, (case, bound)
    x0, z0 = inputs[0] == 0, res_block(*inputs)[1] == 0
    fx, fz = float(x0.double().mean()), float(z0.double().mean())
    assert fx >= ZERO_X_FRAC and fz >= ZERO_MID_FRAC, (case, fx, fz)
    iy, ix = torch.arange(H), torch.arange(W)
    border = _outer_or((iy == 0) | (iy == H - 1), (ix == 0) | (ix == W - 1))
    # both sides of a seam: the last row / column of a tile and the first of the next
    sy, sx = _seams(H, T), _seams(W, T)
    seam = _outer_or(sy | sy.roll(-1), sx | sx.roll(-1))
    for name, zero in (("x", x0), ("mid", z0)):
        assert bool((zero & border).any()), (case, name, "no zero on the border")
        assert not bool(seam.any()) or bool((zero & seam).any()), (case, name, "no zero on a seam")
    stats = {"bound": bound, "zero_x": fx, "zero_mid": fz}
    return (inputs, g) + run(res_block, inputs, g, torch.float64, "cpu") + (stats,)


def scaled_conv_pool(scale):
    return lambda x, w, b: conv_pool(x * scale, w, b)


@functools.lru_cache(maxsize=None)
def lattice_cp_case(case):
    """(inputs, g, p64, grads64 incl. dx, stats) of an exact conv + pool case; exactness and the
    ties asserted."""
    B, cin, cout, H, W, scale, seed = case
    HO, WO = (H + 1) // 2, (W + 1) // 2
    inputs = lattice(seed, (B, cin, H, W), 0, 8, [(cout, cin, 3, 3)])
    g = torch.randint(-2, 3, (B, cout, HO, WO), dtype=torch.float64)
    fn = scaled_conv_pool(scale)
    bound = abs_bound(lambda x, w, b: conv_pool_sums(x * scale, w, b), inputs, g)
    assert bound < EXACT_LIMIT * min(scale, 1.0), (case, bound)
    z = F.pad(fn(*inputs)[1], (1, 1, 1, 1), value=-math.inf)
    win = F.unfold(z, 3, stride=2).reshape(B, cout, 9, HO, WO)
    ismax = win == win.amax(dim=2, keepdim=True)
    tied = ismax.sum(dim=2) >= 2
    first = (ismax.cumsum(dim=2) == 0).sum(dim=2)
    last = 8 - (ismax.flip(2).cumsum(dim=2) == 0).sum(dim=2)
    assert bool((first != last)[tied].all()) and bool((first == last)[~tied].all()), case
    ft = float(tied.double().mean())
    if H * W > 1:  # the window of a 1 x 1 image holds one position and eight of padding: no tie
        assert ft >= TIE_FRAC, (case, ft)
        py, px = torch.arange(HO), torch.arange(WO)
        border = _outer_or((py == 0) | (2 * py + 1 >= H), (px == 0) | (2 * px + 1 >= W))
        seam = _outer_or(_seams(HO, T // 2), _seams(WO, T // 2))
        assert bool((tied & border).any()), (case, "no tied window over the border")
        assert not bool(seam.any()) or bool((tied & seam).any()), (case, "no tie over a seam")
    stats = {"bound": bound / min(scale, 1.0), "tied": ft}
    return (inputs, g) + run(fn, inputs, g, torch.float64, "cpu") + (stats,)


# (cin, cout): one NaN in x, forward only
NAN_CP_CASES = [(4, 16), (4, 32), (16, 16), (16, 32)]


@functools.lru_cache(maxsize=None)
def nan_cp_case(pair):
    """(inputs, p64) of the 2 x 12 x 9 lattice case of (cin, cout) with x[0, 1, 5, 4] = NaN: the
    conv positions (4..6, 3..5) of image 0 are NaN in every channel (0 x NaN is NaN), and so are
    the pooled outputs (2..3, 1..3), whose windows hold one (asserted of the twin)."""
    cin, cout = pair
    case = next(c for c in LATTICE_CP_CASES if c[:6] == (2, cin, cout, 12, 9, 1.0))
    inputs = [t.clone() for t in lattice_cp_case(case)[0]]
    inputs[0][0, 1, 5, 4] = math.nan
    p64 = conv_pool(*inputs)[0]
    want = torch.zeros_like(p64, dtype=torch.bool)
    want[0, :, 2:4, 1:4] = True
    assert torch.equal(p64.isnan(), want), pair
    return inputs, p64


def assert_exact(name, got, twin):
    """got == twin in every element; else the first mismatch (index, both values) and their count."""
    got = got.detach().double().cpu()
    assert got.shape == twin.shape, (name, tuple(got.shape), tuple(twin.shape))
    if torch.equal(got, twin):
        return
    bad = got != twin
    idx = tuple(int(i) for i in bad.nonzero()[0])
    msg = (f"{name}: {int(bad.sum())} of {bad.numel()} elements differ; first at {idx}: "
           f"got {float(got[idx])!r}, twin {float(twin[idx])!r}")
    print(msg)
    raise AssertionError(msg)
