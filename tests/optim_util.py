"""Shared pieces of tests/test_optim_gpu.py: the flat optimizer steps of csrc/ocppo_optim.hip past
their grid caps.

Both launches use capped grids and grid-stride loops, 256 threads a workgroup and one float4 group
(4 elements) a thread and round:
  norm pass  kOptBlocks = 1024 workgroups, kNormU = 4 loads in flight per thread
             -> a second load slot takes data past 1024 * 256 * 4 elements, a second trip of the
                outer loop past 4 times that
  step       kMaxBlocks = 2048 workgroups (Adam, exact Adam, the segment kernel), 1024 (RAdam)
             -> a second round (the prefetch branch taken) past kMaxBlocks * 256 * 4 elements
source_caps() reads the four constants from the source, so a changed cap fails the tests' sizes
loudly instead of leaving them under it.
"""
from __future__ import annotations

import math
import re
from pathlib import Path

import numpy as np
import torch

import pqn_util as U

THREADS, NORM_BLOCKS, NORM_U = 256, 1024, 4
STEP_BLOCKS = {"ocppo_clip_adam_step": 2048, "ocppo_clip_adam_step_exact": 2048,
               "ocppo_clip_adam_step_seg": 2048, "ocppo_clip_radam_step": 1024}
NORM_SLOT = NORM_BLOCKS * THREADS * 4  # 1,048,576 elements a load slot
NORM_TRIP = NORM_SLOT * NORM_U  # 4,194,304 elements a trip of the outer loop
ROUND = 2048 * THREADS * 4  # 2,097,152 elements a round of the 2048-workgroup steps
ROUND_RADAM = 1024 * THREADS * 4

# one full workgroup plus 17 threads into the last round
EDGE = 1024 + 68
P3 = 2 * ROUND + EDGE  # three rounds (five for RAdam), a second trip of the norm pass
P2 = ROUND + EDGE  # two rounds
P2_RADAM = ROUND_RADAM + EDGE
CHUNK = 1_000_000  # 977 workgroups: under every cap, one group a thread

# (entry, the arguments after the workspace, steps, lr, eps) as test_clip_adam_abi_scalar_tail
# runs them
ENTRIES = {
    "adam": ("ocppo_clip_adam_step", (0, None, None, None, None, None), 3, 1e-3, 1e-5),
    "exact": ("ocppo_clip_adam_step_exact", (), 4, 3e-4, 1e-4),
    "radam": ("ocppo_clip_radam_step", (0,), 7, 1e-2, 1e-8),
}
# gradient norms before grad_scale 0.5, around max_norm 0.5: steps 2, 4 and 6 clip
NORMS = (0.2, 2.0, 0.3, 5.0, 0.1, 3.0, 0.4)
CLIPS = [False, True, False, True, False, True, False]


def source_caps() -> dict:
    """The caps as csrc/ocppo_optim.hip states them."""
    import oc_cleanrl_amd

    src = (Path(oc_cleanrl_amd.__file__).parent / "csrc" / "ocppo_optim.hip").read_text()

    def const(pattern):
        m = re.search(pattern, src)
        assert m, pattern
        return math.prod(int(f) for f in m.group(1).split("*"))  # "256 * 8"

    def blocks(rule):
        return const(r"struct %s \{\s*static constexpr int kMaxBlocks = ([0-9 *]+);" % rule)

    return dict(threads=const(r"constexpr int kOptThreads = ([0-9 *]+);"),
                norm_blocks=const(r"constexpr int kOptBlocks = ([0-9 *]+);"),
                norm_u=const(r"constexpr int kNormU = ([0-9 *]+);"),
                adam_blocks=blocks("AdamRule"), exact_blocks=blocks("AdamExactRule"),
                radam_is_norm_blocks="kMaxBlocks = kOptBlocks;" in src)


def step_rounds(entry: str, P: int) -> int:
    """Rounds of the step's grid-stride loop the busiest thread (thread 0 of workgroup 0) runs."""
    groups = P // 4
    grid = min(-(-max(groups, 1) // THREADS), STEP_BLOCKS[entry])
    return -(-groups // (grid * THREADS))


def run_abi(dev, entry, tail, p0, grads, lr, eps, scale, max_norm, each=None):
    """`len(grads)` steps of `entry` through the C ABI on fresh device copies of p0 (a device or
    host tensor) with zero moments; returns device (params, exp_avg, exp_avg_sq, scalars)."""
    from oc_cleanrl_amd import _lib

    P = p0.numel()
    p = p0.to(dev).clone()
    m, v = torch.zeros(P, device=dev), torch.zeros(P, device=dev)
    lrt, sc = torch.tensor([lr], device=dev), torch.zeros(8, device=dev)
    ws = torch.zeros(int(_lib.LIB.ocppo_clip_adam_workspace_bytes(P)), dtype=torch.uint8,
                     device=dev)
    for gr in grads:
        g = gr.to(dev).clone()
        assert g.numel() == P and g.data_ptr() % 16 == 0 and p.data_ptr() % 16 == 0
        _lib.call(entry, torch.cuda.current_stream(dev).cuda_stream, p.data_ptr(), g.data_ptr(),
                  m.data_ptr(), v.data_ptr(), P, lrt.data_ptr(), 0.9, 0.999, eps, scale, max_norm,
                  sc.data_ptr(), ws.data_ptr(), ws.numel(), *tail)
        if each is not None:
            each(p, sc)
    torch.cuda.synchronize()
    return p, m, v, sc


def chunks(P: int):
    """[0, P) as consecutive slices of at most CHUNK elements, each a multiple of 4 long but the
    last, which takes the remainder (and with it the P % 4 scalar tail)."""
    assert CHUNK % 4 == 0
    edges = list(range(0, P, CHUNK))
    return [slice(a, b) for a, b in zip(edges, edges[1:] + [P])]


def normed_grads(P: int, steps: int, seed: int):
    """f32 host gradients whose norms are NORMS[:steps]."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in NORMS[:steps]:
        gr = torch.randn(P, generator=g, dtype=torch.float64)
        out.append((gr * (n / float(gr.norm()))).float())
    return out


def torch_twin(make, grads, p0, dtype, scale, max_norm):
    """Clipped steps of make(p) -> (step(grad), state()) on a `dtype` CPU copy of p0."""
    p = p0.to(dtype).clone()
    step, state = make(p)
    for gr in grads:
        g = gr.to(dtype) * scale
        c, _ = U.clip_coef([g], max_norm)
        step(g * c)
    return (p.detach(),) + tuple(state())


def adam_twin(lr, eps):
    def make(p):
        p.requires_grad_()
        opt = torch.optim.Adam([p], lr=lr, eps=eps)

        def step(g):
            p.grad = g
            opt.step()
        return step, lambda: (opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
    return make


def radam_twin(lr):
    def make(p):
        ref = U.RAdamRef([p], float(np.float32(lr)))
        return (lambda g: ref.step([g])), lambda: (ref.m[0], ref.v[0])
    return make
