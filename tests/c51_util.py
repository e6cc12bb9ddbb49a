"""Shared by the C51 tests: the fixtures of tests/golden/gen_golden_c51.py, a torch restatement of
the loss block they were made from, and the error rule both test files apply."""
from __future__ import annotations

import numpy as np
import torch

import dist_util
from dist_util import F32_FLOOR, rel_err  # noqa: F401  (the test files import them from here)

FIXTURES = ("b32_a6_n51", "ties", "peaked", "b7_a18_n101")
CHECKED = ("target_pmfs", "dlogits", "loss", "q_values")


def fixture(name: str) -> dict:
    return dist_util.fixture(name, "c51_")


def c51_loss_torch(logits, logits_next, atoms, actions, rewards, dones, gamma, v_min, v_max):
    """The C51 loss on [B, A * N] logits in the dtype of `logits` (every tensor in that dtype,
    actions int64): the target net's greedy next action by expected value, the categorical
    projection of r + gamma * atoms * (1 - d) onto the support in index_add_ order (lower
    neighbours, then upper), and the clamped cross entropy against the taken action's pmf.
    `logits` may require grad. Returns a dict of tensors."""
    B, N = logits.shape[0], atoms.numel()
    A = logits.shape[1] // N
    rows = torch.arange(B)
    with torch.no_grad():
        pm = torch.softmax(logits_next.view(B, A, N), dim=2)
        next_action = torch.argmax((pm * atoms).sum(2), 1)
        next_pmfs = pm[rows, next_action]
        next_atoms = rewards.view(B, 1) + gamma * atoms * (1 - dones.view(B, 1))
        delta_z = atoms[1] - atoms[0]
        b = (next_atoms.clamp(v_min, v_max) - v_min) / delta_z
        lo = b.floor().clamp(0, N - 1)
        up = b.ceil().clamp(0, N - 1)
        m_lo = (up + (lo == up).to(b.dtype) - b) * next_pmfs
        m_up = (b - lo) * next_pmfs
        target = torch.zeros_like(next_pmfs)
        for i in range(B):
            target[i].index_add_(0, lo[i].long(), m_lo[i])
            target[i].index_add_(0, up[i].long(), m_up[i])
    old = torch.softmax(logits.view(B, A, N), dim=2)[rows, actions.view(-1)]
    loss = (-(target * old.clamp(min=1e-5, max=1 - 1e-5).log()).sum(-1)).mean()
    return dict(target_pmfs=target, old_pmfs=old, loss=loss,
                q_values=(old * atoms).sum(1).mean(), next_action=next_action)


def restated(z: dict, dtype) -> dict:
    """c51_loss_torch + autograd on fixture `z` in `dtype`, as numpy arrays (with dlogits). In
    float64 gamma is the value the f32 run rounds it to, as in the fixture's twin."""
    t = lambda k: torch.from_numpy(z[k]).to(dtype)  # noqa: E731
    gamma = float(z["gamma"]) if dtype == torch.float32 else float(np.float32(z["gamma"]))
    args = [t("logits"), t("logits_next"), t("atoms"), torch.from_numpy(z["actions"]),
            t("rewards"), t("dones"), gamma, float(z["v_min"]), float(z["v_max"])]
    return dist_util.restated(c51_loss_torch, args, {"dlogits": 0})


def bounds(z: dict) -> dict:
    """Per checked tensor: max(3 x the f32 reference's own error against the f64 twin, 4 * 2^-23)
    and that reference error."""
    return dist_util.bounds(z, CHECKED)
