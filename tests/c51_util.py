"""Shared by the C51 tests: the fixtures of tests/golden/gen_golden_c51.py, a torch restatement of
the loss block they were made from, the error rule both test files apply, and the seeded cases
test_dist_shapes_gpu.py runs at other shapes."""
from __future__ import annotations

import functools

import numpy as np
import torch

import dist_util
from dist_util import F32_FLOOR, rel_err  # noqa: F401  (the test files import them from here)

FIXTURES = ("b32_a6_n51", "ties", "peaked", "b7_a18_n101")
CHECKED = ("target_pmfs", "dlogits", "loss", "q_values")


def fixture(name: str) -> dict:
    return dist_util.fixture(name, "c51_")


def c51_loss_torch(logits, logits_next, atoms, actions, rewards, dones, gamma, v_min, v_max,
                   b=None):
    """The C51 loss on [B, A * N] logits in the dtype of `logits` (every tensor in that dtype,
    actions int64): the target net's greedy next action by expected value, the categorical
    projection of r + gamma * atoms * (1 - d) onto the support in index_add_ order (lower
    neighbours, then upper), and the clamped cross entropy against the taken action's pmf.
    `logits` may require grad. `b` [B, N], when given, is the projected index to use in place of
    the one formed here (projected_index: the f32 one, shared by the f32 run and its twin).
    Returns a dict of tensors."""
    B, N = logits.shape[0], atoms.numel()
    A = logits.shape[1] // N
    rows = torch.arange(B)
    with torch.no_grad():
        pm = torch.softmax(logits_next.view(B, A, N), dim=2)
        next_action = torch.argmax((pm * atoms).sum(2), 1)
        next_pmfs = pm[rows, next_action]
        if b is None:
            next_atoms = rewards.view(B, 1) + gamma * atoms * (1 - dones.view(B, 1))
            delta_z = atoms[1] - atoms[0]
            b = (next_atoms.clamp(v_min, v_max) - v_min) / delta_z
        b = b.to(logits.dtype)
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


def restated(z: dict, dtype, b=None) -> dict:
    """c51_loss_torch + autograd on fixture `z` in `dtype`, as numpy arrays (with dlogits). In
    float64 gamma is the value the f32 run rounds it to, as in the fixture's twin. `b`: the
    projected index to use (c51_loss_torch)."""
    t = lambda k: torch.from_numpy(z[k]).to(dtype)  # noqa: E731
    gamma = float(z["gamma"]) if dtype == torch.float32 else float(np.float32(z["gamma"]))
    args = [t("logits"), t("logits_next"), t("atoms"), torch.from_numpy(z["actions"]),
            t("rewards"), t("dones"), gamma, float(z["v_min"]), float(z["v_max"]), b]
    return dist_util.restated(c51_loss_torch, args, {"dlogits": 0})


def bounds(z: dict) -> dict:
    """Per checked tensor: max(3 x the f32 reference's own error against the f64 twin, 4 * 2^-23)
    and that reference error."""
    return dist_util.bounds(z, CHECKED)


# ---- generated cases (dist_util.LOSS_SHAPES / ACT_SHAPES) ----------------------------------------
def projected_index(z: dict) -> torch.Tensor:
    """The projected index b [B, N] of case or fixture `z`, formed once in f32 in the reference's
    op order: r + (f32(gamma) * z) * (1 - d), clamp, - v_min, / (atoms[1] - atoms[0]). It is a
    function of the inputs alone; the kernel's header promises the same per-op rounding, so the
    f32 restatement and the f64 twin both take this b and differ only downstream of it."""
    t = lambda k: torch.from_numpy(z[k]).float()  # noqa: E731
    atoms, B = t("atoms"), z["rewards"].shape[0]
    next_atoms = t("rewards").view(B, 1) + float(z["gamma"]) * atoms * (1 - t("dones").view(B, 1))
    return (next_atoms.clamp(float(z["v_min"]), float(z["v_max"])) - float(z["v_min"])) / (
        atoms[1] - atoms[0])


def expected_q(logits, atoms, A: int, dtype) -> torch.Tensor:
    """(softmax(logits.view(E, A, N), 2) * atoms).sum(2) in `dtype`."""
    E, N = logits.shape[0], atoms.numel()
    return (torch.softmax(logits.to(dtype).view(E, A, N), dim=2) * atoms.to(dtype)).sum(2)


def make_case(B: int, A: int, N: int, seed: int) -> dict:
    """Seeded inputs of the C51 loss at (B, A, N), with dist_util.plant_edges' rows."""
    rng = dist_util.case_rng("c51", (B, A, N), seed)
    atoms = torch.linspace(dist_util.V_MIN, dist_util.V_MAX, N).numpy()
    z = dict(logits=dist_util.randn2(rng, B, A * N), logits_next=dist_util.randn2(rng, B, A * N),
             atoms=atoms, support=atoms, **dist_util.transitions(rng, B, A),
             gamma=dist_util.GAMMA, gamma_eff=dist_util.GAMMA, v_min=dist_util.V_MIN,
             v_max=dist_util.V_MAX)

    def index_of(r):  # the f32 index of a `done` row with reward r
        row = dict(z, rewards=np.array([r], np.float32), dones=np.ones(1, np.float32))
        return projected_index(row)[0, 0]

    dist_util.plant_edges(z, N, index_of)
    return z


def with_refs(z: dict) -> dict:
    """Case `z` with its shared f32 index b, the f32 restatement and the f64 twin on that b, and
    the twin's expected values of the target net's next-state actions."""
    b = projected_index(z)
    A = z["logits"].shape[1] // z["atoms"].size
    q64 = expected_q(torch.from_numpy(z["logits_next"]), torch.from_numpy(z["atoms"]), A,
                     torch.float64).numpy()
    return dict(z=z, b=b.numpy(), r32=restated(z, torch.float32, b),
                r64=restated(z, torch.float64, b), q64=q64)


@functools.lru_cache(maxsize=None)
def loss_case(B: int, A: int, N: int) -> dict:
    """The generated case at (B, A, N), made once per session and shared; callers must not
    modify the arrays."""
    return with_refs(make_case(B, A, N, dist_util.CASE_SEED))


@functools.lru_cache(maxsize=None)
def act_case(E: int, A: int, N: int) -> dict:
    """Seeded inputs of the acting kernel at (E, A, N) as CPU tensors, with the expected values
    in f32 and f64 (numpy); shared, callers must not modify them."""
    rng = dist_util.case_rng("c51_act", (E, A, N), dist_util.CASE_SEED)
    logits = torch.from_numpy(dist_util.randn2(rng, E, A * N))
    atoms = torch.linspace(dist_util.V_MIN, dist_util.V_MAX, N)
    return dict(logits=logits, atoms=atoms, support=atoms,
                q32=expected_q(logits, atoms, A, torch.float32).numpy(),
                q64=expected_q(logits, atoms, A, torch.float64).numpy())
