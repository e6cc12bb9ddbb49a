"""Shared by the Rainbow tests: the fixtures of tests/golden/gen_golden_rainbow.py, a plain numpy /
torch restatement of the prioritized n-step replay and of the loss block they were made from
(written fresh; test_rainbow_cpu.py checks it against every fixture, test_dist_shapes_gpu.py then
uses it as the oracle at other shapes, on make_case's seeded inputs), and the error rule."""
from __future__ import annotations

import functools

import numpy as np
import torch

import dist_util
from dist_util import F32_FLOOR, bound, fixture, rel_err  # noqa: F401  (imported from here too)

LOSS_FIXTURES = ("b32_a6_n51", "b7_a18_n101", "ties", "edges")
ADDSEQ_FIXTURES = ("c6_n3", "c8_n1", "c8_n3", "c6_n1")
SAMPLE_FIXTURES = ("c6", "c8")
CHECKED = ("target_pmfs", "loss_per_sample", "loss", "q_values", "dvalue", "dadvantage")
f32 = np.float32


# ---- the error rule (dist_util's rel_err / bound) ------------------------------------------------
def bounds(z: dict) -> dict:
    return dist_util.bounds(z, CHECKED)


def check_elementwise(x, ref32, ref64, what=""):
    """The rule per element (leaf priorities, weights against their own twin): |x - twin| / |twin|
    <= max(3 x |ref32 - twin| / |twin|, 4 * 2^-23)."""
    x, ref32, ref64 = (np.asarray(a, np.float64) for a in (x, ref32, ref64))
    err = np.abs(x - ref64) / np.abs(ref64)
    lim = np.maximum(3 * np.abs(ref32 - ref64) / np.abs(ref64), F32_FLOOR)
    assert (err <= lim).all(), (what, err.max(), lim[np.argmax(err - lim)])
    return float(err.max()), float((np.abs(ref32 - ref64) / np.abs(ref64)).max())


# ---- prioritized n-step replay --------------------------------------------------------------------
class PerOracle:
    """Sum tree + prioritized n-step buffer for one env in numpy, in the reference's arithmetic:
    f32 tree nodes, the n-step reward accumulated in f64 and stored as f32, priorities in f32."""

    def __init__(self, capacity, obs_shape, n_step, gamma, alpha, eps=1e-6, obs_dtype=np.uint8):
        self.capacity, self.n_step, self.gamma = int(capacity), int(n_step), float(gamma)
        self.alpha, self.eps = float(alpha), float(eps)
        self.obs = np.zeros((capacity,) + tuple(obs_shape), obs_dtype)
        self.next_obs = np.zeros_like(self.obs)
        self.actions = np.zeros(capacity, np.int64)
        self.rewards = np.zeros(capacity, f32)
        self.dones = np.zeros(capacity, bool)
        self.tree = np.zeros(2 * capacity - 1, f32)
        self.pos = self.size = 0
        self.max_priority = f32(1.0)
        self.ring = []

    def set_leaf(self, idx, value):
        t = int(idx) + self.capacity - 1
        self.tree[t] = value
        while t > 0:
            t = (t - 1) // 2
            self.tree[t] = self.tree[2 * t + 1] + self.tree[2 * t + 2]

    def add(self, obs, action, reward, next_obs, done):
        self.ring.append((obs, int(action), float(reward), next_obs, bool(done)))
        self.ring = self.ring[-self.n_step:]
        if len(self.ring) < self.n_step:
            return
        total, last = 0.0, self.ring[-1]
        for i, entry in enumerate(self.ring):
            total += self.gamma ** i * entry[2]
            if entry[4]:
                last = entry
                break
        k = self.pos
        self.obs[k], self.actions[k] = self.ring[0][0], self.ring[0][1]
        self.next_obs[k], self.rewards[k], self.dones[k] = last[3], total, last[4]
        self.set_leaf(k, f32(self.max_priority) ** f32(self.alpha))
        self.pos = (k + 1) % self.capacity
        self.size = min(self.size + 1, self.capacity)
        if last[4]:
            self.ring = []

    def update_priorities(self, indices, losses):
        p = np.abs(np.asarray(losses, f32)) + f32(self.eps)
        self.max_priority = max(f32(self.max_priority), p.max())
        for i, v in zip(indices, p):
            self.set_leaf(i, v ** f32(self.alpha))

    def leaves(self):
        return self.tree[self.capacity - 1:]


def retrieve(tree, capacity, value) -> int:
    """The descent in f64 against the f32 nodes; returns the slot."""
    t, value = 0, float(value)
    while 2 * t + 1 < len(tree):
        left = float(tree[2 * t + 1])
        if value <= left:
            t = 2 * t + 1
        else:
            value -= left
            t = 2 * t + 2
    return t - (capacity - 1)


def strata(total, B):
    """[segment * i, segment * (i + 1)) in the reference's f32 arithmetic."""
    seg = f32(total) / f32(B)
    i = np.arange(B)
    return seg * i.astype(f32), seg * (i + 1).astype(f32)


def per_weights(tree, capacity, size, indices, beta, dtype=f32):
    """(probs, weights): weights = (size * probs / total) ** -beta / max, in `dtype`."""
    probs = np.asarray(tree)[np.asarray(indices) + capacity - 1]
    w = (dtype(size) * probs.astype(dtype) / dtype(tree[0])) ** dtype(-beta)
    return probs, w / w.max()


def tree_is_consistent(tree, capacity) -> bool:
    """Every inner node is f32(left + right) of its own children, bitwise."""
    tree = np.asarray(tree, f32)
    i = np.arange(capacity - 1)
    return bool(np.array_equal(tree[i], tree[2 * i + 1] + tree[2 * i + 2]))


# ---- the loss block -------------------------------------------------------------------------------
def dueling_dist(value, advantage, A, N):
    adv = advantage.view(-1, A, N)
    return torch.softmax(value.view(-1, 1, N) + adv - adv.mean(dim=1, keepdim=True), dim=2)


def rainbow_loss_torch(value, advantage, value_no, advantage_no, value_nt, advantage_nt, support,
                       actions, rewards, dones, weights, gamma_n, v_min, v_max, delta_z, b=None):
    """The Rainbow loss on raw head outputs in the dtype of `value`: double-Q action by the online
    net, the target net's pmf there, the n-step categorical projection (host delta_z, (l == b),
    l and u clamped; lower neighbours added first, then upper), the clamped cross entropy per
    sample and its importance-weighted mean. `value` / `advantage` may require grad. `b` [B, N],
    when given, is the projected index to use in place of the one formed here (projected_index:
    the f32 one, shared by the f32 run and its twin)."""
    B, N = value.shape
    A = advantage.shape[1] // N
    rows = torch.arange(B)
    with torch.no_grad():
        best = torch.argmax((dueling_dist(value_no, advantage_no, A, N) * support).sum(2), 1)
        next_pmfs = dueling_dist(value_nt, advantage_nt, A, N)[rows, best]
        if b is None:
            next_atoms = rewards.view(B, 1) + gamma_n * support * (1 - dones.view(B, 1))
            b = (next_atoms.clamp(v_min, v_max) - v_min) / delta_z
        b = b.to(value.dtype)
        lo = b.floor().clamp(0, N - 1)
        up = b.ceil().clamp(0, N - 1)
        m_lo = (up + (lo == b).to(b.dtype) - b) * next_pmfs
        m_up = (b - lo) * next_pmfs
        target = torch.zeros_like(next_pmfs)
        for i in range(B):
            target[i].index_add_(0, lo[i].long(), m_lo[i])
            target[i].index_add_(0, up[i].long(), m_up[i])
    pred = dueling_dist(value, advantage, A, N)[rows, actions.view(-1)]
    per_sample = -(target * pred.clamp(min=1e-5, max=1 - 1e-5).log()).sum(1)
    return dict(best_actions=best, target_pmfs=target, loss_per_sample=per_sample,
                loss=(per_sample * weights.view(-1)).mean(),
                q_values=(pred * support).sum(1).mean())


def loss_args(z: dict, dtype):
    """(tensors, scalars) of loss fixture `z` in `dtype`; in float64 gamma ** n_step and delta_z
    are the values the f32 run rounds them to, as in the fixture's twin."""
    t = lambda k: torch.from_numpy(z[k]).to(dtype)  # noqa: E731
    N = z["support"].shape[0]
    gamma_n = float(z["gamma"]) ** int(z["n_step"])
    delta_z = (float(z["v_max"]) - float(z["v_min"])) / (N - 1)
    if dtype == torch.float64:
        gamma_n, delta_z = float(f32(gamma_n)), float(f32(delta_z))
    tensors = [t(k) for k in ("value", "advantage", "value_next_online", "advantage_next_online",
                              "value_next_target", "advantage_next_target", "support")]
    tensors += [torch.from_numpy(z["actions"]), t("rewards"), t("dones"), t("weights")]
    return tensors, (gamma_n, float(z["v_min"]), float(z["v_max"]), delta_z)


def restated(z: dict, dtype, b=None) -> dict:
    """rainbow_loss_torch + autograd on fixture `z` in `dtype`, as numpy arrays. `b`: the
    projected index to use (rainbow_loss_torch)."""
    tensors, scalars = loss_args(z, dtype)
    return dist_util.restated(rainbow_loss_torch, [*tensors, *scalars, b],
                              {"dvalue": 0, "dadvantage": 1})


# ---- generated cases (dist_util.LOSS_SHAPES / ACT_SHAPES) ----------------------------------------
HEADS = ("value", "advantage", "value_next_online", "advantage_next_online", "value_next_target",
         "advantage_next_target")
N_STEP = 3


def projected_index(z: dict) -> torch.Tensor:
    """The projected index b [B, N] of case or fixture `z`, formed once in f32 in the reference's
    op order: r + (f32(gamma ** n_step) * z) * (1 - d), clamp, - v_min, / f32(delta_z). It is a
    function of the inputs alone; the kernel's header promises the same per-op rounding. The
    (l == b) rule is discontinuous in b (at a clamped row f32 gives N - 1 exactly and keeps the
    row's mass, f64 on the f32 delta_z gives N - 1 + eps and drops it), so the f32 restatement
    and the f64 twin both take this b and differ only downstream of it."""
    t = lambda k: torch.from_numpy(z[k]).float()  # noqa: E731
    support, B = t("support"), z["rewards"].shape[0]
    gamma_n = float(z["gamma"]) ** int(z["n_step"])
    v_min, v_max = float(z["v_min"]), float(z["v_max"])
    next_atoms = t("rewards").view(B, 1) + gamma_n * support * (1 - t("dones").view(B, 1))
    return (next_atoms.clamp(v_min, v_max) - v_min) / ((v_max - v_min) / (support.numel() - 1))


def expected_q(value, advantage, support, A: int, dtype) -> torch.Tensor:
    """(dueling_dist(value, advantage) * support).sum(2) in `dtype`."""
    return (dueling_dist(value.to(dtype), advantage.to(dtype), A, support.numel())
            * support.to(dtype)).sum(2)


def make_case(B: int, A: int, N: int, seed: int) -> dict:
    """Seeded inputs of the Rainbow loss at (B, A, N), with dist_util.plant_edges' rows; PER
    weights in [0.05, 1] with one exact 1."""
    rng = dist_util.case_rng("rainbow", (B, A, N), seed)
    z = {k: dist_util.randn2(rng, B, N if k.startswith("value") else A * N) for k in HEADS}
    weights = (0.05 + 0.95 * rng.random(B)).astype(f32)
    weights[rng.integers(0, B)] = 1.0
    z.update(support=torch.linspace(dist_util.V_MIN, dist_util.V_MAX, N).numpy(), weights=weights,
             **dist_util.transitions(rng, B, A), gamma=dist_util.GAMMA, n_step=N_STEP,
             gamma_eff=dist_util.GAMMA ** N_STEP, v_min=dist_util.V_MIN, v_max=dist_util.V_MAX)

    def index_of(r):  # the f32 index of a `done` row with reward r
        row = dict(z, rewards=np.array([r], f32), dones=np.ones(1, f32))
        return projected_index(row)[0, 0]

    dist_util.plant_edges(z, N, index_of)
    return z


def with_refs(z: dict) -> dict:
    """Case `z` with its shared f32 index b, the f32 restatement and the f64 twin on that b, and
    the twin's expected values of the online net's next-state actions (the double-Q choice)."""
    b = projected_index(z)
    N = z["support"].size
    t = lambda k: torch.from_numpy(z[k])  # noqa: E731
    q64 = expected_q(t("value_next_online"), t("advantage_next_online"), t("support"),
                     z["advantage"].shape[1] // N, torch.float64).numpy()
    return dict(z=z, b=b.numpy(), r32=restated(z, torch.float32, b),
                r64=restated(z, torch.float64, b), q64=q64)


@functools.lru_cache(maxsize=None)
def loss_case(B: int, A: int, N: int) -> dict:
    """The generated case at (B, A, N), made once per session and shared; callers must not
    modify the arrays."""
    return with_refs(make_case(B, A, N, dist_util.CASE_SEED))


@functools.lru_cache(maxsize=None)
def act_case(E: int, A: int, N: int) -> dict:
    """Seeded head outputs of the acting kernel at (E, A, N) as CPU tensors, with the expected
    values in f32 and f64 (numpy); shared, callers must not modify them."""
    rng = dist_util.case_rng("rainbow_act", (E, A, N), dist_util.CASE_SEED)
    value = torch.from_numpy(dist_util.randn2(rng, E, N))
    advantage = torch.from_numpy(dist_util.randn2(rng, E, A * N))
    support = torch.linspace(dist_util.V_MIN, dist_util.V_MAX, N)
    return dict(value=value, advantage=advantage, support=support,
                q32=expected_q(value, advantage, support, A, torch.float32).numpy(),
                q64=expected_q(value, advantage, support, A, torch.float64).numpy())
