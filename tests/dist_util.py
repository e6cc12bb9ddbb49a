"""Shared by the C51 and Rainbow tests (c51_util.py, rainbow_util.py): the fixture loader, the error
rule both apply, the autograd run of a restated loss, and what the generated boundary-shape cases
of test_dist_shapes_cpu.py / test_dist_shapes_gpu.py share (shapes, edge rows, conditions)."""
from __future__ import annotations

import functools

import numpy as np

from conftest import golden

F32_FLOOR = 4 * 2.0 ** -23


@functools.lru_cache(maxsize=None)
def fixture(name: str, prefix: str = "") -> dict:
    """tests/golden/<prefix><name>.npz, loaded once per session and shared; callers must not
    modify the arrays."""
    return golden(f"{prefix}{name}.npz")


def rel_err(x, ref64) -> float:
    """max |x - ref64| relative to ref64's largest element."""
    ref64 = np.asarray(ref64, np.float64)
    return float(np.abs(np.asarray(x, np.float64) - ref64).max() / np.abs(ref64).max())


def bound(ref32, ref64) -> tuple[float, float]:
    """max(3 x the f32 reference's own error against the f64 twin, 4 * 2^-23), and that error."""
    ref = rel_err(ref32, ref64)
    return max(3 * ref, F32_FLOOR), ref


def bounds(z: dict, checked) -> dict:
    """Per checked tensor of fixture `z`: (bound, the f32 reference's own error)."""
    return {k: bound(z[k], z[k + "64"]) for k in checked}


def row_rel_err(x, ref64) -> np.ndarray:
    """Per row of a [B, N] tensor: max |x - ref64| relative to that row's largest ref64 element."""
    ref64 = np.asarray(ref64, np.float64)
    return np.abs(np.asarray(x, np.float64) - ref64).max(1) / np.abs(ref64).max(1)


# ---- generated cases at the kernels' atom / action / batch boundaries ----------------------------
# (B, A, N) of the loss kernels: N = 2, 63, 64, 65, 127, 128 (the second register half empty,
# one-wide, full), A with a partial action batch after zero, one or two full ones, B with a
# partial last round of the 16 waves after zero to six full ones.
LOSS_SHAPES = ((1, 1, 2), (3, 2, 2), (15, 5, 63), (16, 7, 64), (17, 13, 65), (33, 17, 127),
               (49, 11, 128), (100, 18, 128), (16, 6, 128), (17, 12, 64))
ACT_SHAPES = ((1, 1, 2), (4, 7, 64), (5, 13, 65), (9, 17, 128), (3, 18, 127))  # (E, A, N)
CLAMP_SHAPE = (5, 4, 65)  # the out-of-range stored actions
V_MIN, V_MAX, GAMMA = -10.0, 10.0, 0.99
# what a generated case must satisfy before it is launched (assert_case): the f32 reference's own
# error against the twin, and the twin's top-two expected-value gap relative to max |support|
OWN_MAX = GAP_MIN = 64 * 2.0 ** -23
# one seed for every generated case: test_dist_shapes_cpu.py asserts the conditions at every shape
# (a seed that misses one is replaced, the conditions stay)
CASE_SEED = 0


def case_rng(kind: str, shape, seed: int) -> np.random.Generator:
    return np.random.default_rng([seed, *shape, *kind.encode()])


def randn2(rng, *shape) -> np.ndarray:
    """Logits / head outputs of a generated case: randn * 2."""
    return (rng.standard_normal(shape) * 2).astype(np.float32)


def transitions(rng, B: int, A: int) -> dict:
    """Random actions, rewards randn * 4, dones with probability 0.3."""
    return dict(actions=rng.integers(0, A, B),
                rewards=(rng.standard_normal(B) * 4).astype(np.float32),
                dones=(rng.random(B) < 0.3).astype(np.float32))


def integer_index_reward(N: int, index_of) -> np.float32:
    """A reward whose `done` row projects every atom onto one exactly integer index:
    index_of(r) is the learner's f32 index of that row. Strictly between the clamps where the
    support has an inner atom; at N = 2 the only integers are the two ends, so the row sits on
    v_min itself (index 0 with the clamp inactive)."""
    dz = (V_MAX - V_MIN) / (N - 1)
    for k in sorted(range(1, N - 1), key=lambda k: abs(k - (N - 1) / 3)):
        r = np.float32(V_MIN + k * dz)
        b = float(index_of(r))
        if b == k and V_MIN < float(r) < V_MAX:
            return r
    assert N == 2, N
    return np.float32(V_MIN)


def plant_edges(z: dict, N: int, index_of) -> None:
    """The first rows of case `z` (as many as B holds): a reward past v_max, one past v_min (every
    atom clamped, from both sides), and a `done` row with an exactly integer projected index."""
    B = z["rewards"].shape[0]
    for i, (r, d) in enumerate(((30.0, 0.0), (-30.0, 0.0),
                                (integer_index_reward(N, index_of), 1.0))[:B]):
        z["rewards"][i], z["dones"][i] = r, d


def edges_present(z: dict, b) -> bool:
    """Both clamps and the integer-index row are in case `z` (b: its f32 projected index)."""
    b = np.asarray(b)
    N = b.shape[1]
    na = (z["rewards"][:, None]
          + np.float32(z["gamma_eff"]) * z["support"] * (1 - z["dones"][:, None]))
    hi, lo = (na > V_MAX).all(1), (na < V_MIN).all(1)
    whole = (b == np.floor(b)).all(1) & (na >= V_MIN).all(1) & (na <= V_MAX).all(1)
    if N > 2:
        whole &= ((b > 0) & (b < N - 1)).all(1)
    # a row on v_max has b == N - 1 only as far as the f32 division gives it (62.999996 at N = 64)
    return bool(hi.any() and (np.abs(b[hi] - (N - 1)) <= 1e-5 * N).all() and lo.any()
                and (b[lo] == 0).all() and whole.any())


def top_two_gap(q64) -> float:
    """The smallest difference over the rows of [rows, A] between the two largest values (inf at
    A = 1)."""
    q = np.sort(np.asarray(q64, np.float64), 1)
    return float((q[:, -1] - q[:, -2]).min()) if q.shape[1] > 1 else float("inf")


def own_error(ref32, ref64) -> float:
    """rel_err of the f32 reference against its twin; 0 where both are identically zero."""
    if not np.any(ref64):
        assert not np.any(ref32)
        return 0.0
    return rel_err(ref32, ref64)


def assert_case(c: dict, checked, action_key: str) -> None:
    """What keeps a generated case from hiding a failure (none of it is a tolerance): the f32
    restatement and the twin choose the same action in every row, the twin's expected values
    have no near-tie, the f32 reference's own error is small, so max(3 x own, floor) is never
    loose, and the edge rows are there. A seed that misses one of these is replaced."""
    r32, r64, z = c["r32"], c["r64"], c["z"]
    assert np.array_equal(r32[action_key], r64[action_key]), action_key
    assert np.array_equal(r64[action_key], np.argmax(c["q64"], 1))
    assert top_two_gap(c["q64"]) > GAP_MIN * np.abs(z["support"]).max(), top_two_gap(c["q64"])
    for k in checked:
        assert np.isfinite(r64[k]).all() and own_error(r32[k], r64[k]) <= OWN_MAX, \
            (k, own_error(r32[k], r64[k]))
    assert row_rel_err(r32["target_pmfs"], r64["target_pmfs"]).max() <= OWN_MAX
    if z["rewards"].shape[0] >= 3:
        assert edges_present(z, c["b"])


def assert_act_case(c: dict) -> None:
    """An acting case has no near-tie of expected values, in f64 and in torch's f32 alike."""
    assert top_two_gap(c["q64"]) > GAP_MIN * float(c["support"].abs().max()), top_two_gap(c["q64"])
    assert np.array_equal(c["q32"].argmax(1), c["q64"].argmax(1))


def restated(loss_fn, args, grads: dict) -> dict:
    """loss_fn(*args) + autograd as numpy arrays: its dict of tensors, and under each name of
    `grads` the gradient of the loss w.r.t. args[grads[name]]."""
    for i in grads.values():
        args[i].requires_grad_(True)
    out = loss_fn(*args)
    out["loss"].backward()
    res = {k: v.detach().numpy() for k, v in out.items()}
    for name, i in grads.items():
        res[name] = args[i].grad.numpy()
    return res
