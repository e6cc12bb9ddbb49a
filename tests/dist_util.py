"""Shared by the C51 and Rainbow tests (c51_util.py, rainbow_util.py): the fixture loader, the error
rule both apply, and the autograd run of a restated loss."""
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
