"""The MaDi learner's host side (no GPU): arguments, state-dict keys and initial weights against
the reference's fixtures, the module's forward, finalize's rejections, the autograd function's
torch fallback and ops.madi_ok's refusals."""
from __future__ import annotations

import dataclasses
import json

import numpy as np
import pytest
import torch

import madi_util as U
from conftest import GOLDEN, golden

from oc_cleanrl_amd import madi, ops
from oc_cleanrl_amd.agents import EnvSpec, PPODefault

NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")
REF_FILES = ("madi_ref_b1w1h3f16.npz", "madi_ref_b2w1h17f32.npz", "madi_ref_b1w4h17f32.npz")


def test_args_match_the_script():
    ref = json.loads((GOLDEN / "madi_args_fields.json").read_text())
    mine = {f.name: f.default for f in dataclasses.fields(madi.MaDiArgs)}
    assert [r["name"] for r in ref] == list(mine)[:len(ref)]  # same names and order, ours after
    for r in ref:
        if r["name"] == "backend":  # ALE / OCAtari are not available: declared difference
            assert mine["backend"] == "Synthetic" and r["default"] == "OCAtari"
            continue
        got = list(mine[r["name"]]) if isinstance(mine[r["name"]], tuple) else mine[r["name"]]
        assert got == r["default"], r["name"]
    assert mine["mask_bootstrap"] is False
    for n in ("rollout_frame_cache", "rollout_fusion", "update_frame_dedup", "dp_overlap"):
        assert n not in mine and getattr(madi.MaDiArgs, n) is False  # fixed off, not flags


def test_state_dict_keys():
    keys = json.loads((GOLDEN / "madi_state_keys.json").read_text())
    assert list(madi.MaskerNet((4, 84, 84), 3, 32).state_dict()) == keys["masker"]
    agent = PPODefault(EnvSpec((4, 84, 84), 6), None, normalize=False)
    assert list(agent.state_dict()) == keys["agent"]


def test_initial_weights_bitwise():
    fx = golden("madi_init_f32.npz")
    torch.manual_seed(int(fx["seed"]))
    sd = madi.MaskerNet((4, 84, 84), 3, 32).state_dict()
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), fx[k]), k
    w = sd["layers.3.weight"]
    centre = w[:, :, 1, 1].clone()
    assert float((w.abs().sum() - centre.abs().sum()).abs()) == 0.0  # every other tap is zero
    assert torch.allclose(centre @ centre.T, 2.0 * torch.eye(32), atol=1e-5)  # gain sqrt(2)
    assert all(float(sd[f"layers.{i}.bias"].abs().max()) == 0.0 for i in (1, 3, 5))


def _module(fx):
    F, W, H = fx["w1"].shape[0], fx["x"].shape[1], fx["x"].shape[2]
    m = madi.MaskerNet((W, H, H), 3, F)
    convs = [l for l in m.layers if isinstance(l, torch.nn.Conv2d)]
    with torch.no_grad():
        for i, c in enumerate(convs):
            c.weight.copy_(torch.from_numpy(fx[NAMES[2 * i]]))
            c.bias.copy_(torch.from_numpy(fx[NAMES[2 * i + 1]]))
    return m


@pytest.mark.parametrize("name", REF_FILES)
def test_forward_bitwise_against_the_reference_module(name):
    fx = golden(name)
    m = _module(fx)
    with torch.no_grad():
        y = m(torch.from_numpy(fx["x"]).float())
    assert np.array_equal(y.numpy(), fx["y_f32"])
    # the fixture's case is the recipe's, and its f64 twin the recorded one
    B, W, H, _ = fx["x"].shape
    case, y64, g64, zmin = U.case_and_twin((B, W, H, fx["w1"].shape[0]))
    assert int(fx["seed"]) == case["seed"] and np.array_equal(case["x"].numpy(), fx["x"])
    assert zmin >= U.Z_MIN
    np.testing.assert_allclose(y64.numpy(), fx["y_f64"], rtol=1e-12, atol=1e-12)
    for n, d in zip(NAMES, g64):
        np.testing.assert_allclose(d.numpy(), fx["d" + n], rtol=1e-9, atol=1e-12)


def test_finalize_rejections():
    A = madi.MaDiArgs
    with pytest.raises(NotImplementedError):
        madi.finalize(A(architecture="PPO"))
    with pytest.raises(ValueError):
        madi.finalize(A(obs_mode="obj"))
    with pytest.raises(NotImplementedError):
        madi.finalize(A(), world_size=2)
    a = madi.finalize(A(num_envs=4, num_steps=8, num_minibatches=2))
    assert (a.batch_size, a.minibatch_size, a.local_num_envs) == (32, 16, 4)


def test_autograd_function_fallback_equals_the_modules():
    fx = golden("madi_ref_b1w4h17f32.npz")
    m = _module(fx)
    src = torch.from_numpy(fx["x"]).repeat(3, 1, 1, 1)
    src[1] = 255 - src[1]
    idx = torch.tensor([2, 1, 1, 0])
    g = torch.from_numpy(np.tile(fx["g"], (4, 1, 1, 1))) * torch.arange(1, 5).view(4, 1, 1, 1)
    y_ref = m(src[idx].float())
    d_ref = torch.autograd.grad(y_ref, m.weights(), g)
    y = madi.masked_stacks(src, idx, m.weights(), fused=True)  # CPU tensors: the torch ops
    d = torch.autograd.grad(y, m.weights(), g)
    assert torch.equal(y, y_ref)
    for a, b in zip(d, d_ref):
        assert torch.equal(a, b)
    yc = madi.masked_stacks(src, idx, m.weights(), fused=False, channels_last=True)
    assert yc.is_contiguous(memory_format=torch.channels_last) and torch.equal(yc, y_ref)


def test_madi_ok_refusals():
    def weights(F):
        return U.make_case(1, 1, 3, F, 0)["weights"]

    x = torch.zeros((2, 4, 84, 84), dtype=torch.uint8)
    w32 = weights(32)
    assert not ops.madi_ok(x, w32)  # CPU tensors
    # the structural refusals hold whatever the device: judged on a stand-in that claims the GPU
    class OnGpu(torch.Tensor):
        @property
        def device(self):
            return torch.device("cuda", 0)

    g = lambda t: t.as_subclass(OnGpu)  # noqa: E731
    xs, ws = g(x), tuple(g(t) for t in w32)
    assert ops.madi_ok(xs, ws)
    assert not ops.madi_ok(xs, ws, num_layers=2) and not ops.madi_ok(xs, ws, num_layers=4)
    assert not ops.madi_ok(xs, tuple(g(t) for t in weights(8)))
    assert ops.madi_ok(xs, tuple(g(t) for t in weights(16)))
    assert not ops.madi_ok(xs, ws, padding_mode="reflect")
    # a call larger than any that ran on hardware goes to the torch modules; so does a
    # differentiated one with MADI_FUSED_UPDATE off
    assert ops.madi_ok(xs, ws, stacks=320) and ops.madi_ok(xs, ws, stacks=320, backward=True)
    old, ops.MADI_FUSED_UPDATE = ops.MADI_FUSED_UPDATE, False
    try:
        assert ops.madi_ok(xs, ws, stacks=320) and not ops.madi_ok(xs, ws, stacks=320,
                                                                   backward=True)
    finally:
        ops.MADI_FUSED_UPDATE = old
    assert ops.madi_ok(xs, ws, stacks=ops.MADI_MAX_STACKS)
    assert not ops.madi_ok(xs, ws, stacks=ops.MADI_MAX_STACKS + 1)
    assert madi._image_size(3136) == 84 and madi._image_size(64) == 36
    assert not ops.madi_ok(g(torch.zeros((2, 4, 84, 80), dtype=torch.uint8)), ws)
    assert not madi.MaskerNet((4, 84, 84), 2, 32).fused_ok(x)
    assert not madi.MaskerNet((4, 84, 84), 3, 8).fused_ok(x)
