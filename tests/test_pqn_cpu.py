"""PQN without a GPU: the flag surface and network of pqn_atari_envpool.py, the plain-torch twins
of tests/pqn_util.py pinned against torch itself, and the new C-ABI entry points' validation."""
from __future__ import annotations

import ctypes
import dataclasses
import json

import numpy as np
import pytest
import torch
import torch.nn as nn

import pqn_util as U
from conftest import GOLDEN

FX = json.loads((GOLDEN / "pqn_args.json").read_text())


@pytest.fixture(scope="module")
def pqn():
    from oc_cleanrl_amd import pqn

    return pqn


def test_args_match_the_script(pqn):
    fields = dataclasses.fields(pqn.PQNArgs)
    ref = FX["args"]
    assert [f.name for f in fields[:len(ref)]] == [n for n, _ in ref]
    a = pqn.PQNArgs()
    for n, d in ref:
        assert getattr(a, n) == d, n
    own = {f.name: f.default for f in fields[len(ref):]}
    assert own["architecture"] == "PQN_OBJ" and own["obs_mode"] == "obj"
    assert own["backend"] == "Synthetic" and own["vecnorm_reward"] is False
    assert own["encoder_dims"] == (128, 64) and own["decoder_dims"] == (128,)
    # the PPObj-only rollout / update features are fixed off (not flags)
    for n in ("rollout_frame_cache", "rollout_fusion", "rollout_cache_ring", "update_frame_dedup",
              "x6_weight_planes", "dp_overlap", "dp_exchange"):
        assert n not in own and getattr(a, n) is False, n


def test_finalize_sizes_and_refusals(pqn):
    a = pqn.finalize(pqn.PQNArgs(num_envs=6, num_steps=10, num_minibatches=4,
                                 total_timesteps=1000))
    assert (a.batch_size, a.minibatch_size, a.num_iterations) == (60, 15, 16)
    assert (a.local_num_envs, a.local_batch_size, a.local_minibatch_size) == (6, 60, 15)
    with pytest.raises(NotImplementedError, match="one GPU"):
        pqn.finalize(pqn.PQNArgs(), world_size=2)
    with pytest.raises(NotImplementedError, match="architecture"):
        pqn.finalize(pqn.PQNArgs(architecture="PPO_OBJ"))
    with pytest.raises(ValueError, match="obs_mode"):
        pqn.finalize(pqn.PQNArgs(architecture="PQN"))
    with pytest.raises(ValueError, match="divisible"):
        pqn.finalize(pqn.PQNArgs(num_envs=3, num_steps=5, num_minibatches=4))
    with pytest.raises(ValueError, match="duration"):
        pqn.finalize(pqn.PQNArgs(exploration_fraction=0.0))


def _script_qnetwork(A: int) -> nn.Sequential:
    """pqn_atari_envpool.py:117-135 from torch alone, modules made in the script's order."""
    def li(layer):
        torch.nn.init.orthogonal_(layer.weight, np.sqrt(2))
        torch.nn.init.constant_(layer.bias, 0.0)
        return layer

    return nn.Sequential(
        li(nn.Conv2d(4, 32, 8, stride=4)), nn.LayerNorm([32, 20, 20]), nn.ReLU(),
        li(nn.Conv2d(32, 64, 4, stride=2)), nn.LayerNorm([64, 9, 9]), nn.ReLU(),
        li(nn.Conv2d(64, 64, 3, stride=1)), nn.LayerNorm([64, 7, 7]), nn.ReLU(), nn.Flatten(),
        li(nn.Linear(3136, 512)), nn.LayerNorm(512), nn.ReLU(), li(nn.Linear(512, A)))


def test_pixel_network_keys_shapes_and_seeded_init(pqn):
    from oc_cleanrl_amd.agents import EnvSpec

    A = 4
    torch.manual_seed(7)
    net = pqn.PQNetwork(EnvSpec((4, 84, 84), A), "PQN")
    sd = net.state_dict()
    want = [(k, tuple(A if d == "A" else d for d in s)) for k, s in FX["state_dict"]]
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    torch.manual_seed(7)
    ref = _script_qnetwork(A)
    for k, v in ref.state_dict().items():
        assert torch.equal(sd["network." + k], v), k
    x = torch.randint(0, 256, (2, 4, 84, 84)).float()
    assert torch.equal(net(x), ref(x / 255.0))


def test_object_network_is_the_ppobj_stack_with_layernorms(pqn):
    from oc_cleanrl_amd.agents import EnvSpec, layer_init, object_trunk

    torch.manual_seed(3)
    net = pqn.PQNetwork(EnvSpec((4, 12), 6), "PQN_OBJ", None, (32, 16), (32,))
    torch.manual_seed(3)
    plain, d = object_trunk((4, 12), (32, 16), (32,), layer_init)
    head = layer_init(nn.Linear(d, 6))
    lins = [m for m in net.network if isinstance(m, nn.Linear)]
    for got, ref in zip(lins, [m for m in plain if isinstance(m, nn.Linear)] + [head]):
        assert torch.equal(got.weight, ref.weight) and torch.equal(got.bias, ref.bias)
    kinds = [type(m).__name__ for m in net.network]
    assert kinds == ["Linear", "LayerNorm", "ReLU"] * 2 + ["Flatten"] + \
        ["Linear", "LayerNorm", "ReLU", "Linear"]
    x = torch.randn(5, 4, 12)
    sd = {k: v for k, v in net.state_dict().items()}
    assert torch.allclose(net(x), U.q_network_ref(sd, x), rtol=0, atol=1e-6)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_radam_twin_equals_torch_optim(dtype):
    """The from-the-formula RAdam against torch.optim.RAdam on the CPU over 8 steps (steps 1-5
    un-rectified, 6-8 rectified): 1e-12 in f64; in f32 it was observed BITWISE equal here (torch
    2.10 CPU, single-tensor and foreach), asserted within 1 ulp."""
    torch.manual_seed(0)
    ps = [torch.randn(5, 3, dtype=dtype), torch.randn(70, dtype=dtype)]
    tp = [p.clone().requires_grad_() for p in ps]
    opt = torch.optim.RAdam(tp, lr=1e-2)
    ref = U.RAdamRef([p.clone() for p in ps], 1e-2)
    rect = []
    for _ in range(8):
        gs = [torch.randn_like(p) for p in ps]
        for p, g in zip(tp, gs):
            p.grad = g.clone()
        opt.step()
        rect.append(ref.step(gs) > 5.0)
        for p, q in zip(tp, ref.params):
            if dtype == torch.float64:
                assert float((p.detach() - q).abs().max()) <= 1e-12
            else:
                ulp = torch.finfo(dtype).eps * p.detach().abs().clamp_min(2.0 ** -126)
                assert bool(((p.detach() - q).abs() <= ulp).all())
    assert rect == [False] * 5 + [True] * 3


def test_q_lambda_twin_on_a_hand_case():
    """T = 3, N = 2, gamma = 0.5, lambda = 0.25, by hand (env 0 never done; env 1: dones[2] = 1,
    next_done = 1):
      env 0: R2 = 1 + 0.5 * max(4, 2)       = 3
             R1 = 2 + 0.5 * (0.25 * 3 + 0.75 * 8)    = 5.375
             R0 = 0 + 0.5 * (0.25 * 5.375 + 0.75 * 4) = 2.171875
      env 1: R2 = 1 (next_done), R1 = -1 (dones[2] cuts the tail),
             R0 = 3 + 0.5 * (0.25 * -1 + 0.75 * 2)   = 3.625"""
    rewards = torch.tensor([[0.0, 3.0], [2.0, -1.0], [1.0, 1.0]], dtype=torch.float64)
    values = torch.tensor([[9.0, 9.0], [4.0, 2.0], [8.0, 5.0]], dtype=torch.float64)
    dones = torch.tensor([[0.0, 0.0], [0.0, 0.0], [0.0, 1.0]], dtype=torch.float64)
    next_q = torch.tensor([[4.0, 2.0], [7.0, 6.0]], dtype=torch.float64)
    next_done = torch.tensor([0.0, 1.0], dtype=torch.float64)
    got = U.q_lambda_ref(rewards, values, dones, next_q, next_done, 0.5, 0.25)
    want = torch.tensor([[2.171875, 3.625], [5.375, -1.0], [3.0, 1.0]], dtype=torch.float64)
    assert torch.equal(got, want)
    # the literal transcription of :248-261 on the same tensors
    T = 3
    returns = torch.zeros_like(rewards)
    for t in reversed(range(T)):
        if t == T - 1:
            next_value, _ = torch.max(next_q, dim=-1)
            nextnonterminal = 1.0 - next_done
            returns[t] = rewards[t] + 0.5 * next_value * nextnonterminal
        else:
            nextnonterminal = 1.0 - dones[t + 1]
            next_value = values[t + 1]
            returns[t] = rewards[t] + 0.5 * (0.25 * returns[t + 1] + (1 - 0.25) * next_value) * nextnonterminal
    assert torch.equal(returns, want)


def test_schedule_twin(pqn):
    for t in (0, 1, 500, 1000, 5000):
        assert U.linear_schedule(1.0, 0.01, 1000.0, t) == pqn.linear_schedule(1.0, 0.01, 1000.0, t)
    assert U.linear_schedule(1.0, 0.01, 1000.0, 0) == 1.0
    assert U.linear_schedule(1.0, 0.01, 1000.0, 10_000) == 0.01


def test_abi_refuses_bad_arguments_and_takes_zero_sizes():
    from oc_cleanrl_amd import _lib

    L, d = _lib.LIB, ctypes.c_void_p(256)
    bad = _lib.OCPPO_E_INVALID
    # null pointers
    assert L.ocppo_q_lambda(None, None, None, None, None, None, 3, 2, 2, 0.99, 0.65, None) == bad
    assert b"ocppo_q_lambda: null pointer" in L.ocppo_last_error()
    assert L.ocppo_ln_relu_fwd(None, None, None, None, 4, 8, 1e-5, 1, None, None, None) == bad
    assert b"ocppo_ln_relu_fwd: null pointer" in L.ocppo_last_error()
    assert L.ocppo_ln_relu_bwd(None, d, d, None, d, d, d, 4, 8, 1, d, d, d, d, 1 << 20) == bad
    assert b"ocppo_ln_relu_bwd: null pointer" in L.ocppo_last_error()  # relu needs y
    assert L.ocppo_pqn_act(None, None, 4, 64, None, None, 6, 0, None, 0, 1.0, 0.1, 10.0, None,
                           None, None, None) == bad
    assert b"ocppo_pqn_act: null pointer" in L.ocppo_last_error()
    assert L.ocppo_pqn_loss_fwd_bwd(None, None, None, None, 4, 6, None, None) == bad
    assert b"ocppo_pqn_loss_fwd_bwd: null pointer" in L.ocppo_last_error()
    assert L.ocppo_clip_radam_step(None, None, None, None, None, 64, None, 0.9, 0.999, 1e-8, 1.0,
                                   10.0, None, None, 0, 0) == bad
    assert b"ocppo_clip_radam_step: null pointer" in L.ocppo_last_error()
    # bad shapes
    for E in (0, 1025):
        assert L.ocppo_ln_relu_fwd(None, d, d, d, 4, E, 1e-5, 1, d, d, d) == bad
        assert b"1 <= E <= 1024" in L.ocppo_last_error()
        assert L.ocppo_ln_relu_bwd(None, d, d, d, d, d, d, 4, E, 1, d, d, d, d, 1 << 20) == bad
        assert b"1 <= E <= 1024" in L.ocppo_last_error()
        assert L.ocppo_ln_relu_workspace_bytes(4, E) == 0
    assert L.ocppo_pqn_act(None, d, 4, 64, d, d, 19, 0, d, 0, 1.0, 0.1, 10.0, d, d, None,
                           None) == bad
    assert b"1 <= A <= 18" in L.ocppo_last_error()
    for H in (0, 6, 1028):
        assert L.ocppo_pqn_act(None, d, 4, H, d, d, 6, 0, d, 0, 1.0, 0.1, 10.0, d, d, None,
                               None) == bad
    assert L.ocppo_pqn_act(None, ctypes.c_void_p(260), 4, 64, d, d, 6, 0, d, 0, 1.0, 0.1, 10.0, d,
                           d, None, None) == bad
    assert b"16-B aligned" in L.ocppo_last_error()
    assert L.ocppo_pqn_loss_fwd_bwd(None, d, d, d, 4, 19, d, d) == bad
    assert b"1 <= A <= 18" in L.ocppo_last_error()
    assert L.ocppo_q_lambda(None, d, d, d, d, d, 3, 2, 0, 0.99, 0.65, d) == bad
    assert L.ocppo_clip_radam_step(None, d, d, d, d, 64, d, 0.9, 0.999, 1e-8, 1.0, 10.0, d, d,
                                   1 << 20, 1) == bad
    assert b"plane jobs" in L.ocppo_last_error()
    assert L.ocppo_clip_radam_step(None, d, d, d, d, 64, d, 0.9, 0.999, 1e-8, 1.0, 10.0, d, d, 8,
                                   0) == _lib.OCPPO_E_WORKSPACE
    assert L.ocppo_ln_relu_bwd(None, d, d, d, d, d, d, 4, 8, 1, d, d, d, d, 8) == \
        _lib.OCPPO_E_WORKSPACE
    # zero sizes launch nothing
    assert L.ocppo_q_lambda(None, None, None, None, None, None, 0, 4, 2, 0.99, 0.65, None) == 0
    assert L.ocppo_q_lambda(None, None, None, None, None, None, 4, 0, 2, 0.99, 0.65, None) == 0
    assert L.ocppo_ln_relu_fwd(None, None, None, None, 0, 8, 1e-5, 1, None, None, None) == 0
    assert L.ocppo_ln_relu_bwd(None, None, None, None, None, None, None, 0, 8, 1, None, None,
                               None, None, 0) == 0
    assert L.ocppo_pqn_act(None, None, 0, 64, None, None, 6, 0, None, 0, 1.0, 0.1, 10.0, None,
                           None, None, None) == 0
    assert L.ocppo_pqn_loss_fwd_bwd(None, None, None, None, 0, 6, None, None) == 0
    assert L.ocppo_clip_radam_step(None, None, None, None, None, 0, None, 0.9, 0.999, 1e-8, 1.0,
                                   10.0, None, None, 0, 0) == 0
