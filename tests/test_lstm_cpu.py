"""The recurrent PPO agent without a GPU: the flag surface, the seeded init, the torch path and the
float64 twin against the reference's fixtures (tests/golden/gen_golden_lstm.py), the environment-
wise minibatch indices, finalize's refusals, and the C-ABI's argument checks."""
from __future__ import annotations

import ctypes
import dataclasses
import json

import numpy as np
import pytest
import torch

import lstm_util as U
from conftest import GOLDEN, golden

NAME = "lstm_ref_t4b3_mixed"


@pytest.fixture(scope="module")
def fx():
    return golden(NAME + ".npz"), golden(NAME + "_f64.npz")


@pytest.fixture(scope="module")
def agent(fx):
    from oc_cleanrl_amd import lstm
    from oc_cleanrl_amd.agents import EnvSpec

    torch.manual_seed(int(fx[0]["seed"]))
    return lstm.LSTMAgent(EnvSpec((1, 84, 84), int(fx[0]["n_actions"])), "PPO")


def test_args_match_the_script():
    from oc_cleanrl_amd import lstm

    want = json.loads((GOLDEN / "lstm_args_fields.json").read_text())
    fields = dataclasses.fields(lstm.LSTMArgs)
    got = [[f.name, f.default] for f in fields[:len(want)]]
    assert got == want
    a = lstm.LSTMArgs()
    assert (a.architecture, a.lstm_hidden, a.vecnorm_reward) == ("PPO_OBJ", 128, False)
    assert not (a.rollout_frame_cache or a.rollout_fusion or a.update_frame_dedup)


def test_seeded_init_is_the_reference_bitwise(fx, agent):
    f32, _ = fx
    sd = agent.state_dict()
    assert list(sd) == [str(k) for k in f32["keys"]]
    for k, v in sd.items():
        want, got, s_want, s_got = U.packed(f32, "p:" + k, v.numpy())
        assert np.array_equal(want, got), k
        assert s_want == s_got, k


def _run(agent, f32, dtype):
    agent = agent.to(dtype)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dtype)  # noqa: E731
    hidden, (hT, cT) = agent.get_states(t(f32["x"]), (t(f32["h0"]), t(f32["c0"])), t(f32["done"]))
    logits, value = agent.actor(hidden), agent.critic(hidden)
    loss = (logits * t(f32["wl"])).sum() + (value * t(f32["wv"])).sum()
    agent.zero_grad()
    loss.backward()
    return dict(hidden=hidden, hT=hT, cT=cT, logits=logits, value=value, loss=loss)


def test_torch_path_reproduces_the_fixture(fx, agent):
    f32, _ = fx
    sd = {k: v.clone() for k, v in agent.state_dict().items()}
    out = _run(agent, f32, torch.float32)
    for k, v in out.items():
        np.testing.assert_allclose(v.detach().numpy(), f32[k], rtol=2e-5, atol=2e-6, err_msg=k)
    for k, p in agent.named_parameters():
        want, got, s_want, s_got = U.packed(f32, "g:" + k, p.grad.numpy())
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * np.abs(want).max(), err_msg=k)
        if s_want is not None:  # a sampled tensor: its sum, at the elements' tolerance summed
            assert abs(s_got - s_want) <= 1e-5 * np.abs(want).max() * p.numel(), k
    # the reference's signatures and return values
    x = torch.from_numpy(f32["x"].astype(np.float32))
    st = (torch.from_numpy(f32["h0"]), torch.from_numpy(f32["c0"]))
    d = torch.from_numpy(f32["done"])
    act, lp, ent, val, st2 = agent.get_action_and_value(x, st, d)
    assert act.shape == lp.shape == ent.shape == (12,) and val.shape == (12, 1)
    assert st2[0].shape == st2[1].shape == (1, 3, 128)
    assert agent.get_value(x, st, d).shape == (12, 1)
    agent.load_state_dict(sd)


def test_twin_matches_the_f64_fixture(fx, agent):
    f32, f64 = fx
    p = {k: v.detach().double().requires_grad_() for k, v in agent.state_dict().items()}
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    hidden, hT, cT, logits, value = U.agent_ref(p, t(f32["x"]), t(f32["done"]), t(f32["h0"])[0],
                                                t(f32["c0"])[0], pixels=True)
    loss = (logits * t(f32["wl"])).sum() + (value * t(f32["wv"])).sum()
    loss.backward()
    for k, v in (("hidden", hidden), ("hT", hT.unsqueeze(0)), ("cT", cT.unsqueeze(0)),
                 ("logits", logits), ("value", value), ("loss", loss)):
        np.testing.assert_allclose(v.detach().numpy(), f64[k], rtol=1e-9, atol=1e-12, err_msg=k)
    for k, v in p.items():
        want, got, s_want, s_got = U.packed(f64, "g:" + k, v.grad.numpy())
        np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-11 * np.abs(want).max(),
                                   err_msg=k)
        if s_want is not None:
            assert abs(s_got - s_want) <= 1e-11 * np.abs(want).max() * v.numel(), k


def test_minibatch_indices_are_the_scripts(fx):
    from oc_cleanrl_amd import lstm

    f32, _ = fx
    want = f32["mb_inds"]  # [epochs, minibatches, T * envs / minibatches]
    E, nmb, per = want.shape
    rng = np.random.RandomState(int(f32["mb_seed"]))
    envinds = np.arange(8)
    for e in range(E):
        got = lstm.epoch_indices(envinds, rng, num_steps=4, num_minibatches=4)
        assert got.dtype == np.int64 and np.array_equal(got, want[e].reshape(-1))
        # time-major: a minibatch's first envs-per-minibatch entries are its environments
        assert np.array_equal(got.reshape(nmb, per)[:, :2].reshape(-1), envinds)


def test_finalize_refusals():
    from oc_cleanrl_amd import lstm

    ok = lstm.finalize(lstm.LSTMArgs(num_envs=8, num_minibatches=4))
    assert (ok.batch_size, ok.minibatch_size, ok.local_num_envs) == (1024, 256, 8)
    with pytest.raises(ValueError):
        lstm.finalize(lstm.LSTMArgs(num_envs=6, num_minibatches=4))
    with pytest.raises(NotImplementedError):
        lstm.finalize(lstm.LSTMArgs(), world_size=2)
    for h in (0, 16, 96, 256):
        with pytest.raises(ValueError):
            lstm.finalize(lstm.LSTMArgs(lstm_hidden=h))
    for h in (32, 64, 128):
        lstm.finalize(lstm.LSTMArgs(lstm_hidden=h))


def test_abi_refuses_bad_arguments_without_a_launch():
    from oc_cleanrl_amd import _lib

    L = _lib.LIB
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(T, B, H, ptr=p, opt=p):
        return L.ocppo_lstm_seq_fwd(None, ptr, p, p, p, p, p, T, B, H, p, opt, opt, opt, p, p)

    def bwd(T, B, H, ptr=p):
        return L.ocppo_lstm_seq_bwd(None, ptr, p, p, p, p, p, T, B, H, p)

    def step(N, I, H, ptr=p):
        return L.ocppo_lstm_step(None, ptr, p, p, p, p, p, N, I, H, p, p)

    bad = _lib.OCPPO_E_INVALID
    for H in (0, 16, 48, 256, -32):
        assert fwd(1, 1, H) == bad and b"hidden size" in L.ocppo_last_error()
        assert bwd(1, 1, H) == bad and step(1, 4, H) == bad
    assert fwd(-1, 1, 32) == bad and fwd(1, -1, 32) == bad
    assert bwd(-1, 1, 32) == bad and bwd(1, -1, 64) == bad
    assert step(-1, 4, 128) == bad and step(1, -4, 128) == bad and step(1, 0, 128) == bad
    assert fwd(1, 1, 32, ptr=None) == bad and b"null" in L.ocppo_last_error()
    assert bwd(1, 1, 32, ptr=None) == bad and step(1, 4, 32, ptr=None) == bad
    # zero sizes launch nothing, whatever the pointers
    assert fwd(0, 1, 32, ptr=None) == fwd(1, 0, 128, ptr=None) == _lib.OCPPO_OK
    assert bwd(0, 3, 64, ptr=None) == bwd(2, 0, 32, ptr=None) == _lib.OCPPO_OK
    assert step(0, 4, 32, ptr=None) == _lib.OCPPO_OK


def test_ops_refuse_cpu_tensors():
    from oc_cleanrl_amd import ops

    T, B, H, I = 2, 3, 32, 5
    z = torch.zeros
    with pytest.raises(ValueError):
        ops.lstm_seq(z(T, B, 4 * H), z(4 * H, H), z(4 * H), z(T, B), z(B, H), z(B, H))
    with pytest.raises(ValueError):
        ops.lstm_step(z(B, I), z(4 * H, I), z(4 * H), z(4 * H, H), z(4 * H), z(B), z(B, H),
                      z(B, H))
    with pytest.raises(ValueError):
        ops.lstm_seq_fwd(z(T, B, 4 * H), z(4 * H, H), z(4 * H), z(T, B), z(B, H), z(B, H))
    assert ops.lstm_shape_ok(128, 2, 512, 128) and ops.lstm_shape_ok(1, 1, 1, 32)
    assert not ops.lstm_shape_ok(0, 2, 512, 128) and not ops.lstm_shape_ok(4, 2, 512, 96)
    assert not ops.lstm_shape_ok(4, 0, 512, 64) and not ops.lstm_shape_ok(4, 2, 0, 64)
