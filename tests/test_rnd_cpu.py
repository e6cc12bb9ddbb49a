"""RND without a GPU: the flag surface and networks of ppo_rnd_envpool.py, the restatements of
tests/rnd_util.py pinned against a literal transcription of the script's loop, and the new C-ABI
entry points' validation."""
from __future__ import annotations

import ctypes
import dataclasses
import json

import numpy as np
import pytest
import torch

import rnd_util as U
from conftest import GOLDEN

FX = json.loads((GOLDEN / "rnd_args.json").read_text())


@pytest.fixture(scope="module")
def rnd():
    from oc_cleanrl_amd import rnd

    return rnd


def _spec(shape, A):
    from oc_cleanrl_amd.agents import EnvSpec

    return EnvSpec(shape, A)


def test_args_match_the_script(rnd):
    fields = dataclasses.fields(rnd.RNDArgs)
    ref = FX["fields"]
    assert [f.name for f in fields[:len(ref)]] == [n for n, _ in ref]
    a = rnd.RNDArgs()
    for n, d in ref:
        assert getattr(a, n) == d, n
    own = {f.name: f.default for f in fields[len(ref):]}
    assert own["architecture"] == "RND_OBJ" and own["obs_mode"] == "obj"
    assert own["backend"] == "Synthetic" and own["vecnorm_reward"] is False
    assert own["rnd_dims"] == (128, 128) and own["rnd_feature_dim"] == 512
    for n in ("rollout_frame_cache", "rollout_fusion", "rollout_cache_ring", "update_frame_dedup",
              "x6_weight_planes", "dp_overlap", "dp_exchange", "fused_heads_loss"):
        assert n not in own and getattr(a, n) is False, n
    assert rnd.ARCHITECTURES == ("RND_OBJ", "RND")
    b = rnd.parse_dataclass(rnd.RNDArgs, ["--int-coef", "0.5", "--rnd_dims", "64", "32"])
    assert b.int_coef == 0.5 and b.rnd_dims == (64, 32)


def test_finalize_sizes_and_refusals(rnd):
    a = rnd.finalize(rnd.RNDArgs(num_envs=6, num_steps=10, num_minibatches=4,
                                 total_timesteps=1000))
    assert (a.batch_size, a.minibatch_size, a.num_iterations) == (60, 15, 16)
    assert (a.local_num_envs, a.local_batch_size, a.local_minibatch_size) == (6, 60, 15)
    with pytest.raises(NotImplementedError, match="one GPU"):
        rnd.finalize(rnd.RNDArgs(), world_size=2)
    with pytest.raises(NotImplementedError, match="architecture"):
        rnd.finalize(rnd.RNDArgs(architecture="PPO_OBJ"))
    with pytest.raises(ValueError, match="obs_mode"):
        rnd.finalize(rnd.RNDArgs(architecture="RND"))
    with pytest.raises(NotImplementedError, match="RND_OBJ"):  # the pixel trainer path
        rnd.finalize(rnd.RNDArgs(architecture="RND", obs_mode="dqn"))
    rnd.finalize(rnd.RNDArgs(architecture="RND", obs_mode="dqn"), trainer=False)
    with pytest.raises(ValueError, match="update_proportion"):
        rnd.finalize(rnd.RNDArgs(update_proportion=1.5))
    with pytest.raises(ValueError, match="divisible"):
        rnd.finalize(rnd.RNDArgs(num_envs=3, num_steps=5, num_minibatches=4))


def test_state_dict_keys_and_shapes(rnd):
    ag = rnd.RNDAgent(_spec((4, 12), 6), "RND_OBJ", None, (32, 16), (24,))
    sd = {k: tuple(v.shape) for k, v in ag.state_dict().items()}
    assert sd == {"network.0.weight": (32, 12), "network.0.bias": (32,),
                  "network.2.weight": (16, 32), "network.2.bias": (16,),
                  "network.5.weight": (24, 64), "network.5.bias": (24,),
                  "extra_layer.0.weight": (24, 24), "extra_layer.0.bias": (24,),
                  "actor.0.weight": (24, 24), "actor.0.bias": (24,),
                  "actor.2.weight": (6, 24), "actor.2.bias": (6,),
                  "critic_ext.weight": (1, 24), "critic_ext.bias": (1,),
                  "critic_int.weight": (1, 24), "critic_int.bias": (1,)}
    m = rnd.RNDModel("RND_OBJ", 12, (16, 20), 32)
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.endswith("weight")}
    assert sd == {"predictor.0.weight": (16, 12), "predictor.2.weight": (20, 16),
                  "predictor.4.weight": (32, 20), "predictor.6.weight": (32, 32),
                  "predictor.8.weight": (32, 32), "target.0.weight": (16, 12),
                  "target.2.weight": (20, 16), "target.4.weight": (32, 20)}
    # the script's pixel networks
    ag = rnd.RNDAgent(_spec((4, 84, 84), 18), "RND")
    sd = {k: tuple(v.shape) for k, v in ag.state_dict().items() if k.endswith("weight")}
    assert sd == {"network.0.weight": (32, 4, 8, 8), "network.2.weight": (64, 32, 4, 4),
                  "network.4.weight": (64, 64, 3, 3), "network.7.weight": (256, 3136),
                  "network.9.weight": (448, 256), "extra_layer.0.weight": (448, 448),
                  "actor.0.weight": (448, 448), "actor.2.weight": (18, 448),
                  "critic_ext.weight": (1, 448), "critic_int.weight": (1, 448)}
    m = rnd.RNDModel("RND")
    sd = {k: tuple(v.shape) for k, v in m.state_dict().items() if k.endswith("weight")}
    assert sd == {"predictor.0.weight": (32, 1, 8, 8), "predictor.2.weight": (64, 32, 4, 4),
                  "predictor.4.weight": (64, 64, 3, 3), "predictor.7.weight": (512, 3136),
                  "predictor.9.weight": (512, 512), "predictor.11.weight": (512, 512),
                  "target.0.weight": (32, 1, 8, 8), "target.2.weight": (64, 32, 4, 4),
                  "target.4.weight": (64, 64, 3, 3), "target.7.weight": (512, 3136)}
    x = torch.zeros(2, 4, 84, 84)
    _, lp, ent, ve, vi = ag.get_action_and_value(x)
    assert lp.shape == ent.shape == (2,) and ve.shape == vi.shape == (2, 1)
    pf, tf = m(torch.zeros(2, 1, 84, 84))
    assert pf.shape == tf.shape == (2, 512) and pf.requires_grad and not tf.requires_grad


def test_seeded_init_is_reproducible_and_scaled(rnd):
    def build():
        torch.manual_seed(7)
        return (rnd.RNDAgent(_spec((4, 12), 6), "RND_OBJ", None, (32, 16), (24,)),
                rnd.RNDModel("RND_OBJ", 12, (16, 16), 32))

    (a1, m1), (a2, m2) = build(), build()
    for x, y in ((a1, a2), (m1, m2)):
        for (k, v), w in zip(x.state_dict().items(), y.state_dict().values()):
            assert torch.equal(v, w), k
    # orthogonal rows scaled by std: extra_layer 0.1, actor / critics 0.01, the rest sqrt(2)
    norm = lambda w: float(torch.linalg.matrix_norm(w.detach(), 2))  # noqa: E731
    assert abs(norm(a1.extra_layer[0].weight) - 0.1) < 1e-5
    assert abs(norm(a1.actor[0].weight) - 0.01) < 1e-6
    assert abs(norm(a1.critic_int.weight) - 0.01) < 1e-6
    assert abs(norm(m1.predictor[8].weight) - 2 ** 0.5) < 1e-5
    assert all(float(p.abs().max()) == 0 for k, p in a1.state_dict().items() if k.endswith("bias"))
    assert not torch.equal(m1.predictor[0].weight, m1.target[0].weight)


def test_target_is_frozen_and_outside_the_optimizer_list(rnd):
    ag = rnd.RNDAgent(_spec((4, 12), 6), "RND_OBJ", None, (32, 16), (24,))
    m = rnd.RNDModel("RND_OBJ", 12, (16, 16), 32)
    assert all(not p.requires_grad for p in m.target.parameters())
    assert all(p.requires_grad for p in m.predictor.parameters())
    params = rnd.combined_parameters(ag, m)
    assert [id(p) for p in params] == [id(p) for p in ag.parameters()] + \
        [id(p) for p in m.predictor.parameters()]
    assert not any(p is q for p in m.target.parameters() for q in params)
    pf, tf = m(torch.randn(5, 12))
    (pf - tf).pow(2).sum().backward()
    assert all(p.grad is None for p in m.target.parameters())
    assert all(p.grad is not None for p in m.predictor.parameters())


class _RunningMeanStd:
    """gym.wrappers.normalize.RunningMeanStd, transcribed."""

    def __init__(self, epsilon=1e-4, shape=()):
        self.mean, self.var, self.count = np.zeros(shape, "float64"), np.ones(shape, "float64"), epsilon

    def update_from_moments(self, batch_mean, batch_var, batch_count):
        delta = batch_mean - self.mean
        tot_count = self.count + batch_count
        new_mean = self.mean + delta * batch_count / tot_count
        m_a = self.var * self.count
        m_b = batch_var * batch_count
        M2 = m_a + m_b + np.square(delta) * self.count * batch_count / tot_count
        self.mean, self.var, self.count = new_mean, M2 / tot_count, tot_count


def test_restatement_of_steps_4_and_5_against_the_script_loop():
    """T = 4, N = 3, two rollouts: the script's lines :390-442 transcribed literally against
    rnd_util's reward_filter_np / reward_stats_np / gae_ref."""
    T, N = 4, 3
    g = torch.Generator().manual_seed(0)
    gamma, int_gamma, gae_lambda, int_coef, ext_coef = 0.999, 0.99, 0.95, 1.0, 2.0
    reward_rms, rewems_script = _RunningMeanStd(), None
    state, rewems = (0.0, 1.0, 1e-4), None
    for _ in range(2):
        curiosity_rewards = torch.rand((T, N), generator=g)
        rewards, ext_values, int_values = (torch.randn((T, N), generator=g) for _ in range(3))
        dones = (torch.rand((T, N), generator=g) < 0.3).float()
        next_done = (torch.rand(N, generator=g) < 0.5).float()
        next_value_ext, next_value_int = torch.randn((1, N), generator=g), torch.randn((1, N), generator=g)
        mine_cur = curiosity_rewards.clone()
        # ---- the script ----
        out = []
        for reward_per_step in curiosity_rewards.cpu().data.numpy().T:
            rewems_script = reward_per_step if rewems_script is None else \
                rewems_script * int_gamma + reward_per_step
            out.append(rewems_script)
        curiosity_reward_per_env = np.array(out)
        mean, std, count = (np.mean(curiosity_reward_per_env), np.std(curiosity_reward_per_env),
                            len(curiosity_reward_per_env))
        reward_rms.update_from_moments(mean, std ** 2, count)
        curiosity_rewards /= np.sqrt(reward_rms.var)
        ext_advantages, int_advantages = torch.zeros_like(rewards), torch.zeros_like(curiosity_rewards)
        ext_lastgaelam = int_lastgaelam = 0
        for t in reversed(range(T)):
            if t == T - 1:
                ext_nextnonterminal, int_nextnonterminal = 1.0 - next_done, 1.0
                ext_nextvalues, int_nextvalues = next_value_ext, next_value_int
            else:
                ext_nextnonterminal, int_nextnonterminal = 1.0 - dones[t + 1], 1.0
                ext_nextvalues, int_nextvalues = ext_values[t + 1], int_values[t + 1]
            ext_delta = rewards[t] + gamma * ext_nextvalues * ext_nextnonterminal - ext_values[t]
            int_delta = curiosity_rewards[t] + int_gamma * int_nextvalues * int_nextnonterminal - int_values[t]
            ext_advantages[t] = ext_lastgaelam = (
                ext_delta + gamma * gae_lambda * ext_nextnonterminal * ext_lastgaelam)
            int_advantages[t] = int_lastgaelam = (
                int_delta + int_gamma * gae_lambda * int_nextnonterminal * int_lastgaelam)
        ext_returns, int_returns = ext_advantages + ext_values, int_advantages + int_values
        b_advantages = int_advantages.reshape(-1) * int_coef + ext_advantages.reshape(-1) * ext_coef
        # ---- the restatement ----
        per_env, rewems = U.reward_filter_np(mine_cur.numpy(), rewems, int_gamma)
        assert np.array_equal(per_env, curiosity_reward_per_env)
        assert count == N  # len() of the [N, T] array
        state = U.reward_stats_np(state, per_env)
        # the script's moments are f32 (np.mean of an f32 array); the restatement's are f64
        assert abs(state[1] - reward_rms.var) <= 1e-6 * reward_rms.var
        assert state[2] == reward_rms.count
        mine_cur = mine_cur / float(np.sqrt(reward_rms.var))
        assert torch.allclose(mine_cur, curiosity_rewards, rtol=1e-6, atol=0)
        got = U.gae_ref(rewards, ext_values, dones, next_value_ext.view(-1), next_done,
                        curiosity_rewards, int_values, next_value_int.view(-1), gamma, int_gamma,
                        gae_lambda, int_coef, ext_coef)
        for a, b in zip(got, (ext_advantages, ext_returns, int_advantages, int_returns,
                              b_advantages.view(T, N))):
            assert torch.equal(a, b)
        state = (float(reward_rms.mean), float(reward_rms.var), float(reward_rms.count))


def test_rms_restatement_is_the_law_and_the_exact_twin_agrees():
    x = np.random.RandomState(0).randn(33, 5) * 3 + 2
    ref = _RunningMeanStd(shape=(5,))
    ref.update_from_moments(x.mean(0), x.var(0), x.shape[0])
    got = U.rms_update_np(U.rms_init(5), x)
    assert np.array_equal(got[0], ref.mean) and np.array_equal(got[1], ref.var)
    assert got[2] == ref.count
    twin, _ = U.rms_update_exact(U.rms_init(5), x)
    assert np.allclose(twin[0], got[0], rtol=1e-14) and np.allclose(twin[1], got[1], rtol=1e-13)


def test_mask_stream_restatement():
    m = U.mask_ref(1, 0, 4096, 0.25)
    assert 0.2 < float(m.mean()) < 0.3
    assert float(U.mask_ref(1, 0, 64, 0.0).sum()) == 0 and float(U.mask_ref(1, 0, 64, 1.0).sum()) == 64
    assert not torch.equal(m, U.mask_ref(1, 1, 4096, 0.25))
    assert not torch.equal(m, U.mask_ref(2, 0, 4096, 0.25))


def test_abi_argument_errors_arrive_without_a_launch():
    from oc_cleanrl_amd import _lib

    L, d = _lib.LIB, ctypes.c_void_p(64)
    big = 1 << 20
    calls = {
        "ocppo_rms_update": lambda x=d, C=3: L.ocppo_rms_update(None, x, 0, 4, C, 4, d, d, big),
        "ocppo_rnd_normalize": lambda x=d, C=3: L.ocppo_rnd_normalize(None, x, 0, 4, C, 4, d, d),
    }
    for name, fn in calls.items():
        assert fn(x=None) == _lib.OCPPO_E_INVALID and b"null pointer" in L.ocppo_last_error(), name
        assert fn(C=0) == _lib.OCPPO_E_INVALID and b"C=0" in L.ocppo_last_error(), name
    assert L.ocppo_rms_update(None, d, 7, 4, 3, 4, d, d, big) == _lib.OCPPO_E_INVALID
    assert b"dtype" in L.ocppo_last_error()
    assert L.ocppo_rms_update(None, d, 0, 4, 3, 2, d, d, big) == _lib.OCPPO_E_INVALID
    assert L.ocppo_rms_update(None, d, 0, 4, 3, 4, d, d, 8) == _lib.OCPPO_E_WORKSPACE
    assert L.ocppo_rnd_error(None, None, d, 4, 4, d) == _lib.OCPPO_E_INVALID
    assert L.ocppo_rnd_error(None, d, d, 4, 0, d) == _lib.OCPPO_E_INVALID
    assert L.ocppo_rnd_error(None, None, None, 0, 4, None) == _lib.OCPPO_OK
    assert L.ocppo_rnd_reward_norm(None, None, d, d, 4, 4, 0.99, d, big, None) == _lib.OCPPO_E_INVALID
    assert b"null pointer" in L.ocppo_last_error()
    assert L.ocppo_rnd_reward_norm(None, d, d, d, 0, 4, 0.99, d, big, None) == _lib.OCPPO_E_INVALID
    gae = lambda p: L.ocppo_rnd_gae(None, *([p] * 8), 4, 4, 0.999, 0.99, 0.95, 1.0, 2.0,  # noqa: E731
                                    *([p] * 5))
    assert gae(None) == _lib.OCPPO_E_INVALID and b"null pointer" in L.ocppo_last_error()
    aux = lambda p, prop, ws=big: L.ocppo_rnd_aux_loss_fwd_bwd(  # noqa: E731
        None, p, d, d, d, 4, 4, 1, d, prop, 0.5, d, d, d, d, ws)
    for prop in (-0.01, 1.01, float("nan")):
        assert aux(d, prop) == _lib.OCPPO_E_INVALID
        assert b"update_proportion" in L.ocppo_last_error()
    assert aux(None, 0.25) == _lib.OCPPO_E_INVALID and b"null pointer" in L.ocppo_last_error()
    assert aux(d, 0.25, 8) == _lib.OCPPO_E_WORKSPACE
    assert L.ocppo_rnd_mask(None, 1, d, 4, 2.0, d) == _lib.OCPPO_E_INVALID
    assert L.ocppo_rnd_mask(None, 1, None, 4, 0.5, d) == _lib.OCPPO_E_INVALID
    assert L.ocppo_rms_update_workspace_bytes(16384, 12) % 8 == 0
    assert L.ocppo_rms_update_workspace_bytes(4, 0) == 0
