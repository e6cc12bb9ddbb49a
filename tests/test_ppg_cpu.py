"""oc_cleanrl_amd.ppg without a GPU: the flag surface, the derived sizes and refusals, the agent's
keys and init, where the value gradient stops, and the twin's auxiliary loss."""
from __future__ import annotations

import dataclasses
import json

import pytest
import torch

import ppg_util as U
from conftest import GOLDEN


@pytest.fixture(scope="module")
def ppg():
    from oc_cleanrl_amd import ppg

    return ppg


def _agent(ppg, arch="PPG_OBJ", shape=(4, 12), A=6, **kw):
    from oc_cleanrl_amd.agents import EnvSpec

    torch.manual_seed(0)
    return ppg.PPGAgent(EnvSpec(shape, A), arch, None, **kw)


def test_args_fields_and_defaults_are_the_scripts(ppg):
    want = json.loads((GOLDEN / "ppg_args_fields.json").read_text())
    got = {f.name: f.default for f in dataclasses.fields(ppg.PPGArgs)}
    assert len(want) == 36
    for w in want:
        assert w["name"] in got, w["name"]
        assert got[w["name"]] == w["default"] and type(got[w["name"]]) is type(w["default"]), w
    # the script's order, in front of this package's fields
    assert list(got)[:len(want)] == [w["name"] for w in want]
    for name in ("n_iteration", "e_policy", "v_value", "e_auxiliary", "beta_clone",
                 "num_aux_rollouts", "n_aux_grad_accum", "adv_norm_fullbatch", "num_phases",
                 "aux_batch_rollouts", "backend", "obs_mode", "num_features", "cuda_graphs"):
        assert name in got, name


def test_finalize_derived_sizes_at_the_defaults(ppg):
    a = ppg.finalize(ppg.PPGArgs())
    assert a.batch_size == 64 * 256 and a.minibatch_size == 2048
    assert a.num_iterations == 25_000_000 // 16384 == 1525
    assert a.num_phases == 1525 // 32 == 47
    assert a.aux_batch_rollouts == 2048
    assert a.update_epochs == a.e_policy == 1 and a.local_num_envs == 64


@pytest.mark.parametrize("kw, world, exc, word", [
    (dict(v_value=2), 1, NotImplementedError, "v_value"),
    (dict(n_aux_grad_accum=2), 1, NotImplementedError, "n_aux_grad_accum"),
    (dict(num_envs=3, n_iteration=3, num_aux_rollouts=4, num_minibatches=1), 1, ValueError,
     "num_aux_rollouts"),
    (dict(), 2, NotImplementedError, "world_size"),
    (dict(architecture="PPG", obs_mode="dqn"), 1, NotImplementedError, "architecture"),
])
def test_finalize_refusals_name_the_field(ppg, kw, world, exc, word):
    with pytest.raises(exc, match=word):
        ppg.finalize(ppg.PPGArgs(**kw), world)


def test_pixel_architecture_builds_when_not_for_the_trainer(ppg):
    a = ppg.finalize(ppg.PPGArgs(architecture="PPG", obs_mode="dqn"), trainer=False)
    assert a.architecture == "PPG"
    ag = _agent(ppg, "PPG", (3, 16, 16), 15)
    keys = set(ag.state_dict())
    for k in ("network.0.conv.weight", "network.0.res_block0.conv0.weight",
              "network.2.res_block1.conv1.bias", "network.5.weight", "actor.weight",
              "critic.bias", "aux_critic.weight"):
        assert k in keys, k
    assert ag.network[5].weight.shape == (256, 32 * 2 * 2)
    w = ag.network[5].weight
    assert torch.allclose(w.norm(dim=1), torch.full((256,), 1.4), rtol=1e-5)
    with torch.no_grad():
        pi, v, av = ag.get_pi_value_and_aux_value(torch.randint(0, 255, (2, 3, 16, 16)).float())
    assert pi.logits.shape == (2, 15) and v.shape == av.shape == (2, 1)


def test_agent_keys_and_head_init(ppg):
    ag = _agent(ppg, encoder_dims=(16, 8), decoder_dims=(32,))
    assert list(ag.state_dict()) == [
        "network.0.weight", "network.0.bias", "network.2.weight", "network.2.bias",
        "network.5.weight", "network.5.bias", "actor.weight", "actor.bias", "critic.weight",
        "critic.bias", "aux_critic.weight", "aux_critic.bias"]
    for head, rows in ((ag.actor, 6), (ag.critic, 1), (ag.aux_critic, 1)):
        assert head.weight.shape == (rows, 32)
        n = head.weight.detach().norm(dim=1)
        assert float((n - 0.1).abs().max()) <= 4 * 2.0 ** -23, n
        assert not bool(head.bias.any())
    assert [id(p) for p in ag.head_parameters()] == [
        id(p) for n, p in ag.named_parameters() if not n.startswith("aux_critic")]


def _policy_loss(ppg, ag, vf_coef, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 160, (10, 4, 12), generator=g).float()
    _, lp, ent, v = ag.get_action_and_value(x, torch.randint(0, 6, (10,), generator=g))
    adv, ret = torch.randn(10, generator=g), torch.randn(10, generator=g)
    ratio = (lp - lp.detach() + 0.1 * torch.randn(10, generator=g)).exp()
    pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 0.8, 1.2)).mean()
    vl = 0.5 * ((v.view(-1) - ret) ** 2).mean()
    return pg - 0.01 * ent.mean() + vl * vf_coef


def test_value_loss_does_not_shape_the_trunk_in_the_policy_phase(ppg):
    ag = _agent(ppg, encoder_dims=(16, 8), decoder_dims=(32,))
    grads = []
    for vf in (0.5, 1.0):
        ag.zero_grad(set_to_none=True)
        _policy_loss(ppg, ag, vf).backward()
        assert ag.aux_critic.weight.grad is None and ag.aux_critic.bias.grad is None
        grads.append({n: p.grad.clone() for n, p in ag.named_parameters() if p.grad is not None})
    a, b = grads
    assert set(a) == {n for n, _ in ag.named_parameters() if not n.startswith("aux_critic")}
    for n in a:
        if n.startswith("critic"):
            assert torch.equal(b[n], 2 * a[n]) and bool(a[n].any()), n
        else:
            assert torch.equal(a[n], b[n]), n  # trunk and actor: no trace of the value loss
    # get_value, as in the script, does not detach
    ag.zero_grad(set_to_none=True)
    ag.get_value(torch.ones(2, 4, 12)).sum().backward()
    assert ag.network[0].weight.grad is not None and bool(ag.network[0].weight.grad.any())


def test_auxiliary_loss_reaches_every_parameter(ppg):
    ag = _agent(ppg, encoder_dims=(16, 8), decoder_dims=(32,))
    x = torch.randint(0, 160, (10, 4, 12)).float()
    pi, v, av = ag.get_pi_value_and_aux_value(x)
    old = torch.randn(10, 6)
    kl, al, rl = U.aux_losses(pi.logits, v.view(-1), av.view(-1), old, torch.randn(10))
    (al + kl + rl).backward()
    assert all(p.grad is not None and bool(p.grad.any()) for p in ag.parameters())
    assert torch.equal(ag.get_pi(x).logits, pi.logits)


@pytest.mark.parametrize("M, A", [(1, 1), (3, 6), (65, 18)])
def test_twin_aux_loss_is_kl_divergence_plus_two_mses(ppg, M, A):
    g = torch.Generator().manual_seed(M * 100 + A)
    new, old = (torch.randn((M, A), generator=g, dtype=torch.float64) * 3 for _ in range(2))
    v, av, ret = (torch.randn(M, generator=g, dtype=torch.float64) for _ in range(3))
    stats, dl, dv, da = U.aux_ref(new, v, av, old, ret, 0.7, torch.float64)
    td = torch.distributions
    kl = td.kl_divergence(td.Categorical(logits=old), td.Categorical(logits=new)).mean()
    mse = torch.nn.functional.mse_loss
    want = torch.stack([kl, 0.5 * mse(av, ret), 0.5 * mse(v, ret)])
    assert torch.allclose(stats, want, rtol=1e-14, atol=0)
    # the gradients the kernel writes in closed form
    p_new, p_old = torch.softmax(new, -1), torch.softmax(old, -1)
    assert torch.allclose(dl, 0.7 / M * (p_new - p_old), rtol=1e-10, atol=1e-16)
    assert torch.allclose(dv, (v - ret) / M, rtol=1e-12, atol=0)
    assert torch.allclose(da, (av - ret) / M, rtol=1e-12, atol=0)
    # ... and the capturable restatement the FUSED_PPG = False path runs is the same function
    got = ppg.aux_losses_torch(new, v, av, old, ret)
    assert torch.allclose(torch.stack(got), want, rtol=1e-13, atol=0)
