"""Continuous-action PPO / RPO without a GPU: the flag surface and the agent against fixtures made
from cleanrl/ppo_continuous_action.py and rpo_continuous_action.py
(tests/golden/gen_golden_contppo.py), ContAgent's plain-torch update against the script's own
gradients, the refusals, the numpy twin of the wrapper chain on a hand-computed case, and the
host restatement of the RPO noise stream."""
import dataclasses
import json
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden

import contppo_util as cu
from oc_cleanrl_amd import contppo, rpo


def _json(name):
    return json.loads((GOLDEN / name).read_text())


# ---- surface ---------------------------------------------------------------------------------------------
def test_args_fields_and_defaults_match_the_script():
    ref = _json("contppo_args_fields.json")
    fields = {f.name: f.default for f in dataclasses.fields(contppo.ContPPOArgs)}
    names = [f.name for f in dataclasses.fields(contppo.ContPPOArgs)]
    own = [n for n in names if n in ref]
    assert own == list(ref), "the script's fields, in its order"
    for k, v in ref.items():
        if k == "env_id":  # declared: HalfCheetah-v4 needs MuJoCo
            assert (v, fields[k]) == ("HalfCheetah-v4", "Pendulum-v1")
        else:
            assert fields[k] == v, k
    assert fields["rpo_alpha"] == 0.0
    for k in ("backend", "cuda_graphs", "fused_optimizer", "log_dir", "metrics_every"):
        assert k in fields


def test_rpo_defaults_match_the_script():
    ref = _json("rpo_args_fields.json")
    args = contppo.ContPPOArgs(**rpo.RPO_DEFAULTS)
    for k, v in ref.items():
        if k == "env_id":
            assert (v, args.env_id) == ("HalfCheetah-v4", "Pendulum-v1")
        else:
            assert getattr(args, k) == v, k
    assert (args.exp_name, args.total_timesteps, args.rpo_alpha) == \
        ("rpo_continuous_action", 8_000_000, 0.5)


def test_finalize_sizes_and_checks():
    a = contppo.finalize(contppo.ContPPOArgs())
    assert (a.batch_size, a.minibatch_size, a.num_iterations) == (2048, 64, 488)
    with pytest.raises(NotImplementedError, match="one GPU"):
        contppo.finalize(contppo.ContPPOArgs(), world_size=2)
    with pytest.raises(ValueError, match="divisible"):
        contppo.finalize(contppo.ContPPOArgs(num_steps=33))
    with pytest.raises(ValueError, match="rpo_alpha"):
        contppo.finalize(contppo.ContPPOArgs(rpo_alpha=-0.1))


def test_agent_keys_shapes_and_seeded_init():
    ref = _json("contppo_state_keys.json")
    ag = contppo.ContAgent(contppo.cont_spec((1, 3), 1))
    sd = ag.state_dict()
    assert list(sd) == list(ref)
    assert {k: list(v.shape) for k, v in sd.items()} == ref
    assert ag.grads_in_place is False
    # the script's layer_init order (:112-129): critic first, then actor_mean, with its gains
    import torch.nn as nn

    from oc_cleanrl_amd.agents import layer_init

    torch.manual_seed(1000 * 33 + 6)
    ag = contppo.ContAgent(contppo.cont_spec((5,), 6))
    torch.manual_seed(1000 * 33 + 6)
    want = []
    for out, std in ((1, 1.0), (6, 0.01)):
        want += [layer_init(nn.Linear(5, 64)), layer_init(nn.Linear(64, 64)),
                 layer_init(nn.Linear(64, out), std=std)]
    got = [m for m in list(ag.critic) + list(ag.actor_mean) if isinstance(m, nn.Linear)]
    for g, w in zip(got, want):
        assert torch.equal(g.weight, w.weight) and torch.equal(g.bias, w.bias)
    assert torch.equal(ag.actor_logstd, torch.zeros(1, 6))
    w = ag.actor_mean[4].weight.detach()
    assert torch.allclose(w @ w.t(), 1e-4 * torch.eye(6), atol=1e-9)  # orthogonal rows, gain 0.01


FIXTURES = pytest.mark.parametrize("name", ["contppo_update_M64_A1.npz",
                                            "contppo_update_M33_A6.npz"])


def _plain_torch_update(name):
    """ContAgent (the fixture's stub parameters) + the update lines :265-300 in plain torch on the
    fixture's batch: (fixture, agent with .grad, fixture outputs, the loss terms)."""
    fx = golden(name)
    ag = cu.fixture_agent(fx)
    t, a, out = cu.load_update(fx)
    _, newlogprob, entropy, newvalue = ag.get_action_and_value(t["obs"], t["actions"])
    ratio = (newlogprob - t["logprobs"]).exp()
    adv = t["advantages"]
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    pg_loss = torch.max(-adv * ratio,
                        -adv * torch.clamp(ratio, 1 - a.clip_coef, 1 + a.clip_coef)).mean()
    newvalue = newvalue.view(-1)
    v_clipped = t["values"] + torch.clamp(newvalue - t["values"], -a.clip_coef, a.clip_coef)
    v_loss = 0.5 * torch.max((newvalue - t["returns"]) ** 2, (v_clipped - t["returns"]) ** 2).mean()
    loss = pg_loss - a.ent_coef * entropy.mean() + v_loss * a.vf_coef
    loss.backward()
    terms = {"loss": loss, "pg_loss": pg_loss, "v_loss": v_loss, "entropy_loss": entropy.mean()}
    return fx, ag, out, {k: v.detach().numpy() for k, v in terms.items()}


@FIXTURES
def test_plain_torch_update_equals_the_scripts_gradients(name):
    """Against the script's f32 run: every loss term and every element of every parameter
    gradient to 1 ulp of the tensor's largest element. Not bitwise: the 64-wide Linear layers run
    on the CPU's GEMM and the means on torch's vectorised sums, whose order depends on the host's
    vector width; with another width pg_loss was seen 3 ulp off (2.2e-8 against 7.5e-9) and loss 2
    ulp, and this test fails there. The bound is the one the learner's specification sets; the
    test below does not depend on the host."""
    fx, ag, out, terms = _plain_torch_update(name)

    def ulp1(name, got, want):
        got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
        tol = float(np.spacing(np.abs(want).max()))
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"{name}: {err:.3g} (1 ulp = {tol:.3g})")
        assert err <= tol, name

    for k, v in terms.items():
        ulp1(k, v, out["f32"][k])
    want = cu.split_grads(fx["f32_grads"], ag)
    for k, p in ag.named_parameters():
        ulp1("grad." + k, p.grad.numpy(), want[k])


@FIXTURES
def test_plain_torch_update_against_the_scripts_f64_run(name):
    """Every loss term and every gradient element against the script's f64 run under the project's
    rule (lstm_util.check), the script's own f32 run being "torch's own computation"."""
    fx, ag, out, terms = _plain_torch_update(name)
    own, twin = cu.split_grads(fx["f32_grads"], ag), cu.split_grads(fx["f64_grads"], ag)
    for k, v in terms.items():
        cu.check(k, v, out["f32"][k], out["f64"][k])
    for k, p in ag.named_parameters():
        cu.check("grad." + k, p.grad, own[k], twin[k])


# ---- refusals ----------------------------------------------------------------------------------------------
def test_trainer_refusals():
    args = contppo.finalize(contppo.ContPPOArgs(num_envs=2, num_steps=8, num_minibatches=2))
    with pytest.raises(NotImplementedError, match="one GPU"):
        contppo.ContPPOTrainer(args, "cpu", 0, 2)
    with pytest.raises(NotImplementedError, match="device env"):
        contppo.ContPPOTrainer(args, "cpu", envs=object())

    class Wide:
        n_actions = 65

    with pytest.raises(ValueError, match="at most 64"):
        contppo.ContPPOTrainer(args, "cpu", device_env=Wide())


# ---- the wrapper chain's twin ------------------------------------------------------------------------------
def _closed_form(samples, count0: float = 1e-4):
    """RunningMeanStd after merging `samples` one by one into (mean 0, var 1, count0), in rational
    arithmetic: population moments combine exactly, so with C = count0 + k, mean = sum / C and
    var = (count0 * 1 + sum of squares) / C - mean^2."""
    xs = [Fraction(float(x)) for x in samples]
    c0 = Fraction(count0)
    C = c0 + len(xs)
    mean = sum(xs) / C
    var = (c0 + sum(x * x for x in xs)) / C - mean * mean
    return float(mean), float(var), float(C)


def test_norm_chain_twin_three_steps_with_a_done():
    """One env, D = 1, gamma = 0.5: a plain step, a terminated step (terminal observation 3, reset
    observation -1: two statistics updates) and a plain step, against the closed form."""
    ch = cu.NormChainRef(1, 1, gamma=0.5)
    eps = 1e-8
    o0 = ch.reset(np.array([[0.25]], np.float32))
    m, v, c = _closed_form([0.25], 1e-4)
    assert o0[0, 0] == pytest.approx((0.25 - m) / np.sqrt(v + eps), rel=1e-12)

    o1, r1 = ch.step(np.array([[1.0]], np.float32), np.zeros((1, 1), np.float32), [2.0], [0], [0])
    m, v, c = _closed_form([0.25, 1.0], 1e-4)
    assert o1[0, 0] == pytest.approx((1.0 - m) / np.sqrt(v + eps), rel=1e-12)
    rets = [2.0]  # 0 * 0.5 * 1 + 2
    rm, rv, rc = _closed_form(rets, 1e-4)
    assert r1[0] == 10.0 < 2.0 / np.sqrt(rv + eps)  # the first return's variance is ~0: clipped

    o2, r2 = ch.step(np.array([[-1.0]], np.float32), np.array([[3.0]], np.float32), [0.5], [1], [0])
    m, v, c = _closed_form([0.25, 1.0, 3.0, -1.0], 1e-4)  # the terminal obs first, then the reset's
    assert ch.obs_rms[0].count == pytest.approx(c, rel=1e-15) and c == pytest.approx(4.0001)
    assert o2[0, 0] == pytest.approx((-1.0 - m) / np.sqrt(v + eps), rel=1e-12)
    rets.append(0.5)  # terminated: 2 * 0.5 * (1 - 1) + 0.5
    rm, rv, rc = _closed_form(rets, 1e-4)
    assert r2[0] == pytest.approx(0.5 / np.sqrt(rv + eps), rel=1e-12) and r2[0] < 10

    o3, r3 = ch.step(np.array([[0.5]], np.float32), np.zeros((1, 1), np.float32), [-1.0], [0], [0])
    m, v, c = _closed_form([0.25, 1.0, 3.0, -1.0, 0.5], 1e-4)
    assert o3[0, 0] == pytest.approx((0.5 - m) / np.sqrt(v + eps), rel=1e-12)
    rets.append(0.5 * 0.5 - 1.0)
    rm, rv, rc = _closed_form(rets, 1e-4)
    assert r3[0] == pytest.approx(-1.0 / np.sqrt(rv + eps), rel=1e-12)
    st = ch.state()
    assert st.shape == (1, 7)
    np.testing.assert_allclose(st[0], [m, v, c, rets[-1], rm, rv, rc], rtol=1e-12)


# ---- the RPO stream's restatement ---------------------------------------------------------------------------
def test_rpo_noise_ref_range_and_keys():
    z = cu.rpo_noise_ref(1, 0, 0, 64, 6, 0.5)
    assert z.dtype == torch.float32 and float(z.min()) >= -0.5 and float(z.max()) < 0.5
    assert abs(float(z.mean())) < 0.1
    assert not torch.equal(z, cu.rpo_noise_ref(1, 1, 0, 64, 6, 0.5))
    assert not torch.equal(z, cu.rpo_noise_ref(1, 0, 1, 64, 6, 0.5))
    assert not torch.equal(z, cu.rpo_noise_ref(2, 0, 0, 64, 6, 0.5))
    # Philox4x32-10's published known-answer vector (Random123 kat_vectors: counter and key of
    # all-ones words)
    assert cu.philox4x32_10([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == \
        [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
