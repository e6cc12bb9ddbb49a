"""What the continuous-SAC tests share, in plain torch / NumPy (cleanrl/sac_continuous_action.py):

  * stub_networks / stub_batch / CASES: the update fixtures' parameters and batches (seeded CPU
    draws, the same bits on any machine, so they are not stored; the arrays are
    tests/golden/gen_golden_sac_continuous.py's);
  * update_ref: the package's modules run through the script's update in plain torch, any dtype;
  * assert_branches: the rows a fixture needs, asserted on the CPU;
  * the NumPy twins of the library's new streams (the Philox words of the acting and update
    streams; Box-Muller is td3_util's);
  * StubEnv, td3_util's.

Every observation has unit scale and the heads' gains keep |mean| small and r = O(2), so the heads'
own f32 rounding moves log_std by ~1e-7 (a log-std head driven into tanh's tails by large inputs
would carry its GEMM's cancellation error, 1e-5, into log_prob on any device whose GEMM sums in
another order than the reference's). The pre-squash x = mean + sigma z is placed by the recorded
draws z, formed from the stub actor's f64 sigma: an element of a "large" row (b % 3 != 0) with
sigma >= SIGMA_SPLIT has sigma |z| in [13.5, 16.5]; every other element has sigma |z| <= 3.
"""
from __future__ import annotations

import copy

import numpy as np
import torch

from lstm_util import FLOOR, bound, check, rel_err  # noqa: F401  (re-exported for the tests)
from rnd_util import MASK64
from td3_util import BOUNDS, M32, StubEnv, box_muller, philox_words, stub_parameters, unit24  # noqa: F401

CSAC_ACT_KEY = 0x5AC0C7A1D3E2F481
CSAC_UPDATE_KEY = 0x5AC0D9B7E6A3C215
TARGET_DRAW = 0

# the update fixtures: (B, A, D) and the hyper-parameters they were run with
CASES = [(64, 1, 3), (33, 6, 5)]
HYPER = dict(gamma=0.99, tau=0.005, q_lr=1e-3, log_alpha=-0.5)
NEAR = 1e-4
X_SMALL, X_LARGE = 4.0, 12.0
NETS = ("actor", "qf1", "qf2")
SKIP_GRADS = ("fc2.weight",)  # 65,536 elements each: fc2.bias and fc1.weight pin their factors
DRAWS = ("z_target", "z_pi", "z_alpha")  # Normal.rsample's three calls, in the script's order
# on the two heads' weights after the gain-2 stub, and added to fc_logstd's bias (r then reaches both
# of tanh's tails and enough elements have sigma >= SIGMA_SPLIT), chosen so that the script alone
# meets assert_branches with the generator's margin
MEAN_GAIN, LOGSTD_GAIN, LOGSTD_SHIFT = 1.0 / 16, {1: 2.0, 6: 1.0}, {1: -2.0, 6: 1.0}  # by A
SIGMA_SPLIT = 2.5


def large_rows(B: int):
    return torch.arange(B) % 3 != 0


def stub_networks(make, B: int, A: int):
    """The five networks with their stub parameters: make(name) constructs one ("actor" or "q").
    The second critics are close to the first ones, so that both min() take both inputs."""
    s = 2000 * B + 10 * A
    actor = stub_parameters(make("actor"), s + 1, 2.0)
    with torch.no_grad():
        actor.fc_mean.weight.mul_(MEAN_GAIN)
        actor.fc_logstd.weight.mul_(LOGSTD_GAIN[A])
        actor.fc_logstd.bias.add_(LOGSTD_SHIFT[A])
    nets = {"actor": actor,
            "qf1": stub_parameters(make("q"), s + 3, 2.0),
            "qf1_target": stub_parameters(make("q"), s + 4, 2.0)}
    nets["qf2"] = stub_parameters(make("q"), s + 5, 2.0, near=nets["qf1"])
    nets["qf2_target"] = stub_parameters(make("q"), s + 6, 2.0, near=nets["qf1_target"])
    return nets


def stub_batch(B: int, A: int, D: int, actor) -> dict:
    """The seeded batch of a fixture case; dones cycle 1, 0, 0, 0; three recorded draws z_target
    (on next_obs), z_pi, z_alpha (on obs) placed by `actor`'s f64 sigma (the module docstring)."""
    g = torch.Generator().manual_seed(B + 7 * A)
    low, high = (torch.tensor(v) for v in BOUNDS[A])
    t = {"obs": torch.randn(B, D, generator=g), "next_obs": torch.randn(B, D, generator=g),
         "actions": low + (high - low) * torch.rand(B, A, generator=g),
         "rewards": torch.randn(B, generator=g),
         "dones": (torch.arange(B) % 4 == 0).float(), "low": low, "high": high}
    big = large_rows(B)[:, None]
    ac = copy.deepcopy(actor).double()
    for k in DRAWS:
        u = torch.rand(B, A, generator=g).double()
        sign = torch.where(torch.rand(B, A, generator=g) < 0.5, -1.0, 1.0).double()
        with torch.no_grad():
            _, r = heads(ac, t["next_obs" if k == "z_target" else "obs"].double())
            sigma = torch.exp(-5 + 3.5 * (torch.tanh(r) + 1))
        assert float((sigma - SIGMA_SPLIT).abs().min()) > 1e-3  # no element sits on the split
        far = big & (sigma >= SIGMA_SPLIT)
        t[k] = (sign * torch.where(far, (13.5 + 3.0 * u) / sigma,
                                   u * torch.clamp(3.0 / sigma, max=1.0))).float()
    return t


def package_networks(B: int, A: int, D: int) -> dict:
    from oc_cleanrl_amd import sac_continuous as sc

    spec = sc.box_spec(D, *BOUNDS[A])
    return stub_networks(lambda k: sc.Actor(spec) if k == "actor" else sc.QNetwork(spec), B, A)


def package_case(B: int, A: int, D: int):
    """(stub networks, stub batch) of a fixture case on the package's modules."""
    nets = package_networks(B, A, D)
    return nets, stub_batch(B, A, D, nets["actor"])


def grad_names(nets: dict):
    """(net, parameter) of every gradient a fixture holds, in order."""
    return [(n, k) for n in NETS for k, _ in nets[n].named_parameters() if k not in SKIP_GRADS]


def heads(actor, x):
    """(mean, r) of a script-keyed actor: fc_mean's and fc_logstd's outputs."""
    h = torch.relu(actor.fc2(torch.relu(actor.fc1(x))))
    return actor.fc_mean(h), actor.fc_logstd(h)


def adam_steps(log_alpha0: float, grads, lr: float, dtype):
    """log_alpha after each of torch.optim.Adam([log_alpha], lr)'s steps on the given gradients
    (CPU, `dtype`)."""
    la = torch.tensor([log_alpha0], dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([la], lr=lr)
    out = []
    for g in grads:
        la.grad = torch.as_tensor(g, dtype=dtype).reshape(1).clone()
        opt.step()
        out.append(la.detach().clone())
    return torch.cat(out)


def update_ref(nets: dict, t: dict, dtype, h: dict = HYPER) -> dict:
    """The script's update (:263-311) with policy_frequency = target_network_frequency = 1 on deep
    copies of `nets` cast to dtype, in the package's plain-torch statement
    (sac_continuous.squash), without the q / actor optimizer steps: the tensors the fixtures hold."""
    from oc_cleanrl_amd import sac_continuous as sc

    n = {k: copy.deepcopy(v).to(dtype) for k, v in nets.items()}
    c = {k: v.to(dtype) for k, v in t.items()}
    ac = n["actor"]
    A = c["actions"].shape[1]
    log_alpha = torch.tensor([h["log_alpha"]], dtype=dtype)
    alpha = log_alpha.exp()
    with torch.no_grad():
        na, nlp = sc.squash(*heads(ac, c["next_obs"]), c["z_target"], ac.action_scale, ac.action_bias)
        nq = torch.min(n["qf1_target"](c["next_obs"], na), n["qf2_target"](c["next_obs"], na)) \
            - alpha * nlp
        y = c["rewards"].flatten() + (1 - c["dones"].flatten()) * h["gamma"] * nq.view(-1)
    out = {"next_actions": na, "next_log_pi": nlp.view(-1), "next_q_value": y}
    qs = [n["qf1"](c["obs"], c["actions"]), n["qf2"](c["obs"], c["actions"])]
    for q in qs:
        q.retain_grad()
    losses = [torch.nn.functional.mse_loss(q.view(-1), y) for q in qs]
    sum(losses).backward()
    out["dq1"], out["dq2"] = qs[0].grad.view(-1), qs[1].grad.view(-1)
    grads = {(m, k): p.grad.clone() for m in ("qf1", "qf2") for k, p in n[m].named_parameters()}
    mean, r = heads(ac, c["obs"])
    mean.retain_grad()
    r.retain_grad()
    pi, lp = sc.squash(mean, r, c["z_pi"], ac.action_scale, ac.action_bias)
    actor_loss = (alpha * lp - torch.min(n["qf1"](c["obs"], pi), n["qf2"](c["obs"], pi))).mean()
    actor_loss.backward(inputs=list(ac.parameters()) + [mean, r])
    out["dmean"], out["dr"] = mean.grad, r.grad
    grads.update({("actor", k): p.grad for k, p in ac.named_parameters()})
    with torch.no_grad():
        _, lp2 = sc.squash(*heads(ac, c["obs"]), c["z_alpha"], ac.action_scale, ac.action_bias)
        shifted = lp2 + (-float(A))
        alpha_loss = (-alpha * shifted).mean()
        la = adam_steps(h["log_alpha"], [-alpha * shifted.mean()], h["q_lr"], dtype)
    out["temp"] = torch.cat([la, la.exp()])
    out["losses"] = torch.stack(losses + [actor_loss, alpha_loss]).detach()
    out["grads"] = torch.cat([grads[k].reshape(-1) for k in grad_names(nets)])
    tau = h["tau"]
    p, tp = n["qf1"].fc3.weight, n["qf1_target"].fc3.weight
    out["polyak"] = (tau * p.data + (1 - tau) * tp.data).reshape(-1)
    return {k: v.detach() for k, v in out.items()}


FIXTURE_KEYS = ("next_actions", "next_log_pi", "next_q_value", "losses", "dq1", "dq2", "dmean",
                "dr", "polyak", "temp", "grads")


def fixture_name(B: int, A: int) -> str:
    return f"sac_continuous_update_B{B}_A{A}.npz"


def assert_branches(t: dict, nets: dict, margin: float = 0.0):
    """The rows a continuous-SAC fixture needs, asserted on the CPU in f64: dones 0 and 1; for each
    of the three draws, r in both tanh tails, every pre-squash |x| below X_SMALL or above X_LARGE,
    at least a quarter of the rows all-small and a quarter with an element beyond X_LARGE; q1t -
    q2t and q1pi - q2pi of both signs and none within NEAR of zero. margin: widens the excluded
    band of |x| (the generator's, so that another machine's last bits cannot move a row)."""
    assert set(t["dones"].tolist()) == {0.0, 1.0}
    B = t["obs"].shape[0]
    d = {k: copy.deepcopy(v).double() for k, v in nets.items()}
    ac = d["actor"]
    with torch.no_grad():
        for zk, ok, q1, q2 in (("z_target", "next_obs", "qf1_target", "qf2_target"),
                               ("z_pi", "obs", "qf1", "qf2"), ("z_alpha", "obs", None, None)):
            o = t[ok].double()
            mean, r = heads(ac, o)
            ls = -5 + 3.5 * (torch.tanh(r) + 1)
            assert float(ls.min()) < -4.9 and float(ls.max()) > 1.9, (zk, ls.min(), ls.max())
            x = (mean + ls.exp() * t[zk].double()).abs()
            small, large = x < X_SMALL - margin, x > X_LARGE + margin
            assert bool((small | large).all()), (zk, x[~(small | large)])
            assert int(small.all(1).sum()) * 4 >= B and int(large.any(1).sum()) * 4 >= B, zk
            if q1 is None:
                continue
            act = torch.tanh(mean + ls.exp() * t[zk].double()) * ac.action_scale + ac.action_bias
            dq = d[q1](o, act) - d[q2](o, act)
            assert (dq < -NEAR).any() and (dq > NEAR).any() and float(dq.abs().min()) > NEAR, zk


# ---- the streams -----------------------------------------------------------------------------------------
def csac_words(key: int, seed: int, counter: int, draw: int, rows: int, A: int):
    """Words 0 and 1 of the block (row * 64 + a, counter's low 32 bits, draw) under seed ^ key,
    [rows, A, 2]."""
    return philox_words((seed & MASK64) ^ key, (draw << 32) | (counter & M32), rows, A)


def act_words(seed: int, t: int, E: int, A: int):
    return csac_words(CSAC_ACT_KEY, seed, t, 0, E, A)


def update_words(seed: int, counter: int, draw: int, B: int, A: int):
    return csac_words(CSAC_UPDATE_KEY, seed, counter, draw, B, A)
