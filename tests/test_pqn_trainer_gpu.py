"""pqn.PQNTrainer end to end on the Synthetic object env (4 envs x 8 steps, 2 minibatches, 2
epochs, 2 iterations = 8 optimizer steps) and one pixel iteration."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import pqn_util as U

pytestmark = pytest.mark.gpu

N, T, NMB, EPOCHS, ITERS = 4, 8, 2, 2, 2


def _args(pqn, **kw):
    base = dict(num_envs=N, num_steps=T, num_minibatches=NMB, update_epochs=EPOCHS,
                encoder_dims=(32, 16), decoder_dims=(32,), total_timesteps=N * T * ITERS,
                exploration_fraction=0.5, save_model=False, seed=3)
    base.update(kw)
    return pqn.finalize(pqn.PQNArgs(**base))


def _run(dev, fused=True, graphs=True, ln_update=False):
    """ITERS iterations; per iteration the data the update consumed, and the end state."""
    from oc_cleanrl_amd import pqn

    old = pqn.FUSED_PQN, pqn.FUSED_LN_UPDATE
    pqn.FUSED_PQN, pqn.FUSED_LN_UPDATE = fused, ln_update
    try:
        tr = pqn.PQNTrainer(_args(pqn, cuda_graphs=graphs), dev, log=False)
        c = lambda t: t.detach().cpu().clone()  # noqa: E731
        out = dict(sd0={k: c(v) for k, v in tr.agent.state_dict().items()}, its=[], tr=tr)
        for _ in range(ITERS):
            m = tr.train_iteration()
            out["its"].append(dict(
                obs=c(tr.obs[:T]).float(), actions=c(tr.actions), returns=c(tr.returns),
                rewards=c(tr.rewards), values=c(tr.values[:T]), dones=c(tr.dones),
                next_q=c(tr.next_q), perm=c(tr.perm_dev), lr=float(tr.lr), metrics=m,
                eps=float(tr.epsilon)))
        torch.cuda.synchronize()
        out["sd"] = {k: c(v) for k, v in tr.agent.state_dict().items()}
        out["flat"] = c(tr.optimizer.params) if fused else None
        out["graphs_ready"] = tr.graphs_ready
        return out
    finally:
        pqn.FUSED_PQN, pqn.FUSED_LN_UPDATE = old


@pytest.fixture(scope="module")
def fused(dev):
    return _run(dev)


@pytest.fixture(scope="module")
def torch_path(dev):
    return _run(dev, fused=False, graphs=False)


def test_returns_are_bitwise_the_twin_and_metrics(fused):
    from oc_cleanrl_amd import pqn

    a = fused["tr"].args
    assert fused["graphs_ready"]
    for i, it in enumerate(fused["its"]):
        want = U.q_lambda_ref(it["rewards"], it["values"], it["dones"][:T], it["next_q"],
                              it["dones"][T], a.gamma, a.q_lambda)
        assert torch.equal(it["returns"], want)
        assert int(it["actions"].min()) >= 0 and int(it["actions"].max()) < fused["tr"].A
        m = it["metrics"]
        assert np.isfinite(m["losses/td_loss"]) and np.isfinite(m["losses/q_values"])
        want_eps = pqn.linear_schedule(a.start_e, a.end_e,
                                       a.exploration_fraction * a.total_timesteps,
                                       (i + 1) * T * N)
        assert abs(m["charts/epsilon"] - want_eps) <= 1e-6 and abs(it["eps"] - want_eps) <= 1e-6
    from oc_cleanrl_amd import ops

    assert isinstance(fused["tr"].optimizer, ops.FlatRAdam)
    assert float(fused["tr"].optimizer.scalars[0]) == ITERS * EPOCHS * NMB


def test_values_are_the_greedy_q_of_the_stored_observations(dev):
    """One rollout on the initial parameters: values[t] against the twin's max_a Q(obs[t])."""
    from oc_cleanrl_amd import pqn

    tr = pqn.PQNTrainer(_args(pqn, cuda_graphs=False), dev, log=False)
    sd = {k: v.detach().cpu().clone() for k, v in tr.agent.state_dict().items()}
    tr._load_staged()
    tr._rollout()
    torch.cuda.synchronize()
    obs = tr.obs[:T].float().cpu().view((T * N,) + tr.obs_shape)
    f32 = U.q_network_ref(sd, obs).max(1).values
    twin = U.q_network_ref({k: v.double() for k, v in sd.items()}, obs.double()).max(1).values
    U.check("values", tr.values[:T].reshape(-1), f32, twin)
    assert int(tr.actions.min()) >= 0 and int(tr.actions.max()) < tr.A


def _twin_update(run, dtype):
    """The update of pqn_atari_envpool.py:269-283 in `dtype` plain torch over the data each of
    `run`'s iterations consumed (its observations, actions, returns and permutation), from its
    initial parameters: the state dict after all iterations."""
    tr = run["tr"]
    p = {k: v.to(dtype).clone().requires_grad_() for k, v in run["sd0"].items()}
    ref = U.RAdamRef([v.detach() for v in p.values()], 0.0)
    M, B = tr.M, tr.B
    for it in run["its"]:
        ref.lr = it["lr"]
        obs = it["obs"].view((B,) + tr.obs_shape).to(dtype)
        acts, rets = it["actions"].view(-1), it["returns"].view(-1).to(dtype)
        for j in range(EPOCHS * NMB):
            idx = it["perm"][j * M:(j + 1) * M]
            q = U.q_network_ref(p, obs[idx])
            old = q.gather(1, acts[idx].unsqueeze(-1)).squeeze(-1)
            loss = torch.nn.functional.mse_loss(rets[idx], old)
            grads = torch.autograd.grad(loss, list(p.values()))
            c, _ = U.clip_coef(grads, tr.args.max_grad_norm)
            ref.step([g * c for g in grads])
            for v, new in zip(p.values(), ref.params):
                v.data.copy_(new)
    return {k: v.detach() for k, v in p.items()}


def test_fused_path_agrees_with_the_torch_path(fused, torch_path):
    """8 optimizer steps from one seed: both paths took the same actions, and every parameter of
    the fused path is within the rule of the f64 twin of the update (tests/pqn_util.py over the
    data the fused run consumed), the torch path's error against that twin being "torch's own"."""
    for a, b in zip(fused["its"], torch_path["its"]):
        assert torch.equal(a["actions"], b["actions"]) and torch.equal(a["obs"], b["obs"])
    twin = _twin_update(fused, torch.float64)
    for k in twin:
        U.check(f"params {k}", fused["sd"][k], torch_path["sd"][k], twin[k])


def test_update_layernorm_on_the_kernel_agrees_too(torch_path, dev):
    """FUSED_LN_UPDATE (off by default: measured slower) puts ops.ln_relu under autograd in the
    update: the same rule, and graphs on is bitwise graphs off there as well."""
    run = _run(dev, ln_update=True)
    for a, b in zip(run["its"], torch_path["its"]):
        assert torch.equal(a["actions"], b["actions"])
    twin = _twin_update(run, torch.float64)
    for k in twin:
        U.check(f"params (ln_relu in the update) {k}", run["sd"][k], torch_path["sd"][k], twin[k])
    assert torch.equal(_run(dev, graphs=False, ln_update=True)["flat"], run["flat"])


def test_graphs_off_and_a_second_run_are_bitwise_the_first(fused, dev):
    eager = _run(dev, graphs=False)
    again = _run(dev)
    assert not eager["graphs_ready"] and again["graphs_ready"]
    for other in (eager, again):
        assert torch.equal(other["flat"], fused["flat"])
        for a, b in zip(other["its"], fused["its"]):
            for k in ("returns", "actions", "values", "next_q"):
                assert torch.equal(a[k], b[k]), k
            assert a["metrics"]["losses/td_loss"] == b["metrics"]["losses/td_loss"]


def test_pixel_architecture_runs_an_iteration(dev):
    from oc_cleanrl_amd import pqn

    args = pqn.finalize(pqn.PQNArgs(architecture="PQN", obs_mode="dqn", num_envs=2, num_steps=4,
                                    num_minibatches=2, update_epochs=1, total_timesteps=8,
                                    save_model=False))
    tr = pqn.PQNTrainer(args, dev, log=False)
    m = tr.train_iteration()
    assert np.isfinite(m["losses/td_loss"]) and np.isfinite(m["losses/q_values"])
    assert [k for k in tr.agent.state_dict()][-1] == "network.13.bias"
