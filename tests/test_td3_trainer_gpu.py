"""td3.TD3Trainer end to end on the GPU (E = 2, batch 8, learning_starts 8, 32 steps; Pendulum-v1
and td3_util.StubEnv with A = 3, a non-zero action bias and terminations): the fused kernels
against plain torch, graphs against eager, DDPG against TD3, and the checkpoint."""
import pytest
import torch

import td3_util as U

pytestmark = pytest.mark.gpu

STEPS, LS = 32, 8
ADAM_STEP_PCT = 3e-6  # 1 % of an Adam step at lr 3e-4 (DESIGN 21.3's bound)


def _args(algo="td3", **kw):
    from oc_cleanrl_amd import ddpg, td3

    cls = td3.TD3Args if algo == "td3" else ddpg.DDPGArgs
    base = dict(num_envs=2, batch_size=8, learning_starts=float(LS), buffer_size=128,
                total_timesteps=STEPS, cuda_graphs=False)
    base.update(kw)
    return cls(**base)


def _run(dev, monkeypatch, algo="td3", env="pendulum", fused=True, steps=STEPS, prep=None, **kw):
    """A trainer after `steps` steps, with the actions it took and a snapshot of its state."""
    from oc_cleanrl_amd import td3

    monkeypatch.setattr(td3, "FUSED_TD3", fused)
    a = _args(algo, **kw)
    tr = td3.TD3Trainer(a, dev, log=False,
                        device_env=U.StubEnv(a.num_envs, dev) if env == "stub" else None)
    assert tr.fused is fused
    if prep is not None:
        prep(tr)
    pf = a.policy_frequency
    acts = []
    for _ in range(steps // pf):
        tr.steps(pf)
        acts.append(tr.actions.clone())  # the chunk's last action
    torch.cuda.synchronize()
    return tr, torch.stack(acts)


def _state(tr):
    rb = tr.rb
    return {"obs": rb.obs, "next_obs": rb.next_obs, "actions": rb.actions, "rewards": rb.rewards,
            "dones": rb.dones, "state": rb.state, "counter": rb.counter,
            "actor": tr.actor_opt.params, "q": tr.q_opt.params, "target_actor": tr.ta_flat,
            "target_q": tr.tq_flat, "q_stats": tr.q_stats, "pi_q": tr.pi_q}


REPLAY = ("obs", "next_obs", "actions", "rewards", "dones", "state", "counter")
PARAMS = ("actor", "q", "target_actor", "target_q")


@pytest.mark.parametrize("env", ["pendulum", "stub"])
@pytest.mark.parametrize("algo", ["td3", "ddpg"])
def test_fused_against_plain_torch(dev, monkeypatch, algo, env):
    on, acts_on = _run(dev, monkeypatch, algo, env, fused=True)
    off, acts_off = _run(dev, monkeypatch, algo, env, fused=False)
    assert torch.equal(acts_on, acts_off)
    s_on, s_off = _state(on), _state(off)
    for k in REPLAY:
        assert torch.equal(s_on[k], s_off[k]), k
    assert int(s_on["state"][0]) == STEPS and int(s_on["counter"]) == STEPS - LS - 1
    for k in PARAMS:
        d = float((s_on[k] - s_off[k]).abs().max())
        print(f"{algo} {env} {k}: max |fused - torch| = {d:.3g}")
        assert d <= ADAM_STEP_PCT, (k, d)
    assert not torch.equal(on.ta_flat, on.actor_opt.params)  # the run did train
    # the stub env terminated and was truncated; Pendulum is only ever truncated (not in 32 steps)
    dones = s_on["dones"][:STEPS]
    assert bool(dones.any()) is (env == "stub")
    m_on, m_off = on.metrics(), off.metrics()
    assert set(m_on) == set(m_off)
    names = {"losses/qf1_values", "losses/qf1_loss", "losses/actor_loss"}
    if algo == "td3":
        names |= {"losses/qf2_values", "losses/qf2_loss", "losses/qf_loss"}
    if env == "stub":
        names |= {"charts/episodic_return", "charts/episodic_length"}
    assert set(m_on) == names
    for k in names:
        assert abs(m_on[k] - m_off[k]) <= 1e-4 * max(1.0, abs(m_off[k])), k


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("algo,env,pf", [("td3", "pendulum", 2), ("td3", "stub", 3),
                                         ("ddpg", "stub", 2)])
def test_graphs_against_eager_bitwise(dev, monkeypatch, algo, env, pf, fused):
    """Across the learning_starts boundary: fill chunks (eager, captured, replayed), the eager
    chunk around step 8, train chunks (eager, captured, replayed)."""
    steps = STEPS - STEPS % pf
    eager, acts_e = _run(dev, monkeypatch, algo, env, fused, steps, policy_frequency=pf)
    graph, acts_g = _run(dev, monkeypatch, algo, env, fused, steps, policy_frequency=pf,
                         cuda_graphs=True)
    assert set(graph.graphs) == {"fill", "train"} and not eager.graphs
    assert torch.equal(acts_e, acts_g)
    for (k, a), b in zip(_state(eager).items(), _state(graph).values()):
        assert torch.equal(a, b), k
    assert eager.global_step == graph.global_step == steps
    assert int(graph.step_dev) == steps
    with pytest.raises(ValueError, match="multiple"):
        graph.steps(pf + 1)


def test_ddpg_differs_from_td3_only_as_the_scripts_do(dev, monkeypatch):
    td3_, _ = _run(dev, monkeypatch, "td3", "stub")
    ddpg_, _ = _run(dev, monkeypatch, "ddpg", "stub")
    assert not hasattr(ddpg_.q, "qf2") and ddpg_.dq2 is None
    assert len(td3_.checkpoint()) == 3 and len(ddpg_.checkpoint()) == 2
    # DDPG's four constructions draw less from the generator than TD3's six: same actor and qf1
    # initialisation, different training
    assert not torch.equal(td3_.actor_opt.params, ddpg_.actor_opt.params)
    # TD3 with policy_noise 0 differs from DDPG only through the second critic: with qf2 (and its
    # target) set to qf1 before the first step, min(q1t, q2t) is q1t and qf1's first update (step
    # 9, critics only) and first policy step (step 10) are bitwise DDPG's
    n = ddpg_.q_opt.params.numel()

    def twin_of_qf1(tr):
        assert tr.q_opt.params.numel() == 2 * n
        tr.q_opt.params[n:].copy_(tr.q_opt.params[:n])
        tr.tq_flat[n:].copy_(tr.tq_flat[:n])

    for steps in (LS + 2, LS + 4):
        t0, a_t = _run(dev, monkeypatch, "td3", "stub", steps=steps, policy_noise=0.0,
                       prep=twin_of_qf1)
        d0, a_d = _run(dev, monkeypatch, "ddpg", "stub", steps=steps)
        assert torch.equal(a_t, a_d)
        assert torch.equal(t0.q_opt.params[:n], d0.q_opt.params)
        assert torch.equal(t0.q_opt.params[n:], d0.q_opt.params)
        assert torch.equal(t0.actor_opt.params, d0.actor_opt.params)
        assert torch.equal(t0.tq_flat[:n], d0.tq_flat)
    init, _ = _run(dev, monkeypatch, "ddpg", "stub", steps=LS)
    assert not torch.equal(d0.q_opt.params, init.q_opt.params)  # the update happened


def test_checkpoint_loads_into_the_script_keyed_modules(dev, monkeypatch, tmp_path):
    from oc_cleanrl_amd import td3
    from oc_cleanrl_amd.dqn import run_learner

    monkeypatch.setattr(td3, "FUSED_TD3", True)
    a = _args("td3", log_dir=str(tmp_path), save_model=True, log_every=16, cuda_graphs=True)
    tr = run_learner(td3.TD3Trainer, a, dev)
    assert tr.global_step == STEPS
    path = next(tmp_path.rglob("*.cleanrl_model"))
    actor_sd, qf1_sd, qf2_sd = torch.load(path, map_location="cpu")
    spec = td3.box_spec(3, [-2.0], [2.0])
    actor, qf1, qf2 = td3.Actor(spec), td3.QNetwork(spec), td3.QNetwork(spec)
    actor.load_state_dict(actor_sd)
    qf1.load_state_dict(qf1_sd)
    qf2.load_state_dict(qf2_sd)
    import json

    from conftest import GOLDEN

    keys = json.loads((GOLDEN / "td3_state_keys.json").read_text())
    assert list(actor_sd) == list(keys["Actor"]) and list(qf1_sd) == list(keys["QNetwork"])
    obs = torch.tensor([[1.0, 0.0, 0.5]])
    with torch.no_grad():
        act = actor(obs)
        assert act.shape == (1, 1) and float(act.abs()) <= 2.0
        assert torch.equal(act, tr.actor.cpu()(obs))
        assert torch.equal(qf1(obs, act), tr.q.qf1.cpu()(obs, act))
    lines = (path.parent / "metrics.jsonl").read_text().splitlines()
    assert len(lines) == 2 and "losses/qf_loss" in lines[-1] and "losses/actor_loss" in lines[-1]
