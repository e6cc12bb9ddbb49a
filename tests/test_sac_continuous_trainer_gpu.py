"""sac_continuous.ContSACTrainer end to end on the GPU (E = 2, batch 8, learning_starts 8, 32 steps;
Pendulum-v1 and td3_util.StubEnv with A = 3, a non-zero action bias and terminations): the fused
kernels against plain torch, graphs against eager, the constant temperature, the soft update's
schedule and the checkpoint."""
import json

import pytest
import torch

import sac_continuous_util as U

pytestmark = pytest.mark.gpu

STEPS, LS = 32, 8


def _args(**kw):
    from oc_cleanrl_amd import sac_continuous as sc

    base = dict(num_envs=2, batch_size=8, learning_starts=float(LS), buffer_size=128,
                total_timesteps=STEPS, cuda_graphs=False)
    base.update(kw)
    return sc.ContSACArgs(**base)


def _run(dev, monkeypatch, env="pendulum", fused=True, steps=STEPS, every=None, **kw):
    """A trainer after `steps` steps, with the actions it took (the last of every `every` steps)."""
    from oc_cleanrl_amd import sac_continuous as sc

    monkeypatch.setattr(sc, "FUSED_CSAC", fused)
    a = _args(**kw)
    tr = sc.ContSACTrainer(a, dev, log=False,
                           device_env=U.StubEnv(a.num_envs, dev) if env == "stub" else None)
    assert tr.fused is fused
    every = every or tr.chunk_len
    acts = []
    for _ in range(steps // every):
        tr.steps(every)
        acts.append(tr.actions.clone())
    torch.cuda.synchronize()
    return tr, torch.stack(acts)


def _state(tr):
    rb, t = tr.rb, tr.temp
    return {"obs": rb.obs, "next_obs": rb.next_obs, "actions": rb.actions, "rewards": rb.rewards,
            "dones": rb.dones, "state": rb.state, "counter": rb.counter,
            "actor": tr.actor_opt.params, "q": tr.q_opt.params, "target_q": tr.tq_flat,
            "alpha": t.alpha, "log_alpha": t.log_alpha, "exp_avg": t.exp_avg,
            "exp_avg_sq": t.exp_avg_sq, "alpha_step": t.step, "q_stats": tr.q_stats,
            "pi_loss": tr.pi_loss, "alpha_loss": tr.alpha_loss}


REPLAY = ("obs", "next_obs", "actions", "rewards", "dones", "state", "counter")
PARAMS = ("actor", "q", "target_q", "alpha", "log_alpha")


@pytest.mark.parametrize("env", ["pendulum", "stub"])
def test_fused_against_plain_torch(dev, monkeypatch, env):
    """Actions and replay bitwise; the parameter buffers, alpha and log_alpha within the rule's
    floor of the plain-torch path (there is no f64 twin of a run: the off path is the reference,
    its own error 0). Measured on MI355X (max |on - off| / max |off|): 0 for all five on both envs
    (DESIGN 23.3): the off path differentiates sac_continuous.SquashTorch, the kernel's order."""
    on, acts_on = _run(dev, monkeypatch, env, fused=True)
    off, acts_off = _run(dev, monkeypatch, env, fused=False)
    assert torch.equal(acts_on, acts_off)
    s_on, s_off = _state(on), _state(off)
    for k in REPLAY:
        assert torch.equal(s_on[k], s_off[k]), k
    assert int(s_on["state"][0]) == STEPS and int(s_on["counter"]) == STEPS - LS - 1
    assert int(s_on["alpha_step"]) == int(s_off["alpha_step"]) == 2 * ((STEPS - 1) // 2 - LS // 2)
    errs = {k: U.rel_err(s_on[k], s_off[k]) for k in PARAMS}
    for k, e in errs.items():
        print(f"{env} {k}: max |fused - torch| / max |torch| = {e:.3g}")
    for k, e in errs.items():
        assert e <= U.bound(0.0), (k, e)
    assert not torch.equal(on.tq_flat, on.q_opt.params)  # the run did train
    assert float(on.temp.alpha) != 1.0
    dones = s_on["dones"][:STEPS]
    assert bool(dones.any()) is (env == "stub")
    m_on, m_off = on.metrics(), off.metrics()
    names = {"losses/qf1_values", "losses/qf2_values", "losses/qf1_loss", "losses/qf2_loss",
             "losses/qf_loss", "losses/actor_loss", "losses/alpha", "losses/alpha_loss"}
    if env == "stub":
        names |= {"charts/episodic_return", "charts/episodic_length"}
    assert set(m_on) == set(m_off) == names
    for k in names:
        assert abs(m_on[k] - m_off[k]) <= 1e-4 * max(1.0, abs(m_off[k])), k


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("env,pf,tnf", [("pendulum", 2, 1), ("stub", 3, 2)])
def test_graphs_against_eager_bitwise(dev, monkeypatch, env, pf, tnf, fused):
    """Across the learning_starts boundary: fill chunks (eager, captured, replayed), the eager
    chunk around step 8, train chunks (eager, captured, replayed)."""
    from oc_cleanrl_amd import sac_continuous as sc

    chunk = sc.chunk_length(pf, tnf)
    steps = STEPS - STEPS % chunk
    kw = dict(policy_frequency=pf, target_network_frequency=tnf)
    eager, acts_e = _run(dev, monkeypatch, env, fused, steps, every=chunk, **kw)
    graph, acts_g = _run(dev, monkeypatch, env, fused, steps, cuda_graphs=True, **kw)
    assert graph.chunk_len == chunk
    assert set(graph.graphs) == {"fill", "train"} and not eager.graphs
    assert torch.equal(acts_e, acts_g)
    for (k, a), b in zip(_state(eager).items(), _state(graph).values()):
        assert torch.equal(a, b), k
    assert eager.global_step == graph.global_step == steps
    assert int(graph.step_dev) == steps
    if chunk > 1:
        with pytest.raises(ValueError, match="multiple"):
            graph.steps(chunk + 1)


def test_autotune_off_keeps_alpha_at_the_flags_value(dev, monkeypatch):
    tr, _ = _run(dev, monkeypatch, "stub", alpha=0.3, autotune=False)
    t = tr.temp
    assert float(t.alpha) == pytest.approx(0.3) and float(t.log_alpha) == 0.0
    assert int(t.step) == 0 and float(t.exp_avg) == 0.0 and float(t.exp_avg_sq) == 0.0
    assert not torch.equal(tr.tq_flat, tr.q_opt.params)
    m = tr.metrics()
    assert m["losses/alpha"] == pytest.approx(0.3) and "losses/alpha_loss" not in m
    assert "losses/actor_loss" in m


def test_targets_move_only_on_target_network_frequency_steps(dev, monkeypatch):
    from oc_cleanrl_amd import sac_continuous as sc

    monkeypatch.setattr(sc, "FUSED_CSAC", True)
    tr = sc.ContSACTrainer(_args(policy_frequency=2, target_network_frequency=3), dev, log=False)
    moved = []
    for g in range(20):
        before = tr.tq_flat.clone()
        tr.steps(1)
        moved.append(not torch.equal(before, tr.tq_flat))
    assert moved == [g > LS and g % 3 == 0 for g in range(20)]


def test_checkpoint_loads_into_the_script_keyed_modules(dev, monkeypatch, tmp_path):
    from conftest import GOLDEN
    from oc_cleanrl_amd import sac_continuous as sc
    from oc_cleanrl_amd.dqn import run_learner

    monkeypatch.setattr(sc, "FUSED_CSAC", True)
    a = _args(log_dir=str(tmp_path), save_model=True, log_every=16, cuda_graphs=True)
    tr = run_learner(sc.ContSACTrainer, a, dev)
    assert tr.global_step == STEPS
    path = next(tmp_path.rglob("*.cleanrl_model"))
    actor_sd, qf1_sd, qf2_sd = torch.load(path, map_location="cpu")
    spec = sc.box_spec(3, [-2.0], [2.0])
    actor, qf1, qf2 = sc.Actor(spec), sc.QNetwork(spec), sc.QNetwork(spec)
    actor.load_state_dict(actor_sd)
    qf1.load_state_dict(qf1_sd)
    qf2.load_state_dict(qf2_sd)
    keys = json.loads((GOLDEN / "sac_continuous_state_keys.json").read_text())
    assert list(actor_sd) == list(keys["Actor"]) and list(qf1_sd) == list(keys["SoftQNetwork"])
    assert list(qf2_sd) == list(keys["SoftQNetwork"])
    obs = torch.tensor([[1.0, 0.0, 0.5]])
    with torch.no_grad():
        act, logp, mean_action = actor.get_action(obs)
        assert act.shape == (1, 1) and float(act.abs()) <= 2.0 and logp.shape == (1, 1)
        mean, log_std = actor(obs)
        m2, l2 = tr.actor.cpu()(obs)
        assert torch.equal(mean, m2) and torch.equal(log_std, l2)
        assert torch.equal(qf1(obs, act), tr.q.qf1.cpu()(obs, act))
        assert torch.equal(qf2(obs, act), tr.q.qf2.cpu()(obs, act))
    lines = (path.parent / "metrics.jsonl").read_text().splitlines()
    assert len(lines) == 2 and "losses/qf_loss" in lines[-1] and "losses/alpha" in lines[-1]
