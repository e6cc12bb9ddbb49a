"""ppg.PPGTrainer end to end on the Synthetic object env: PPG_OBJ, 4 envs x 8 steps, 2 policy
iterations a phase, 2 minibatches, 2 auxiliary epochs over minibatches of 2 rollouts, two phases,
small networks."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import ppg_util as U

pytestmark = pytest.mark.gpu

N, T, NMB, NIT, EAUX, K, PHASES = 4, 8, 2, 2, 2, 2, 2
R = N * NIT
PPO_NAMES = {"charts/learning_rate", "losses/value_loss", "losses/policy_loss", "losses/entropy",
             "losses/old_approx_kl", "losses/approx_kl", "losses/clipfrac",
             "losses/explained_variance"}
AUX_NAMES = {"losses/aux/kl_loss", "losses/aux/aux_value_loss", "losses/aux/real_value_loss"}


def _args(ppg, **kw):
    base = dict(num_envs=N, num_steps=T, num_minibatches=NMB, n_iteration=NIT, e_auxiliary=EAUX,
                num_aux_rollouts=K, encoder_dims=(32, 16), decoder_dims=(32,),
                total_timesteps=N * T * NIT * PHASES, save_model=False, seed=3)
    base.update(kw)
    return ppg.finalize(ppg.PPGArgs(**base))


def _run(dev, fused=True, graphs=True, phases=PHASES):
    """The run's record: per policy iteration the rollout and the update's inputs, per phase the
    state just before and just after the auxiliary phase."""
    from oc_cleanrl_amd import ppg

    old = ppg.FUSED_PPG
    ppg.FUSED_PPG = fused
    try:
        tr = ppg.PPGTrainer(_args(ppg, cuda_graphs=graphs), dev, log=False)
        c = lambda t: t.detach().cpu().clone()  # noqa: E731
        o = tr.optimizer

        def state():
            return dict(sd={k: c(v) for k, v in tr.agent.state_dict().items()},
                        flat=c(o.params), exp_avg=c(o.exp_avg), exp_avg_sq=c(o.exp_avg_sq),
                        scalars=c(o.scalars), aux_obs=c(tr.aux_obs),
                        aux_returns=c(tr.aux_returns), aux_pi=c(tr.aux_pi))

        out = dict(sd0=state(), its=[], pre=[], post=[], tr=tr)
        inner = tr.auxiliary_phase

        def recorded():
            out["pre"].append(state())
            m = inner()
            out["post"].append({**state(), "aux_perm": c(tr.aux_perm_all),
                                "aux_stats": c(tr.aux_stats)})
            return m

        tr.auxiliary_phase = recorded
        for _ in range(phases * NIT):
            m = tr.train_iteration()
            out["its"].append({**{k: c(getattr(tr, k)) for k in (
                "obs", "actions", "logprobs", "advantages", "returns", "values", "perm_dev",
                "stats", "full_stats")}, "lr": float(tr.lr), "metrics": m})
        torch.cuda.synchronize()
        out["graphs_ready"] = tr.graphs_ready and tr.g_aux is not None
        return out
    finally:
        ppg.FUSED_PPG = old


@pytest.fixture(scope="module")
def fused(dev):
    return _run(dev)


@pytest.fixture(scope="module")
def torch_path(dev):
    return _run(dev, fused=False, graphs=False, phases=1)


def test_graphs_on_is_bitwise_graphs_off(fused, dev):
    eager = _run(dev, graphs=False)
    assert fused["graphs_ready"] and not eager["graphs_ready"]
    for ph in range(PHASES):
        for when in ("pre", "post"):
            a, b = eager[when][ph], fused[when][ph]
            for k in ("flat", "exp_avg", "exp_avg_sq", "scalars", "aux_obs", "aux_returns",
                      "aux_pi"):
                assert torch.equal(a[k], b[k]), (ph, when, k)
        assert torch.equal(eager["post"][ph]["aux_stats"], fused["post"][ph]["aux_stats"])


def test_policy_phase_leaves_aux_critic_alone_and_fills_the_buffer(fused):
    from oc_cleanrl_amd import ops

    tr = fused["tr"]
    sp = tr.optimizer.split
    first, second = fused["pre"]
    # phase 1: aux_critic is its init, its moments zero, its count zero
    for k in ("aux_critic.weight", "aux_critic.bias"):
        assert torch.equal(first["sd"][k], fused["sd0"]["sd"][k]), k
    assert not bool(first["exp_avg"][sp:].any()) and not bool(first["exp_avg_sq"][sp:].any())
    assert float(first["scalars"][ops.OPT_TAIL_STEP]) == 0
    assert float(first["scalars"][ops.OPT_STEP]) == NIT * NMB == \
        float(first["scalars"][ops.OPT_TAIL_SKIPPED])
    # phase 2: bit-unchanged since the end of phase 1's auxiliary phase (moments now non-zero)
    after = fused["post"][0]
    assert bool(after["exp_avg"][sp:].any())
    for k in ("flat", "exp_avg", "exp_avg_sq"):
        assert torch.equal(second[k][sp:], after[k][sp:]), k
        assert not torch.equal(second[k][:sp], after[k][:sp]), k
    naux = EAUX * (R // K)
    assert float(after["scalars"][ops.OPT_TAIL_STEP]) == naux == \
        float(second["scalars"][ops.OPT_TAIL_STEP])
    assert float(second["scalars"][ops.OPT_STEP]) == 2 * NIT * NMB + naux
    # each iteration's rollout in its slice, in the rollout's storage dtype
    assert first["aux_obs"].dtype == fused["its"][0]["obs"].dtype
    for ph, pre in enumerate(fused["pre"]):
        for u in range(NIT):
            it = fused["its"][ph * NIT + u]
            assert torch.equal(pre["aux_obs"][:, N * u:N * (u + 1)], it["obs"][:T]), (ph, u)
            assert torch.equal(pre["aux_returns"][:, N * u:N * (u + 1)], it["returns"]), (ph, u)


def test_aux_pi_is_the_pre_auxiliary_policy_on_the_buffer(fused):
    for pre, post in zip(fused["pre"], fused["post"]):
        obs = U.flatten01(pre["aux_obs"])
        ref = []
        for dtype in (torch.float32, torch.float64):
            p = {k: v.to(dtype) for k, v in pre["sd"].items()}
            ref.append(U.agent_ref(p, obs.to(dtype))[0].view(T, R, -1))
        U.check("aux_pi", post["aux_pi"], ref[0], ref[1])
        assert torch.equal(post["aux_obs"], pre["aux_obs"])


def _twin_phase(run, dtype):
    """Phase 1 in `dtype` plain torch over the data the run consumed (its rollouts, shuffles and
    auxiliary buffer), from its initial parameters: torch.optim.Adam's steps with aux_critic's
    grad None through the policy iterations."""
    tr = run["tr"]
    a, M = tr.args, tr.M
    keys = list(run["sd0"]["sd"])
    p = {k: v.to(dtype).clone().requires_grad_() for k, v in run["sd0"]["sd"].items()}
    opt = U.SegAdamRef([p[k].detach() for k in keys], eps=1e-8)

    def step(loss, lr):
        grads = torch.autograd.grad(loss, [p[k] for k in keys], allow_unused=True)
        cc, _ = U.clip_coef([g for g in grads if g is not None], a.max_grad_norm)
        opt.lr = lr
        opt.step([None if g is None else g * cc for g in grads])
        for k, new in zip(keys, opt.params):
            p[k].data.copy_(new)

    for it in run["its"][:NIT]:
        c = lambda k: it[k].to(dtype)  # noqa: E731
        obs = c("obs")[:T].reshape((T * N,) + tuple(it["obs"].shape[2:]))
        adv = c("advantages").view(-1)
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)  # full batch (:345)
        acts, lps = it["actions"].view(-1), c("logprobs").view(-1)
        ret, val = c("returns").view(-1), c("values")[:T].reshape(-1)
        for j in range(NMB):
            idx = it["perm_dev"][j * M:(j + 1) * M]
            logits, value, _ = U.agent_ref(p, obs[idx])
            step(U.policy_loss_ref(logits, value, acts[idx], lps[idx], adv[idx], ret[idx],
                                   val[idx], a), it["lr"])
    assert opt.ts[keys.index("aux_critic.weight")] == 0
    pre, post = run["pre"][0], run["post"][0]
    aux_obs, aux_ret = pre["aux_obs"].to(dtype), pre["aux_returns"].to(dtype)
    with torch.no_grad():
        aux_pi = U.agent_ref(p, U.flatten01(aux_obs))[0].view(T, R, -1)
    for e in range(EAUX):
        for i in range(R // K):
            cols = post["aux_perm"][e * R + i * K:e * R + (i + 1) * K]
            logits, value, aux = U.agent_ref(p, U.flatten01(aux_obs[:, cols]))
            kl, al, rl = U.aux_losses(logits, value.view(-1), aux.view(-1),
                                      U.flatten01(aux_pi[:, cols]), U.flatten01(aux_ret[:, cols]))
            step(al + a.beta_clone * kl + rl, run["its"][NIT - 1]["lr"])
    assert opt.ts[keys.index("aux_critic.weight")] == EAUX * (R // K)
    assert opt.ts[0] == NIT * NMB + EAUX * (R // K)
    return {k: p[k].detach() for k in keys}


def test_parameters_after_a_phase_follow_the_twin(fused, torch_path):
    """Every parameter after phase 1 (4 policy steps, 8 auxiliary steps): the fused path against
    the f64 twin over the data the fused run consumed, the FUSED_PPG = False run's error against
    that twin being torch's own."""
    for a, b in zip(fused["its"][:NIT], torch_path["its"]):
        assert torch.equal(a["actions"], b["actions"]) and torch.equal(a["obs"], b["obs"])
        assert torch.equal(a["perm_dev"], b["perm_dev"])
    assert torch.equal(fused["post"][0]["aux_perm"], torch_path["post"][0]["aux_perm"])
    twin = _twin_phase(fused, torch.float64)
    for k in twin:
        U.check(f"params {k}", fused["post"][0]["sd"][k], torch_path["post"][0]["sd"][k], twin[k])
    # the first policy minibatch's advantage statistics are the whole batch's
    adv = fused["its"][0]["advantages"].double().view(-1)
    U.check("full-batch adv stats", fused["its"][0]["full_stats"][0],
            torch.stack([adv.float().mean(), adv.float().std()]),
            torch.stack([adv.mean(), adv.std()]))


def test_metrics_carry_the_scripts_names(fused):
    for n, it in enumerate(fused["its"]):
        m = it["metrics"]
        assert PPO_NAMES <= set(m), PPO_NAMES - set(m)
        assert (AUX_NAMES <= set(m)) == ((n + 1) % NIT == 0), (n, set(m))
        assert all(np.isfinite(v) for v in m.values()), m
    tr = fused["tr"]
    assert tr.phase == PHASES and tr.update == 0
    assert tr.global_step == N * T * NIT * PHASES


def test_checkpoint_round_trips_agent_step_counts_and_phase_position(dev, tmp_path):
    from oc_cleanrl_amd import ops, ppg

    tr = ppg.PPGTrainer(_args(ppg, cuda_graphs=False), dev, log=False)
    for _ in range(NIT + 1):  # one phase and the next phase's first policy iteration
        tr.train_iteration()
    assert (tr.phase, tr.update) == (1, 1)
    path = tmp_path / "ppg.cleanrl_model"
    tr.save(path)
    ck = torch.load(path, weights_only=False)
    other = ppg.PPGTrainer(_args(ppg, cuda_graphs=False, seed=11), dev, log=False)
    assert (other.phase, other.update) == (0, 0)
    other.load_checkpoint(ck)
    for (k, v), w in zip(other.agent.state_dict().items(), tr.agent.state_dict().values()):
        assert torch.equal(v, w), k
    assert torch.equal(other.optimizer.scalars, tr.optimizer.scalars)
    assert float(other.optimizer.scalars[ops.OPT_STEP]) == (NIT + 1) * NMB + EAUX * (R // K)
    assert float(other.optimizer.tail_step) == EAUX * (R // K)
    assert torch.equal(other.optimizer.exp_avg, tr.optimizer.exp_avg)
    assert (other.phase, other.update) == (1, 1)
    assert torch.equal(other.aux_obs[:, :N], tr.aux_obs[:, :N])
    assert torch.equal(other.aux_returns[:, :N], tr.aux_returns[:, :N])
    fresh = ppg.PPGAgent(ppg.EnvSpec(tr.obs_shape, tr.A), "PPG_OBJ", None,
                         tr.args.encoder_dims, tr.args.decoder_dims)
    fresh.load_state_dict(ck["model_weights"])


def test_run_ppg_writes_metrics_and_a_checkpoint(dev, tmp_path):
    import json

    from oc_cleanrl_amd import ppg

    args = _args(ppg, total_timesteps=N * T * NIT, log_dir=str(tmp_path), save_model=True,
                 cuda_graphs=False)
    assert args.num_phases == 1
    tr = ppg.run_ppg(args, dev)
    assert tr.global_step == N * T * NIT and (tr.phase, tr.update) == (1, 0)
    run_dir = next(tmp_path.iterdir())
    lines = [json.loads(s) for s in (run_dir / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == NIT and lines[-1]["global_step"] == N * T * NIT
    assert PPO_NAMES | AUX_NAMES | {"charts/SPS"} <= set(lines[-1])
    assert not AUX_NAMES & set(lines[0])
    ck = torch.load(run_dir / "ppg_procgen_final.cleanrl_model", weights_only=False)
    assert list(ck["model_weights"]) == list(tr.agent.state_dict())
    assert ck["args"]["n_iteration"] == NIT


def test_trainer_refuses_what_the_scope_leaves_out(dev):
    from oc_cleanrl_amd import ppg

    args = ppg.finalize(ppg.PPGArgs(architecture="PPG", obs_mode="dqn", num_envs=2, num_steps=4,
                                    n_iteration=2, num_aux_rollouts=2, num_minibatches=1),
                        trainer=False)
    with pytest.raises(NotImplementedError):
        ppg.PPGTrainer(args, dev, log=False)
