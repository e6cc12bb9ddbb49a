"""rnd.RNDTrainer end to end on the Synthetic object env: RND_OBJ, 8 envs x 16 steps, 2
minibatches, 2 epochs, one warm-up round, small networks."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import rnd_util as U

pytestmark = pytest.mark.gpu

N, T, NMB, EPOCHS, ITERS = 8, 16, 2, 2, 3
NAMES = {"charts/learning_rate", "losses/value_loss", "losses/policy_loss", "losses/entropy",
         "losses/old_approx_kl", "losses/fwd_loss", "losses/approx_kl"}


def _args(rnd, **kw):
    base = dict(num_envs=N, num_steps=T, num_minibatches=NMB, update_epochs=EPOCHS,
                num_iterations_obs_norm_init=1, encoder_dims=(32, 16), decoder_dims=(32,),
                rnd_dims=(16, 16), rnd_feature_dim=32, total_timesteps=N * T * ITERS,
                save_model=False, seed=3)
    base.update(kw)
    return rnd.finalize(rnd.RNDArgs(**base))


def _run(dev, fused=True, graphs=True, iters=ITERS):
    from oc_cleanrl_amd import rnd

    old = rnd.FUSED_RND
    rnd.FUSED_RND = fused
    try:
        tr = rnd.RNDTrainer(_args(rnd, cuda_graphs=graphs), dev, log=False)
        c = lambda t: t.detach().cpu().clone()  # noqa: E731
        sd = lambda: {**{k: c(v) for k, v in tr.agent.state_dict().items()},  # noqa: E731
                      **{k: c(v) for k, v in tr.rnd.state_dict().items()}}
        out = dict(sd0=sd(), rms0=c(tr.obs_rms), its=[], tr=tr)
        for _ in range(iters):
            m = tr.train_iteration()
            out["its"].append({
                **{k: c(getattr(tr, k)) for k in (
                    "obs", "actions", "logprobs", "rewards", "dones", "values", "int_values",
                    "curiosity", "ext_advantages", "int_advantages", "advantages", "returns",
                    "int_returns", "rnd_obs", "obs_rms", "reward_rms", "rewems", "perm_dev",
                    "stats", "rstats")}, "lr": float(tr.lr), "metrics": m})
        torch.cuda.synchronize()
        out["sd"] = sd()
        out["flat"] = c(tr.optimizer.params)
        out["graphs_ready"] = tr.graphs_ready
        return out
    finally:
        rnd.FUSED_RND = old


@pytest.fixture(scope="module")
def fused(dev):
    return _run(dev)


@pytest.fixture(scope="module")
def torch_path(dev):
    return _run(dev, fused=False, graphs=False, iters=1)


def test_graphs_on_is_bitwise_graphs_off(fused, dev):
    eager = _run(dev, graphs=False)
    assert fused["graphs_ready"] and not eager["graphs_ready"]
    assert torch.equal(eager["flat"], fused["flat"])
    for a, b in zip(eager["its"], fused["its"]):
        for k in ("curiosity", "advantages", "returns", "int_returns", "rnd_obs", "obs_rms",
                  "reward_rms", "rstats"):
            assert torch.equal(a[k], b[k]), k


def test_target_frozen_predictor_trained_metrics_named(fused):
    sd0, sd = fused["sd0"], fused["sd"]
    for k in sd:
        if k.startswith("target."):
            assert torch.equal(sd0[k], sd[k]), k
    assert any(not torch.equal(sd0[k], sd[k]) for k in sd if k.startswith("predictor."))
    assert all(not torch.equal(sd0[k], sd[k]) for k in sd if k.startswith("predictor.")
               and k.endswith("weight"))
    tr = fused["tr"]
    assert not any(p is q for p in tr.rnd.target.parameters() for q in tr.params)
    for it in fused["its"]:
        m = it["metrics"]
        assert NAMES <= set(m), NAMES - set(m)
        assert all(np.isfinite(v) for v in m.values()), m
        assert int(it["actions"].min()) >= 0 and int(it["actions"].max()) < tr.A
    assert int(tr.mask_counter) == ITERS * EPOCHS * NMB
    assert float(tr.optimizer.scalars[0]) == ITERS * EPOCHS * NMB


def _twin_rollout(run, dtype):
    """Iteration 1's rollout-end buffers recomputed in `dtype` from the run's own stored rollout
    (observations, rewards, dones), its initial parameters and its post-warm-up statistics."""
    tr, it = run["tr"], run["its"][0]
    a = tr.args
    p = {k: v.to(dtype) for k, v in run["sd0"].items()}
    obs = it["obs"].to(dtype)  # [T + 1, N, W, F], exact in bf16 / f32
    C = obs.shape[-1]
    rms0 = run["rms0"].numpy()
    newest = obs[:, :, -1].double().numpy()
    cur = []
    for t in range(T):
        x = torch.from_numpy(U.normalize_ref(newest[t + 1], rms0[:C], rms0[C:2 * C])).to(dtype)
        cur.append(U.curiosity_ref(U.rnd_features_ref(p, x, "predictor"),
                                   U.rnd_features_ref(p, x, "target")))
    cur = torch.stack(cur)
    per_env, rewems = [], torch.zeros(T, dtype=dtype)
    for n in range(N):
        rewems = rewems * (float(np.float32(a.int_gamma)) if dtype == torch.float32
                           else a.int_gamma) + cur[:, n]
        per_env.append(rewems)
    pe = torch.stack(per_env).double().numpy()
    rstate = U.reward_stats_np((0.0, 1.0, 1e-4), pe)
    cur = cur / float(np.sqrt(rstate[1]))
    _, ve, vi = U.agent_ref(p, obs.view((-1,) + tuple(obs.shape[2:])))
    ve, vi = ve.view(T + 1, N), vi.view(T + 1, N)
    rewards, dones = it["rewards"].to(dtype), it["dones"].to(dtype)
    g = U.gae_ref(rewards, ve[:T], dones[:T], ve[T], dones[T], cur, vi[:T], vi[T], a.gamma,
                  a.int_gamma, a.gae_lambda, a.int_coef, a.ext_coef)
    st = U.rms_update_np((rms0[:C], rms0[C:2 * C], float(rms0[2 * C])),
                         newest[:T].reshape(T * N, C))
    rnd_obs = U.normalize_ref(newest[:T].reshape(T * N, C), st[0], st[1])
    return dict(curiosity=cur, ext_advantages=g[0], returns=g[1], int_advantages=g[2],
                int_returns=g[3], advantages=g[4], values=ve, int_values=vi,
                rnd_obs=torch.from_numpy(rnd_obs), obs_rms=np.concatenate([st[0], st[1], [st[2]]]),
                reward_rms=np.array(rstate))


def test_fused_path_agrees_with_the_torch_path(fused, torch_path):
    """One iteration from one seed: both paths took the same actions, and every buffer of the
    fused path is within the rule of the f64 twin (computed from the fused run's own rollout),
    the torch path's buffers being "torch's own"."""
    a, b = fused["its"][0], torch_path["its"][0]
    assert torch.equal(a["actions"], b["actions"]) and torch.equal(a["obs"], b["obs"])
    assert torch.equal(a["perm_dev"], b["perm_dev"])
    twin = _twin_rollout(fused, torch.float64)
    for k in ("values", "int_values", "curiosity", "ext_advantages", "int_advantages",
              "advantages", "returns", "int_returns", "rnd_obs"):
        U.check(k, a[k], b[k], twin[k])
    for k in ("obs_rms", "reward_rms"):  # f64 on both paths; the f32 rollout feeds reward_rms
        U.check(k, a[k], b[k], twin[k])
    # the loss statistics of the first minibatch (same parameters on both paths)
    U.check("rstats[0]", a["rstats"][0, :2], b["rstats"][0, :2], _twin_stats(fused, twin))
    assert float(a["rstats"][0, 2]) == float(b["rstats"][0, 2])


def _twin_stats(run, twin):
    """int_v_loss and fwd_loss of iteration 1's first minibatch in f64 on the twin's buffers."""
    tr, it = run["tr"], run["its"][0]
    a = tr.args
    p = {k: v.double() for k, v in run["sd0"].items()}
    idx = it["perm_dev"][:tr.M]
    x = twin["rnd_obs"][idx]
    mask = U.mask_ref(tr.seed, 0, tr.M, a.update_proportion)
    s, _, _ = U.aux_ref(U.rnd_features_ref(p, x, "predictor"), U.rnd_features_ref(p, x, "target"),
                        twin["int_values"][:T].reshape(-1)[idx],
                        twin["int_returns"].reshape(-1)[idx], mask, a.vf_coef, torch.float64)
    return s[:2]


def _twin_update(run, dtype):
    """Iteration 1's update (:457-521) in `dtype` plain torch over the data the run's update
    consumed (its rollout buffers, permutation and masks), from its initial parameters."""
    tr, it = run["tr"], run["its"][0]
    a, M = tr.args, tr.M
    keys = [k for k in run["sd0"] if not k.startswith("target.")]
    p = {k: v.to(dtype).clone() for k, v in run["sd0"].items()}
    for k in keys:
        p[k].requires_grad_()
    opt = U.AdamRef([p[k].detach() for k in keys])
    opt.lr = it["lr"]
    c = lambda k: it[k].to(dtype)  # noqa: E731
    obs = c("obs")[:T].reshape((T * N,) + tuple(it["obs"].shape[2:]))
    acts, lps = it["actions"].view(-1), c("logprobs").view(-1)
    adv, ret, val = c("advantages").view(-1), c("returns").view(-1), c("values")[:T].reshape(-1)
    iret, rnd_obs = c("int_returns").view(-1), c("rnd_obs")
    for j in range(EPOCHS * NMB):
        idx = it["perm_dev"][j * M:(j + 1) * M]
        logits, ve, vi = U.agent_ref(p, obs[idx])
        pf = U.rnd_features_ref(p, rnd_obs[idx], "predictor")
        tf = U.rnd_features_ref(p, rnd_obs[idx], "target").detach()
        mask = U.mask_ref(tr.seed, j, M, a.update_proportion).to(dtype)
        fl = torch.nn.functional.mse_loss(pf, tf, reduction="none").mean(-1)
        fwd = (fl * mask).sum() / torch.clamp(mask.sum(), min=1.0)
        int_v = 0.5 * ((vi.view(-1) - iret[idx]) ** 2).mean()
        loss = U.ppo_loss_ref(logits, ve, acts[idx], lps[idx], adv[idx], ret[idx], val[idx], a) \
            + int_v * a.vf_coef + fwd
        grads = torch.autograd.grad(loss, [p[k] for k in keys])
        cc, _ = U.clip_coef(grads, a.max_grad_norm)
        opt.step([g * cc for g in grads])
        for k, new in zip(keys, opt.params):
            p[k].data.copy_(new)
    return {k: p[k].detach() for k in keys}


def test_parameters_after_one_iteration_follow_the_twin_update(fused, torch_path, dev):
    """Every trained parameter after iteration 1's four optimizer steps: the fused path against
    the f64 twin of the update over the data the fused run consumed, the torch path's error
    against that twin being torch's own (the rule of the PQN and SAC trainer tests)."""
    one = _run(dev, iters=1)
    assert torch.equal(one["its"][0]["advantages"], fused["its"][0]["advantages"])
    twin = _twin_update(one, torch.float64)
    for k in twin:
        U.check(f"params {k}", one["sd"][k], torch_path["sd"][k], twin[k])


def test_checkpoint_round_trips_both_modules(fused, dev, tmp_path):
    from oc_cleanrl_amd import rnd
    from oc_cleanrl_amd.agents import EnvSpec

    tr = fused["tr"]
    path = tmp_path / "rnd.cleanrl_model"
    tr.save(path)
    ck = torch.load(path, weights_only=False)
    a = tr.args
    agent = rnd.RNDAgent(EnvSpec(tr.obs_shape, tr.A), a.architecture, None, a.encoder_dims,
                         a.decoder_dims)
    model = rnd.RNDModel(a.architecture, tr.obs_shape[-1], a.rnd_dims, a.rnd_feature_dim)
    agent.load_state_dict(ck["model_weights"])
    model.load_state_dict(ck["rnd_weights"])
    for k, v in {**agent.state_dict(), **model.state_dict()}.items():
        assert torch.equal(v, fused["sd"][k]), k
    assert torch.equal(ck["obs_rms"].cpu(), tr.obs_rms.cpu())
    other = rnd.RNDTrainer(_args(rnd, cuda_graphs=False, seed=11), dev, log=False)
    other.load_checkpoint(ck)
    for k, v in {**other.agent.state_dict(), **other.rnd.state_dict()}.items():
        assert torch.equal(v.cpu(), fused["sd"][k]), k
    assert torch.equal(other.reward_rms, tr.reward_rms)


def test_trainer_refuses_what_the_scope_leaves_out(dev):
    from oc_cleanrl_amd import rnd

    with pytest.raises(NotImplementedError):
        rnd.finalize(rnd.RNDArgs(architecture="RND", obs_mode="dqn"))
    with pytest.raises(NotImplementedError):
        rnd.finalize(rnd.RNDArgs(), world_size=2)
    args = rnd.finalize(rnd.RNDArgs(architecture="RND", obs_mode="dqn", num_envs=2, num_steps=4),
                        trainer=False)
    with pytest.raises(NotImplementedError):
        rnd.RNDTrainer(args, dev, log=False)
