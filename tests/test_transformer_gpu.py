"""The object-set transformer agent and its trainer on the GPU: the fused block path against the
fixtures made from the reference (hidden, logits, value and every parameter gradient under the
project's error rule), the switch back to torch's modules, one trainer update against CPU torch
autograd + torch.optim.Adam, hipGraph replay against eager execution, and the dropout > 0 route.
Run with -s for the (measured / torch's own) pairs."""
import copy

import numpy as np
import pytest
import torch

import transformer_util as tu
from conftest import golden

pytestmark = pytest.mark.gpu

FIXTURES = ("e32_max", "e128_mean", "e32_first_nomask")


def _agent(z, dev, dropout=0.0):
    from oc_cleanrl_amd.agents import EnvSpec
    from oc_cleanrl_amd.transformer import OCTransformerAgent

    ag = OCTransformerAgent(EnvSpec((int(z["S"]), int(z["F"])), int(z["n_actions"])),
                            int(z["emb_dim"]), int(z["num_heads"]), int(z["num_blocks"]),
                            bool(z["masking"]), int(z["num_obj"]), None,
                            pooling_type=str(z["pooling_type"]),
                            num_post_layers=int(z["num_post_layers"]), dropout=dropout)
    ag.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("p:")})
    return ag.to(dev).train()


def _loss_backward(ag, z, dev):
    x = torch.from_numpy(z["x"]).to(dev)
    hidden = ag.trunk(x)
    logits, value = ag.heads(hidden)
    loss = (logits * torch.from_numpy(z["wl"]).to(dev)).sum() + \
        (value * torch.from_numpy(z["wv"]).to(dev)).sum()
    ag.zero_grad()
    loss.backward()
    return hidden.detach(), logits.detach(), value.detach()


@pytest.mark.parametrize("ln_hip", [True, False])
@pytest.mark.parametrize("name", FIXTURES)
def test_fused_agent_matches_reference_fixture(dev, name, ln_hip, monkeypatch):
    from oc_cleanrl_amd import ops
    from oc_cleanrl_amd import transformer as T

    monkeypatch.setattr(T, "ADD_LAYERNORM_HIP", ln_hip)

    z, z64 = golden(f"transformer_{name}.npz"), golden(f"transformer_{name}_f64.npz")
    calls = {"mha": 0, "ln": 0}
    mha, ln = ops.mha, ops.add_layernorm
    monkeypatch.setattr(ops, "mha", lambda *a: (calls.__setitem__("mha", calls["mha"] + 1),
                                                mha(*a))[1])
    monkeypatch.setattr(ops, "add_layernorm",
                        lambda *a: (calls.__setitem__("ln", calls["ln"] + 1), ln(*a))[1])
    ag = _agent(z, dev)
    hidden, logits, value = _loss_backward(ag, z, dev)
    nb = int(z["num_blocks"])
    assert calls == {"mha": nb, "ln": 2 * nb if ln_hip else 0}  # the fused path ran
    for k, got in (("hidden", hidden), ("logits", logits), ("value", value)):
        tu.check(f"{name} {k}", got, z[k], z64[k])
    for k, p in ag.named_parameters():
        if "g:" + k in z:
            tu.check(f"{name} g:{k}", p.grad, z["g:" + k], z64["g:" + k])
        else:
            assert p.grad is None, k


@pytest.mark.parametrize("name", FIXTURES[:1] + FIXTURES[2:])
def test_fused_path_off_is_torchs_modules(dev, name, monkeypatch):
    from oc_cleanrl_amd import transformer as T

    z = golden(f"transformer_{name}.npz")
    ag = _agent(z, dev)
    monkeypatch.setattr(T, "FUSED_ATTN", False)
    hidden, _, _ = _loss_backward(ag, z, dev)
    grads = {k: p.grad.clone() for k, p in ag.named_parameters() if p.grad is not None}
    x = torch.from_numpy(z["x"]).to(dev)
    mask = ag.valid_mask(x) if ag.masking else None
    h = ag.transformer(ag.encoder(x), src_key_padding_mask=None if mask is None else ~mask)
    ref = T.pool(ag.network(h) if ag.masking else h, mask, ag.pooling_type)
    assert torch.equal(hidden, ref.detach())
    assert any(k.endswith("norm1.weight") for k in grads)
    # and a dropout > 0 agent never takes the fused path
    assert not T.attn_ok(x, int(z["emb_dim"]), int(z["num_heads"]), 0.0)
    monkeypatch.setattr(T, "FUSED_ATTN", True)
    assert T.attn_ok(x, int(z["emb_dim"]), int(z["num_heads"]), 0.0)
    assert not T.attn_ok(x, int(z["emb_dim"]), int(z["num_heads"]), 0.1)


@pytest.fixture(params=[True, False], ids=["ln_hip", "ln_torch"])
def ln_hip(request, monkeypatch):
    """Both routes of the fused path's residual add + LayerNorm (transformer.ADD_LAYERNORM_HIP)."""
    from oc_cleanrl_amd import transformer as T

    monkeypatch.setattr(T, "ADD_LAYERNORM_HIP", request.param)
    return request.param


def _trainer(dev, **kw):
    from oc_cleanrl_amd.transformer import TransformerArgs, TransformerTrainer, finalize

    cfg = dict(num_envs=8, num_steps=8, buffer_window_size=6, num_features=8, emb_dim=32,
               num_heads=4, num_blocks=2, num_minibatches=2, update_epochs=2, dropout=0.0,
               total_timesteps=8 * 8 * 100, seed=7, save_model=False, gemm_table=False)
    cfg.update(kw)
    return TransformerTrainer(finalize(TransformerArgs(**cfg)), dev, log=False)


def _cpu_update(agent, dtype, obs, mb, perm, a, M, n_mb):
    """ppo_atari_oc_transformer.py's update block (the loop of ppo_atari_oc.py:566-605) on the
    CPU: torch autograd of the loss, clip_grad_norm_, torch.optim.Adam(eps=1e-5)."""
    ag = copy.deepcopy(agent).to("cpu", dtype).train()
    opt = torch.optim.Adam(ag.parameters(), lr=a.learning_rate, eps=1e-5)
    t = lambda k: mb[k].to(dtype)  # noqa: E731
    for j in range(n_mb):
        idx = perm[j * M:(j + 1) * M]
        sl = slice(j * M, (j + 1) * M)
        hidden = ag.trunk(obs[idx].to(dtype))
        logits, value = ag.actor(hidden), ag.critic(hidden)
        dist = torch.distributions.Categorical(logits=logits)
        logratio = dist.log_prob(mb["actions"][sl]) - t("logprobs")[sl]
        ratio = logratio.exp()
        adv = t("advantages")[sl]
        if a.norm_adv:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - a.clip_coef,
                                                         1 + a.clip_coef)).mean()
        v = value.view(-1)
        ret, old = t("returns")[sl], t("values")[sl]
        v_clipped = old + torch.clamp(v - old, -a.clip_coef, a.clip_coef)
        v_loss = 0.5 * torch.max((v - ret) ** 2, (v_clipped - ret) ** 2).mean()
        loss = pg - a.ent_coef * dist.entropy().mean() + v_loss * a.vf_coef
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ag.parameters(), a.max_grad_norm)
        opt.step()
    return dict(ag.named_parameters())


def test_trainer_update_matches_cpu_autograd_and_adam(dev, ln_hip):
    """One update (2 epochs x 2 minibatches, from a loaded permutation) of the fused path: every
    parameter's delta against CPU torch (f32) and its f64 twin, under the rule."""
    tr = _trainer(dev, cuda_graphs=False)
    a = tr.args
    assert tr.agent.grads_in_place is False and not tr.direct_grads and not tr.frame_cache
    with torch.no_grad():
        tr.exp_stream.claim(tr.T)
    tr._rollout()
    rng = np.random.RandomState(3)
    perm = np.concatenate([rng.permutation(tr.B) for _ in range(tr.E)])
    tr.load_permutation(perm)
    tr._prepare_minibatches()
    torch.cuda.synchronize()
    before = {k: p.detach().cpu().clone() for k, p in tr.agent.named_parameters()}
    agent0 = copy.deepcopy(tr.agent).cpu()
    obs = tr.b_obs.float().cpu()
    mb = {k: v.detach().cpu().clone() for k, v in tr.mb.items()}
    for e in range(tr.E):
        tr._update_epoch(e)
    torch.cuda.synchronize()
    assert np.isfinite(tr.stats.cpu().numpy()).all()
    n_mb = tr.E * tr.nmb
    p32 = _cpu_update(agent0, torch.float32, obs, mb, torch.from_numpy(perm), a, tr.M, n_mb)
    p64 = _cpu_update(agent0, torch.float64, obs, mb, torch.from_numpy(perm), a, tr.M, n_mb)
    for k, p in tr.agent.named_parameters():
        b = before[k]
        assert not torch.equal(p.detach().cpu(), b), k
        tu.check(f"delta {k}", p.detach().cpu().double() - b.double(),
                 p32[k].detach().double() - b.double(), p64[k].detach() - b.double())


def _state(tr):
    o = tr.optimizer
    return [p.detach().clone() for p in tr.params] + \
        [o.exp_avg.clone(), o.exp_avg_sq.clone(), tr.obs.clone(), tr.actions.clone(),
         tr.logprobs.clone(), tr.rewards.clone(), tr.dones.clone(), tr.values.clone(),
         tr.advantages.clone(), tr.returns.clone()]


def test_captured_iterations_match_eager_bitwise(dev, ln_hip):
    """Iterations 2 and 3 replayed as hipGraphs leave parameters, Adam moments and the rollout
    buffers bitwise equal to eager execution (the fused path is capturable and repeatable)."""
    runs = []
    for graphs in (True, False):
        tr = _trainer(dev, cuda_graphs=graphs)
        for _ in range(3):
            tr.train_iteration(collect_metrics=False)
        torch.cuda.synchronize()
        assert tr.graphs_ready == graphs
        runs.append(_state(tr))
        tr.close()
    assert all(torch.equal(x, y) for x, y in zip(*runs))


def test_dropout_trainer_runs_on_the_torch_path(dev, monkeypatch):
    """dropout = 0.1 (the reference's default): torch's layer modules, no parity claim -- two
    iterations with finite losses and moving parameters."""
    from oc_cleanrl_amd import ops

    def boom(*a):
        raise AssertionError("the fused attention path ran with dropout > 0")

    monkeypatch.setattr(ops, "mha", boom)
    tr = _trainer(dev, dropout=0.1)
    before = [p.detach().clone() for p in tr.params]
    for _ in range(2):
        m = tr.train_iteration()
    torch.cuda.synchronize()
    assert np.isfinite(tr.stats.cpu().numpy()).all() and np.isfinite(m["losses/value_loss"])
    assert all(not torch.equal(p, b) for p, b in zip(tr.params, before))
    tr.close()
