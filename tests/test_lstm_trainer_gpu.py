"""LSTMTrainer on the synthetic env (4 envs x 8 steps, 2 minibatches x 2 epochs, lstm_hidden = 32,
a small PPObj trunk): captured against eager bitwise, the fused recurrence against the torch
loop and its float64 rerun under the rule of DESIGN.md 11, the carried state and its snapshot,
and the checkpoint."""
from __future__ import annotations

import copy
import io

import numpy as np
import pytest
import torch

import lstm_util as U

pytestmark = pytest.mark.gpu


def _trainer(dev, **kw):
    from oc_cleanrl_amd.lstm import LSTMArgs, LSTMTrainer, finalize

    cfg = dict(num_envs=4, num_steps=8, num_minibatches=2, update_epochs=2, lstm_hidden=32,
               encoder_dims=(32, 16), decoder_dims=(32,), buffer_window_size=4, num_features=8,
               total_timesteps=4 * 8 * 100, seed=11, save_model=False, gemm_table=False)
    cfg.update(kw)
    return LSTMTrainer(finalize(LSTMArgs(**cfg)), dev, log=False)


def _rolled(dev):
    """A trainer after one eager rollout, minibatches prepared from a fixed env-wise order."""
    from oc_cleanrl_amd.lstm import epoch_indices

    tr = _trainer(dev, cuda_graphs=False)
    with torch.no_grad():
        tr.exp_stream.claim(tr.T)
    tr._rollout()
    rng, envinds = np.random.RandomState(3), np.arange(tr.N)
    perm = np.concatenate([epoch_indices(envinds, rng, tr.T, tr.nmb) for _ in range(tr.E)])
    tr.load_permutation(perm)
    tr._prepare_minibatches()
    torch.cuda.synchronize()
    return tr, perm


def _first_minibatch(tr):
    tr._forward_backward(0)
    torch.cuda.synchronize()
    return tr.grad_buf.clone(), tr.stats[0].clone()


def test_captured_iterations_match_eager_bitwise(dev):
    runs = []
    for graphs in (True, False):
        tr = _trainer(dev, cuda_graphs=graphs)
        for _ in range(2):
            tr.train_iteration(collect_metrics=False)
        torch.cuda.synchronize()
        assert tr.graphs_ready == graphs
        runs.append([p.detach().clone() for p in tr.params] +
                    [tr.lstm_h.clone(), tr.lstm_c.clone(), tr.init_h.clone(), tr.init_c.clone(),
                     tr.values.clone(), tr.actions.clone()])
        tr.close()
    assert all(torch.equal(x, y) for x, y in zip(*runs))
    assert float(runs[0][-6].abs().max()) > 0  # the carried state is live


def _cpu_first_minibatch(tr, perm, dtype):
    """Minibatch 0 of ppo_atari_lstm.py:308-348 on the CPU in `dtype`: (flat gradient in the
    trainer's parameter order, [loss, pg_loss, v_loss, entropy, old_approx_kl, approx_kl])."""
    a, M, epb = tr.args, tr.M, tr.envs_per_mb
    ag = copy.deepcopy(tr.agent).to("cpu", dtype)
    idx = torch.from_numpy(perm[:M])
    t = lambda k: tr.mb[k][:M].detach().cpu().to(dtype)  # noqa: E731
    obs = tr.b_obs.float().cpu()[idx].to(dtype)
    envs = idx[:epb]
    state = (tr.init_h.cpu()[envs].to(dtype).unsqueeze(0),
             tr.init_c.cpu()[envs].to(dtype).unsqueeze(0))
    done = tr.dones[:tr.T].reshape(-1).cpu()[idx].to(dtype)
    hidden, _ = ag.recur(ag.trunk(obs), state, done)
    logits, value = ag.actor(hidden), ag.critic(hidden)
    dist = torch.distributions.Categorical(logits=logits)
    logratio = dist.log_prob(tr.mb["actions"][:M].cpu()) - t("logprobs")
    ratio = logratio.exp()
    adv = t("advantages")
    if a.norm_adv:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - a.clip_coef,
                                                     1 + a.clip_coef)).mean()
    v = value.view(-1)
    ret, old = t("returns"), t("values")
    v_clipped = old + torch.clamp(v - old, -a.clip_coef, a.clip_coef)
    v_loss = 0.5 * torch.max((v - ret) ** 2, (v_clipped - ret) ** 2).mean()
    ent = dist.entropy().mean()
    loss = pg - a.ent_coef * ent + v_loss * a.vf_coef
    ag.zero_grad()
    loss.backward()
    names = {id(p): k for k, p in tr.agent.named_parameters()}
    grads = dict(ag.named_parameters())
    flat = torch.cat([grads[names[id(p)]].grad.reshape(-1) for p in tr.params])
    stats = torch.stack([loss, pg, v_loss, ent, (-logratio).mean(),
                         ((ratio - 1) - logratio).mean()]).detach()
    return flat, stats


def test_fused_recurrence_matches_the_torch_loop_on_the_first_minibatch(dev, monkeypatch):
    from oc_cleanrl_amd import lstm, ops

    tr, perm = _rolled(dev)
    calls = []
    real = ops.lstm_seq
    monkeypatch.setattr(ops, "lstm_seq", lambda *a: (calls.append(1), real(*a))[1])
    g_fused, s_fused = _first_minibatch(tr)
    assert calls, "the fused path did not run"
    monkeypatch.setattr(lstm, "FUSED_LSTM", False)
    n = len(calls)
    g_torch, s_torch = _first_minibatch(tr)
    assert len(calls) == n, "FUSED_LSTM = False still took the fused path"
    g64, s64 = _cpu_first_minibatch(tr, perm, torch.float64)
    # the flat buffer pads every parameter to 64 floats: compare the parameters' own elements
    offs = ops.flat_offsets(tr.params)[0]
    pick = lambda buf: torch.cat([buf[o:o + p.numel()] for p, o in zip(tr.params, offs)])  # noqa: E731
    U.check("flat gradient", pick(g_fused), pick(g_torch), g64)
    for i, name in enumerate(("loss", "pg_loss", "v_loss", "entropy", "old_approx_kl",
                              "approx_kl")):
        U.check(name, s_fused[i], s_torch[i], s64[i])
    tr.close()


def test_state_is_carried_and_the_snapshot_feeds_the_update(dev):
    tr = _trainer(dev, cuda_graphs=False)
    tr.train_iteration(collect_metrics=False)
    torch.cuda.synchronize()
    assert bool((tr.init_h == 0).all()) and float(tr.lstm_h.abs().max()) > 0
    last_h, last_c = tr.lstm_h.clone(), tr.lstm_c.clone()
    tr.train_iteration(collect_metrics=False)
    torch.cuda.synchronize()
    # iteration 2 started from the state iteration 1's rollout ended in
    assert torch.equal(tr.init_h, last_h) and torch.equal(tr.init_c, last_c)
    assert not torch.equal(tr.lstm_h, last_h)
    tr.close()

    tr, _ = _rolled(dev)
    g0, s0 = _first_minibatch(tr)
    tr.lstm_h.add_(1.0)  # the live state is not what the update reads
    tr.lstm_c.sub_(1.0)
    g1, s1 = _first_minibatch(tr)
    assert torch.equal(g0, g1) and torch.equal(s0, s1)
    tr.init_h.add_(0.5)  # ... the snapshot is
    g2, _ = _first_minibatch(tr)
    assert not torch.equal(g0, g2)
    tr.close()


def test_checkpoint_round_trips(dev):
    from oc_cleanrl_amd.agents import EnvSpec
    from oc_cleanrl_amd.lstm import LSTMAgent

    tr = _trainer(dev, cuda_graphs=False)
    tr.train_iteration(collect_metrics=False)
    buf = io.BytesIO()
    torch.save(tr.state_dict_checkpoint(), buf)
    buf.seek(0)
    ck = torch.load(buf, map_location="cpu")
    a = tr.args
    assert ck["args"]["lstm_hidden"] == 32 and ck["Timesteps"] == a.batch_size
    fresh = LSTMAgent(EnvSpec(tr.obs_shape, tr.A), a.architecture, a.lstm_hidden, None,
                      a.encoder_dims, a.decoder_dims)
    fresh.load_state_dict(ck["model_weights"])
    for (k, p), (k2, q) in zip(tr.agent.state_dict().items(), fresh.state_dict().items()):
        assert k == k2 and torch.equal(p.cpu(), q), k
    assert [k.split(".")[0] for k in ck["model_weights"]][-8:] == ["lstm"] * 4 + ["actor"] * 2 + \
        ["critic"] * 2
    tr.close()
