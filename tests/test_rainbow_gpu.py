"""Rainbow on the GPU: the fused loss kernel against the fixtures made from the reference's own
loss block, greedy acting against torch, and RainbowTrainer (graph chunks vs stepwise execution,
one train step vs torch autograd + Adam on the CPU, priorities, target sync, beta, checkpoint)."""
import numpy as np
import pytest
import torch

from rainbow_util import (CHECKED, F32_FLOOR, LOSS_FIXTURES, bounds, check_elementwise,
                          dueling_dist, fixture, rainbow_loss_torch, rel_err)

pytestmark = pytest.mark.gpu
f32 = np.float32
INPUTS = ("value", "advantage", "value_next_online", "advantage_next_online",
          "value_next_target", "advantage_next_target", "support", "actions", "rewards", "dones",
          "weights")


def launch(t, z, outs):
    from oc_cleanrl_amd import ops

    ops.rainbow_loss_fwd_bwd(*[t[k] for k in INPUTS], float(z["gamma"]) ** int(z["n_step"]),
                             float(z["v_min"]), float(z["v_max"]), **outs)


def new_outs(z, dev, fill=float("nan")):
    B, N = z["value"].shape
    AN = z["advantage"].shape[1]
    full = lambda *s: torch.full(s, fill, device=dev)  # noqa: E731
    return dict(dvalue=full(B, N), dadvantage=full(B, AN), loss_per_sample=full(B),
                stats=full(2), target_pmfs=full(B, N),
                best_actions=torch.full((B,), -1, dtype=torch.int64, device=dev))


@pytest.mark.parametrize("name", LOSS_FIXTURES)
def test_loss_kernel_matches_reference(dev, name):
    z = fixture(f"rainbow_loss_{name}")
    t = {k: torch.from_numpy(z[k]).to(dev) for k in INPUTS}
    outs = new_outs(z, dev)  # NaN-filled: every element must be written
    launch(t, z, outs)
    o = {k: v.cpu().numpy() for k, v in outs.items()}
    assert np.array_equal(o["best_actions"], z["best_actions"])
    got = dict(o, loss=o["stats"][0], q_values=o["stats"][1])
    lim = bounds(z)
    report = []
    for k in CHECKED:
        assert np.isfinite(got[k]).all(), k
        err = rel_err(got[k], z[k + "64"])
        report.append(f"{k} {err:.2g} / {lim[k][1]:.2g}")
        assert err <= lim[k][0], (k, err, lim[k])
    print(f"rainbow_loss_{name}: error vs f64 / the f32 reference's own: " + ", ".join(report))
    # a second run and a graph replay are bitwise the first
    again, replayed = new_outs(z, dev, 0.0), new_outs(z, dev, 0.0)
    launch(t, z, again)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(t, z, replayed)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], again[k]) and torch.equal(outs[k], replayed[k]), k


@pytest.mark.parametrize("E,A,N", [(5, 6, 51), (2, 3, 5)])
def test_greedy_actions_equal_torch(dev, E, A, N):
    from oc_cleanrl_amd import ops

    gen = torch.Generator().manual_seed(E * 100 + N)
    value, adv = torch.randn(E, N, generator=gen), torch.randn(E, A * N, generator=gen) * 2
    support = torch.linspace(-10, 10, N)
    q = (dueling_dist(value, adv, A, N) * support).sum(2)
    q_out = torch.zeros(E, A, device=dev)
    actions = ops.rainbow_greedy(value.to(dev), adv.to(dev), support.to(dev), q_out=q_out)
    assert torch.equal(actions.cpu(), torch.argmax(q, 1))
    torch.testing.assert_close(q_out.cpu(), q, rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        ops.rainbow_greedy(value, adv.to(dev), support.to(dev))  # a CPU tensor
    with pytest.raises(ValueError):
        ops.rainbow_greedy(value.to(dev), adv.to(dev)[:, 1:], support.to(dev))


# ---- the trainer ----------------------------------------------------------------------------------
def rainbow_args(**kw):
    from oc_cleanrl_amd.rainbow import RainbowArgs

    base = dict(env_id="ALE/SpaceInvaders-v5", obs_mode="obj", num_envs=1, buffer_size=256,
                learning_starts=32, train_frequency=4, target_network_frequency=32,
                total_timesteps=4000, encoder_dims=(32, 64), decoder_dims=(64,), batch_size=8,
                n_step=3, n_atoms=51, log_every=40)
    base.update(kw)
    return RainbowArgs(**base)


def run(args, n, dev):
    from oc_cleanrl_amd.rainbow import RainbowTrainer

    tr = RainbowTrainer(args, dev, log=False)
    tr.steps(n)
    torch.cuda.synchronize()
    return tr


def test_graph_chunks_match_stepwise(dev):
    a = run(rainbow_args(cuda_graphs=False), 92, dev)  # trained since the last target sync at 64
    b = run(rainbow_args(cuda_graphs=True), 92, dev)
    assert b.graphs and not a.graphs
    for k in ("obs", "next_obs", "actions", "rewards", "dones", "tree", "state", "ring_obs",
              "ring_next_obs", "ring_actions", "ring_rewards", "ring_dones", "counter", "beta_dev"):
        assert torch.equal(getattr(a.rb, k), getattr(b.rb, k)), k
    for x, y in ((a.td_stats, b.td_stats), (a.loss_per_sample, b.loss_per_sample),
                 (a.opt.params, b.opt.params), (a.t_flat, b.t_flat)):
        assert torch.equal(x, y)
    for net_a, net_b in ((a.q, b.q), (a.target, b.target)):  # the noise buffers included
        for (k, v), w in zip(net_a.state_dict().items(), net_b.state_dict().values()):
            assert torch.equal(v, w), k
    assert any(not torch.equal(p, t) for p, t in zip(a.q.parameters(), a.target.parameters()))
    assert int(a.rb.state[1]) > 32


def test_train_step_matches_autograd_and_adam(dev):
    """One train step from a fixed sampled batch and fixed noise moves every parameter as torch
    autograd of the restated loss + torch.optim.Adam(eps=1.5e-4) does on the CPU (the error rule,
    on the parameter delta per tensor); then the sampled leaves hold the new priorities."""
    from oc_cleanrl_amd.rainbow import RainbowTrainer, make_rainbow_net

    args = rainbow_args(cuda_graphs=False)
    tr = RainbowTrainer(args, dev, log=False)
    tr.steps(args.learning_starts)  # replay filled, no train step yet
    tr.q.reset_noise = tr.target.reset_noise = lambda: None  # the noise stays what it is
    ctr = tr.rb.counter.clone()
    d = {k: v.clone().cpu() for k, v in
         tr.rb.sample(args.batch_size, out=tr.batch, step=tr.step_dev).items()}
    tr.rb.counter.copy_(ctr)  # the train step below draws the same batch
    sd0 = {k: v.detach().clone().cpu() for k, v in tr.q.state_dict().items()}
    sdt = {k: v.detach().clone().cpu() for k, v in tr.target.state_dict().items()}
    tr._train_step()
    torch.cuda.synchronize()
    assert torch.equal(tr.batch["observations"].cpu(), d["observations"])
    assert torch.equal(tr.batch["indices"].cpu(), d["indices"])
    sd1 = {k: v.detach().cpu() for k, v in tr.q.state_dict().items()}
    assert tr.opt.eps == 1.5e-4

    def heads(net, x):
        h = net.network(x / 255.0)
        return net.value_head(h), net.advantage_head(h)

    def reference(dtype):
        q, tgt = (make_rainbow_net(args, tr.obs_shape, tr.A) for _ in range(2))
        q.load_state_dict(sd0)
        tgt.load_state_dict(sdt)
        q, tgt = q.to(dtype), tgt.to(dtype)
        opt = torch.optim.Adam(q.parameters(), lr=args.learning_rate, eps=1.5e-4)
        gamma_n, delta_z = args.gamma ** args.n_step, q.delta_z
        if dtype == torch.float64:
            gamma_n, delta_z = float(f32(gamma_n)), float(f32(delta_z))
        obs, nxt = d["observations"].to(dtype), d["next_observations"].to(dtype)
        with torch.no_grad():
            v_nt, a_nt = heads(tgt, nxt)
            v_no, a_no = heads(q, nxt)
        value, adv = heads(q, obs)
        out = rainbow_loss_torch(value, adv, v_no, a_no, v_nt, a_nt, q.support, d["actions"],
                                 d["rewards"].to(dtype), d["dones"].to(dtype),
                                 d["weights"].to(dtype), gamma_n, args.v_min, args.v_max, delta_z)
        opt.zero_grad()
        out["loss"].backward()
        opt.step()
        return ({k: v.detach().double() - sd0[k].double() for k, v in q.state_dict().items()},
                out["loss"].item(), out["loss_per_sample"].detach().numpy())

    d32, loss32, _ = reference(torch.float32)
    d64, loss64, lps64 = reference(torch.float64)
    assert abs(tr.td_stats[0].item() - loss64) <= max(3 * abs(loss32 - loss64),
                                                      F32_FLOOR * abs(loss64))
    worst = {}
    params = {k for k, _ in tr.q.named_parameters()}
    for k in sd0:
        if k not in params:  # support and the noise buffers do not move
            assert torch.equal(sd1[k], sd0[k]), k
            continue
        got = sd1[k].double() - sd0[k].double()
        assert float(d64[k].abs().max()) > 0, k
        err, ref = rel_err(got.numpy(), d64[k].numpy()), rel_err(d32[k].numpy(), d64[k].numpy())
        worst[k] = (err, ref)
        assert err <= max(3 * ref, F32_FLOOR), (k, err, ref)
    print("rainbow train step, parameter delta error vs f64 / torch f32's own: "
          + ", ".join(f"{k} {e:.2g} / {r:.2g}" for k, (e, r) in worst.items()))
    # the new priorities: (|loss_i| + eps) ** alpha of the kernel's own loss_per_sample
    lps = tr.loss_per_sample.cpu().numpy()
    assert rel_err(lps, lps64) <= 1e-4
    idx = d["indices"].numpy()
    keep = sorted({int(i): k for k, i in enumerate(idx)}.values())  # the last occurrence wins
    leaves = tr.rb.tree.cpu().numpy()[idx[keep] + tr.rb.capacity - 1]
    eps, alpha = args.prioritized_replay_eps, args.prioritized_replay_alpha
    want32 = (np.abs(lps[keep]) + f32(eps)) ** f32(alpha)
    want64 = (np.abs(lps[keep].astype(np.float64)) + eps) ** alpha
    check_elementwise(leaves, want32, want64, "priorities")
    assert tr.rb.max_priority == max(1.0, float((np.abs(lps) + f32(eps)).max()))


def test_target_sync_beta_and_checkpoint(dev, tmp_path):
    import json

    from oc_cleanrl_amd.rainbow import run_rainbow

    args = rainbow_args(total_timesteps=96, log_dir=str(tmp_path))
    tr = run_rainbow(args, dev)
    torch.cuda.synchronize()
    assert tr.global_step == 96 and tr.graphs
    for t, p in zip(tr.target.parameters(), tr.q.parameters()):  # synced at step 96, tau = 1
        assert torch.equal(t, p)
    run_dir = next(tmp_path.iterdir())
    lines = [json.loads(s) for s in (run_dir / "metrics.jsonl").read_text().splitlines()]
    last = lines[-1]
    assert {"losses/td_loss", "losses/q_values", "charts/beta", "charts/SPS"} <= set(last)
    assert np.isfinite(last["losses/td_loss"]) and np.isfinite(last["losses/q_values"])
    # beta of the last train step (:611-614)
    assert last["charts/beta"] == pytest.approx(min(1.0, 0.4 + 96 * 0.6 / 96), rel=1e-6)
    assert lines[-2]["charts/beta"] == pytest.approx(0.4 + lines[-2]["global_step"] * 0.6 / 96,
                                                     rel=1e-6)
    ck = torch.load(run_dir / "rainbow_atari_oc.cleanrl_model", weights_only=True)
    z = fixture("rainbow_init_obj")
    assert list(ck["model_weights"]) == [str(k) for k in z["keys"]]  # the reference's keys
    assert set(ck) == {"model_weights", "args"} and ck["args"]["n_step"] == 3


def test_trainer_refuses_vector_envs(dev):
    from oc_cleanrl_amd.rainbow import RainbowTrainer

    with pytest.raises(ValueError):
        RainbowTrainer(rainbow_args(num_envs=2), dev, log=False)
