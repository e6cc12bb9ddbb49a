"""C51 on the GPU: the fused projection + loss kernel and the expected-value epsilon-greedy kernel
against fixtures made from the reference (tests/golden/gen_golden_c51.py), and the C51Trainer on
DQNTrainer's loop (graph chunks, one train step against torch autograd + Adam, hard target copy,
run_c51's files, the pixel network).

Error rule (loss kernel, acting kernel's q, the train step's parameter delta): a tensor's error
against the float64 twin, relative to the twin's largest element, is at most
max(3 x the f32 torch reference's own error against the same twin, 4 * 2^-23)."""
import json

import numpy as np
import pytest
import torch

from c51_util import CHECKED, F32_FLOOR, FIXTURES, bounds, c51_loss_torch, fixture, rel_err

pytestmark = pytest.mark.gpu


def loss_inputs(z, dev):
    t = lambda k: torch.from_numpy(z[k]).to(dev)  # noqa: E731
    return (t("logits"), t("logits_next"), t("atoms"), t("actions"), t("rewards"), t("dones"),
            float(z["gamma"]), float(z["v_min"]), float(z["v_max"]))


def run_loss(z, dev):
    from oc_cleanrl_amd import ops

    ins = loss_inputs(z, dev)
    B, N = z["logits"].shape[0], z["atoms"].size
    out = dict(dlogits=torch.full_like(ins[0], float("nan")),
               stats=torch.full((2,), float("nan"), device=dev),
               target_pmfs=torch.full((B, N), float("nan"), device=dev),
               next_action=torch.full((B,), -1, dtype=torch.int64, device=dev))
    ops.c51_loss_fwd_bwd(*ins, **out)
    torch.cuda.synchronize()
    return ins, out


@pytest.mark.parametrize("name", FIXTURES)
def test_loss_kernel_matches_reference(dev, name):
    z = fixture(name)
    _, out = run_loss(z, dev)
    assert np.array_equal(out["next_action"].cpu().numpy(), z["next_action"])
    got = dict(target_pmfs=out["target_pmfs"].cpu().numpy(), dlogits=out["dlogits"].cpu().numpy(),
               loss=out["stats"][0].item(), q_values=out["stats"][1].item())
    bd = bounds(z)
    errs = {k: rel_err(got[k], z[k + "64"]) for k in CHECKED}
    print(f"c51_{name}: error vs f64 / (f32 reference's own error), bound: "
          + ", ".join(f"{k} {errs[k]:.2g} / {bd[k][1]:.2g}, {bd[k][0]:.2g}" for k in CHECKED))
    for k in CHECKED:
        assert errs[k] <= bd[k][0], (k, errs[k], bd[k])
    B, N = z["logits"].shape[0], z["atoms"].size
    A = z["logits"].shape[1] // N
    taken = np.zeros((B, A), bool)
    taken[np.arange(B), z["actions"]] = True
    dl = got["dlogits"].reshape(B, A, N)
    if name == "ties":
        assert np.abs(got["target_pmfs"].astype(np.float64).sum(1) - 1).max() <= 2.0 ** -22
        assert (dl[~taken] == 0).all()  # rows of the actions not taken: exactly zero
    if name == "peaked":
        assert (got["dlogits"][z["dlogits"] == 0] == 0).all()
    assert (dl[~taken] == 0).all() and np.isfinite(dl).all()


@pytest.mark.parametrize("name", ["b32_a6_n51", "b7_a18_n101"])
def test_loss_kernel_repeatable_and_graph_replay(dev, name):
    from oc_cleanrl_amd import ops

    z = fixture(name)
    ins, a = run_loss(z, dev)
    _, b = run_loss(z, dev)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # without the optional outputs: same dlogits and stats
    stats, dl = ops.c51_loss_fwd_bwd(*ins)
    assert torch.equal(dl, a["dlogits"]) and torch.equal(stats, a["stats"])
    g_out = {k: torch.zeros_like(v) for k, v in a.items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        ops.c51_loss_fwd_bwd(*ins, **g_out)
    for _ in range(2):  # stats are rewritten, not accumulated
        g.replay()
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], g_out[k]), k


def _expected_q(logits, atoms, A, dtype):
    E, N = logits.shape[0], atoms.numel()
    pm = torch.softmax(logits.to(dtype).view(E, A, N), dim=2)
    return (pm * atoms.to(dtype)).sum(2)


@pytest.mark.parametrize("E,A,N,v", [(5, 6, 51, 10.0), (3, 18, 101, 100.0), (2, 3, 5, 2.0)])
def test_epsilon_greedy_kernel(dev, E, A, N, v):
    from oc_cleanrl_amd import ops

    rng = np.random.default_rng(7)
    logits_c = torch.from_numpy((rng.standard_normal((E, A * N)) * 2).astype(np.float32))
    atoms_c = torch.linspace(-v, v, N)
    logits, atoms = logits_c.to(dev), atoms_c.to(dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    q = torch.full((E, A), float("nan"), device=dev)
    eps = torch.zeros(1, device=dev)
    q64 = _expected_q(logits_c, atoms_c, A, torch.float64).numpy()
    ref = rel_err(_expected_q(logits_c, atoms_c, A, torch.float32).numpy(), q64)
    both = set()
    for start_e, end_e in ((0.0, 0.0), (1.0, 1.0), (0.5, 0.5)):
        for t in range(12):
            step.fill_(t)
            act = ops.c51_epsilon_greedy(logits, atoms, 11, step, start_e, end_e, 100.0,
                                         epsilon_out=eps, step_offset=3, q_out=q)
            want = ops.epsilon_greedy(q, 11, step, start_e, end_e, 100.0, step_offset=3)
            assert torch.equal(act, want), (start_e, t)
            assert float(eps) == start_e
            greedy = torch.equal(act, torch.argmax(q, 1))
            if start_e == 0.0:
                assert greedy
            both.add((start_e, greedy))
    err = rel_err(q.cpu().numpy(), q64)
    print(f"c51 q [{E}, {A}, {N}]: error vs f64 {err:.2g}, torch f32's own {ref:.2g}")
    assert err <= max(3 * ref, F32_FLOOR)
    assert np.array_equal(torch.argmax(q, 1).cpu().numpy(), q64.argmax(1))
    if E >= 3:  # epsilon = 0.5 over 12 steps: both sides of the coin were seen
        assert (0.5, True) in both and (0.5, False) in both


def test_epsilon_greedy_tie_takes_lower_index(dev):
    from oc_cleanrl_amd import ops

    E, A, N = 4, 4, 51
    rng = np.random.default_rng(8)
    lg = (rng.standard_normal((E, A, N))).astype(np.float32)
    lg[:, 3] = lg[:, 1]
    lg[:, 1, -1] += 20.0  # both copies put their mass on the top atom: the shared maximum
    lg[:, 3, -1] += 20.0
    logits = torch.from_numpy(lg.reshape(E, A * N)).to(dev)
    atoms = torch.linspace(-10, 10, N).to(dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    q = torch.zeros((E, A), device=dev)
    act = ops.c51_epsilon_greedy(logits, atoms, 1, step, 0.0, 0.0, 10.0, q_out=q)
    assert torch.equal(q[:, 1], q[:, 3]) and bool((q[:, 1] > q[:, 0]).all())
    assert act.tolist() == [1] * E


# ---- the trainer ------------------------------------------------------------------------------
def c51_args(**kw):
    from oc_cleanrl_amd.c51 import C51Args

    base = dict(env_id="ALE/SpaceInvaders-v5", obs_mode="obj", num_envs=4, buffer_size=256,
                learning_starts=64, train_frequency=4, target_network_frequency=32,
                total_timesteps=4000, encoder_dims=(32, 64), decoder_dims=(64,), batch_size=8,
                n_atoms=51, save_model=False, log_every=40)
    base.update(kw)
    return C51Args(**base)


def run(args, n, dev):
    from oc_cleanrl_amd.c51 import C51Trainer

    tr = C51Trainer(args, dev, log=False)
    tr.steps(n)
    torch.cuda.synchronize()
    return tr


def test_graph_chunks_match_stepwise(dev):
    a = run(c51_args(cuda_graphs=False), 124, dev)  # trained since the last target copy at 96
    b = run(c51_args(cuda_graphs=True), 124, dev)
    assert b.graphs and not a.graphs
    for x, y in ((a.rb.state, b.rb.state), (a.rb.obs, b.rb.obs), (a.rb.actions, b.rb.actions),
                 (a.rb.rewards, b.rb.rewards), (a.rb.dones, b.rb.dones), (a.epsilon, b.epsilon),
                 (a.td_stats, b.td_stats), (a.opt.params, b.opt.params), (a.t_flat, b.t_flat)):
        assert torch.equal(x, y)
    assert any(not torch.equal(p, t) for p, t in zip(a.q.parameters(), a.target.parameters()))


def test_train_step_matches_autograd_and_adam(dev):
    """One train step from a fixed sampled batch moves the parameters as torch autograd of the
    restated loss + torch.optim.Adam(eps=0.01 / batch_size) does (the error rule, on the
    parameter delta per tensor)."""
    from oc_cleanrl_amd.c51 import C51Trainer, make_c51net

    args = c51_args(cuda_graphs=False)
    tr = C51Trainer(args, dev, log=False)
    tr.steps(args.learning_starts)  # replay filled, no train step yet
    ctr = tr.rb.counter.clone()
    d = {k: v.clone().cpu() for k, v in tr.rb.sample(args.batch_size, out=tr.batch).items()}
    tr.rb.counter.copy_(ctr)  # the train step below draws the same batch
    sd0 = {k: v.detach().clone().cpu() for k, v in tr.q.state_dict().items()}
    tr._train_step()
    torch.cuda.synchronize()
    assert torch.equal(tr.batch["observations"].cpu(), d["observations"])
    sd1 = {k: v.detach().cpu() for k, v in tr.q.state_dict().items()}
    assert tr.opt.eps == 0.01 / args.batch_size

    def reference(dtype):
        nets = []
        for _ in range(2):
            net = make_c51net(args, tr.obs_shape, tr.A)
            net.load_state_dict(sd0)
            nets.append(net.to(dtype))
        q, tgt = nets
        opt = torch.optim.Adam(q.parameters(), lr=args.learning_rate, eps=0.01 / args.batch_size)
        gamma = args.gamma if dtype == torch.float32 else float(np.float32(args.gamma))
        with torch.no_grad():
            nxt = tgt(d["next_observations"].to(dtype))
        out = c51_loss_torch(q(d["observations"].to(dtype)), nxt, q.atoms, d["actions"],
                             d["rewards"].to(dtype), d["dones"].to(dtype), gamma, args.v_min,
                             args.v_max)
        opt.zero_grad()
        out["loss"].backward()
        opt.step()
        return ({k: v.detach().double() - sd0[k].double() for k, v in q.state_dict().items()},
                out["loss"].item())

    d32, loss32 = reference(torch.float32)
    d64, loss64 = reference(torch.float64)
    assert abs(tr.td_stats[0].item() - loss64) <= max(3 * abs(loss32 - loss64),
                                                      F32_FLOOR * abs(loss64))
    worst = {}
    for k in sd0:
        if k == "atoms":
            assert torch.equal(sd1[k], sd0[k])
            continue
        got = sd1[k].double() - sd0[k].double()
        assert float(d64[k].abs().max()) > 0, k
        err, ref = rel_err(got.numpy(), d64[k].numpy()), rel_err(d32[k].numpy(), d64[k].numpy())
        worst[k] = (err, ref)
        assert err <= max(3 * ref, F32_FLOOR), (k, err, ref)
    print("c51 train step, parameter delta error vs f64 / torch f32's own: "
          + ", ".join(f"{k} {e:.2g} / {r:.2g}" for k, (e, r) in worst.items()))


def test_hard_target_copy(dev):
    from oc_cleanrl_amd.c51 import C51Trainer

    tr = C51Trainer(c51_args(cuda_graphs=True), dev, log=False)
    q0 = [p.detach().clone() for p in tr.q.parameters()]
    tr.steps(64)  # up to learning_starts: no train step
    for p, p0 in zip(tr.q.parameters(), q0):
        assert torch.equal(p, p0)
    tr.steps(28)  # global step 92, one train step before the sync at 96: target still the init
    assert any(not torch.equal(p, p0) for p, p0 in zip(tr.q.parameters(), q0))
    for t, p0 in zip(tr.target.parameters(), q0):
        assert torch.equal(t, p0)
    tr.steps(4)
    torch.cuda.synchronize()
    for t, p in zip(tr.target.parameters(), tr.q.parameters()):
        assert torch.equal(t, p)
    m = tr.metrics()
    assert np.isfinite(m["losses/loss"]) and np.isfinite(m["losses/q_values"])
    assert m["charts/epsilon"] == pytest.approx(max(1 + (0.01 - 1) / 400 * 96, 0.01), rel=1e-6)


def test_run_c51_writes_metrics(dev, tmp_path):
    from oc_cleanrl_amd.c51 import run_c51

    args = c51_args(total_timesteps=160, log_dir=str(tmp_path), save_model=True)
    tr = run_c51(args, dev)
    assert tr.global_step == 160
    runs = list(tmp_path.iterdir())
    assert len(runs) == 1
    lines = [json.loads(s) for s in (runs[0] / "metrics.jsonl").read_text().splitlines()]
    last = lines[-1]
    assert last["global_step"] == 160
    assert {"losses/loss", "losses/q_values", "charts/epsilon", "charts/SPS"} <= set(last)
    assert "losses/td_loss" not in last
    ck = torch.load(runs[0] / "c51_atari_oc.cleanrl_model", weights_only=True)
    assert set(ck) == {"model_weights", "args"} and ck["args"]["n_atoms"] == 51


def test_pixel_network_chunk_and_checkpoint(dev, tmp_path):
    """One pixel-mode run on the NatureCNN trunk: finite metrics, and a checkpoint with the
    reference QNetwork_C51's state-dict keys that loads into a fresh QNetworkC51."""
    from conftest import golden
    from oc_cleanrl_amd.c51 import QNetworkC51, run_c51

    args = c51_args(obs_mode="dqn", env_id="ALE/Pong-v5", num_envs=2, buffer_size=128,
                    learning_starts=16, target_network_frequency=16, total_timesteps=32,
                    torch_deterministic=False, cuda_graphs=False, log_every=16,
                    log_dir=str(tmp_path), save_model=True)
    tr = run_c51(args, dev)
    assert tr.rb.obs.dtype == torch.uint8 and tuple(tr.rb.obs.shape[2:]) == (4, 84, 84)
    m = tr.metrics()
    assert np.isfinite(m["losses/loss"]) and np.isfinite(m["losses/q_values"])
    run_dir = next(tmp_path.iterdir())
    ck = torch.load(run_dir / "c51_atari_oc.cleanrl_model", weights_only=True)
    z = golden("c51_init_a6.npz")
    assert tr.A == int(z["n_actions"])
    assert list(ck["model_weights"]) == [str(k) for k in z["keys"]]
    fresh = QNetworkC51((4, 84, 84), tr.A, n_atoms=51, v_min=-10, v_max=10)
    fresh.load_state_dict(ck["model_weights"], strict=True)
    assert torch.equal(fresh.atoms, torch.from_numpy(z["atoms"]))
