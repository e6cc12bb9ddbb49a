"""End-to-end learner on the GPU: graphs vs eager, reference-shaped outputs, checkpoints."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def small_args(**kw):
    from oc_cleanrl_amd.args import Args, finalize

    base = dict(env_id="ALE/Pong-v5", obs_mode="obj", architecture="PPO_OBJ", num_envs=32,
                num_steps=16, num_minibatches=4, update_epochs=2, total_timesteps=32 * 16 * 10,
                encoder_dims=(32, 64), decoder_dims=(64,), save_model=False)
    base.update(kw)
    return finalize(Args(**base), 1)


def run_iters(args, n, dev):
    from oc_cleanrl_amd.trainer import PPOTrainer

    tr = PPOTrainer(args, dev)
    ms = [tr.train_iteration() for _ in range(n)]
    torch.cuda.synchronize()
    return tr, ms


@pytest.mark.parametrize("fused_opt", [True, False])
def test_graph_replay_matches_eager(dev, fused_opt):
    a, ma = run_iters(small_args(cuda_graphs=False, fused_optimizer=fused_opt), 3, dev)
    b, mb = run_iters(small_args(cuda_graphs=True, fused_optimizer=fused_opt), 3, dev)
    assert b.graphs_ready and not a.graphs_ready
    assert torch.equal(a.actions, b.actions)
    assert torch.equal(a.advantages, b.advantages)
    for p, q in zip(a.agent.parameters(), b.agent.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-5, atol=1e-6)


def test_pixel_natureccn_iteration(dev):
    args = small_args(env_id="ALE/Breakout-v5", obs_mode="dqn", architecture="PPO", num_envs=8,
                      num_steps=8, update_epochs=1, torch_deterministic=False)
    tr, ms = run_iters(args, 2, dev)
    assert tr.obs.dtype == torch.uint8 and tr.obs.shape[2:] == (4, 84, 84)
    assert np.isfinite(ms[-1]["losses/loss"])
    assert tr.channels_last and tr.net_obs.is_contiguous(memory_format=torch.channels_last)


def test_pixel_update_graph_replay_matches_eager(dev):
    """The NatureCNN update captured into hipGraphs (MIOpen convolutions inside the capture)
    computes what the eager update computes: same rollout, parameters to conv-algorithm order."""
    runs = []
    for graphs in (False, True):
        args = small_args(env_id="ALE/Breakout-v5", obs_mode="dqn", architecture="PPO",
                          num_envs=8, num_steps=8, update_epochs=1, torch_deterministic=False,
                          cuda_graphs=graphs)
        tr, ms = run_iters(args, 2, dev)  # iteration 2: the update captured and replayed
        assert tr.graphs_ready == graphs and (len(tr.g_update) > 0) == graphs
        runs.append(tr)
    a, b = runs
    assert torch.equal(a.obs, b.obs) and torch.equal(a.actions, b.actions)
    for p, q in zip(a.agent.parameters(), b.agent.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-4, atol=1e-5)


def test_pixel_channels_last_matches_nchw(dev, monkeypatch):
    """The NHWC NatureCNN path (channels_last agent, NHWC store/gather) computes the same network
    as the plain NCHW one: same initial weights and network input, same logits up to the conv
    kernels' summation order; both train. (The store's f32 network copy is what this compares:
    the u8 rollout path, which skips it, is test_pixel_rollout_reads_the_u8_stacks.)"""
    from oc_cleanrl_amd import trainer as trm
    from oc_cleanrl_amd.trainer import PPOTrainer

    monkeypatch.setattr(trm, "U8_ROLLOUT_CONV", False)

    trs = []
    for cl in (False, True):
        args = small_args(env_id="ALE/Breakout-v5", obs_mode="dqn", architecture="PPO",
                          num_envs=8, num_steps=8, update_epochs=1, torch_deterministic=False,
                          conv_channels_last=cl, cuda_graphs=False)
        trs.append(PPOTrainer(args, dev))
    a, b = trs
    assert not a.channels_last and b.channels_last
    for (ka, pa), (kb, pb) in zip(a.agent.state_dict().items(), b.agent.state_dict().items()):
        assert ka == kb and torch.equal(pa, pb)
    assert b.prescale and not a.prescale
    assert torch.equal(a.net_obs / 255.0, b.net_obs)  # NormalizeImg folded in, bit-exact
    with torch.no_grad():
        la, va = a.agent.logits_and_value(a.net_obs)
        lb, vb = b.agent.logits_and_value(b.net_obs, prescaled=True)
    torch.testing.assert_close(la, lb, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(va, vb, rtol=1e-4, atol=1e-4)
    for tr in trs:
        m = tr.train_iteration()
        assert np.isfinite(m["losses/loss"])


def test_rollout_buffers_are_consistent(dev):
    from oc_cleanrl_amd import ops
    from oracle import ocppo_oracle as O

    tr, _ = run_iters(small_args(), 2, dev)
    T = tr.T
    c = lambda t: t.detach().cpu().numpy()  # noqa: E731
    # the stacked obs in slot t+1 = shift(slot t) + env frame (or reset-fill): slot invariant
    obs = c(tr.obs.float())
    dn = c(tr.dones)
    for t in range(T):
        for n in range(tr.N):
            if dn[t + 1, n] == 0:
                assert np.array_equal(obs[t + 1, n, :-1], obs[t, n, 1:])
            else:
                assert (obs[t + 1, n] == obs[t + 1, n, -1]).all()
    # logprobs stored by the action head = log_prob of the stored actions under the policy that
    # produced them; values/advantages/returns consistent with GAE
    adv, ret = O.gae(c(tr.rewards), c(tr.values[:T]), c(tr.dones[:T]), c(tr.values[T]),
                     c(tr.dones[T]), 0.99, 0.95)
    assert np.array_equal(adv, c(tr.advantages)) and np.array_equal(ret, c(tr.returns))


def test_checkpoint_payload_roundtrip(tmp_path, dev):
    from oc_cleanrl_amd.agents import make_agent

    tr, _ = run_iters(small_args(), 1, dev)
    p = tmp_path / "x.cleanrl_model"
    tr.save(p)
    ck = torch.load(p, weights_only=False)
    assert set(ck) == {"model_weights", "args", "Timesteps"}
    ag = make_agent("PPO_OBJ", tr.obs_shape, tr.A, dev, (32, 64), (64,)).to(dev)
    ag.load_state_dict(ck["model_weights"])
    x = tr.net_obs
    torch.testing.assert_close(ag.get_value(x), tr.agent.get_value(x))


def test_agent_get_action_and_value_api(dev):
    from oc_cleanrl_amd.agents import make_agent

    torch.manual_seed(0)
    ag = make_agent("PPO_OBJ", (4, 12), 6, dev, (32, 64), (64,)).to(dev)
    x = torch.randint(0, 160, (64, 4, 12), device=dev).float()
    torch.manual_seed(5)
    a, lp, ent, v = ag.get_action_and_value(x)
    assert a.dtype == torch.int64 and v.shape == (64, 1)
    # the same seed through torch's own Categorical gives the same actions
    torch.manual_seed(5)
    d = torch.distributions.Categorical(logits=ag.actor(ag.network(x)))
    assert torch.equal(d.sample(), a)
    _, lp2, ent2, _ = ag.get_action_and_value(x, a)
    torch.testing.assert_close(lp2, d.log_prob(a), rtol=1e-6, atol=2e-6)
    torch.testing.assert_close(ent2, d.entropy(), rtol=1e-6, atol=2e-6)
    lp2.sum().backward()
    assert ag.actor.weight.grad is not None


def test_fused_optimizer_tracks_torch_adam(dev):
    """Same seed, same rollout: HIP clip+Adam and torch clip_grad_norm_ + Adam stay close."""
    a, _ = run_iters(small_args(fused_optimizer=True), 2, dev)
    b, _ = run_iters(small_args(fused_optimizer=False), 2, dev)
    for p, q in zip(a.agent.parameters(), b.agent.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("arch,obs", [("PPO_OBJ", (4, 12)), ("PPO", (4, 84, 84))])
def test_fused_trunk_matches_module_forward_and_grads(dev, arch, obs):
    from oc_cleanrl_amd.agents import make_agent

    torch.manual_seed(0)
    ag = make_agent(arch, obs, 6, dev, (64, 128), (64,)).to(dev)
    x = torch.randint(0, 160, (32,) + obs, device=dev).float()
    h1 = ag.network(x)
    h2 = ag.trunk(x)
    # the trunk's autograd forwards of <= 128 rows run on the HIP Linear kernel (agents.SMALL_FWD:
    # an f32 FMA chain in another summation order than hipBLASLt's), so f32-level agreement
    torch.testing.assert_close(h2, h1, rtol=1e-5, atol=2e-6 * float(h1.abs().max()))
    g = torch.randn_like(h1)
    gr1 = torch.autograd.grad(h1, list(ag.network.parameters()), g)
    gr2 = torch.autograd.grad(h2, list(ag.network.parameters()), g)
    for a, b in zip(gr1, gr2):  # split-K weight grads: summation order differs
        torch.testing.assert_close(b, a, rtol=1e-4, atol=1e-5 * float(a.abs().max()))


def test_rollout_frame_cache_matches_full_trunk(dev):
    """Encoding only the newest frame per step (cache + shift) gives the same policy as
    re-encoding all W stacked frames (ppo_atari_oc.py:506), up to GEMM summation order."""
    args = small_args(encoder_dims=(32, 64, 48), decoder_dims=(64,), cuda_graphs=False,
                      rollout_frame_cache=True)
    a, _ = run_iters(args, 1, dev)
    assert a.frame_cache
    with torch.no_grad():
        a._rollout()  # a rollout under fixed weights, no update after it
        torch.cuda.synchronize()
        # the cache holds the encodings of the bootstrap obs (step T)
        torch.testing.assert_close(a.agent.decode(a.cache_logical(a.T)), a.agent.trunk(a.net_obs),
                                   rtol=1e-5, atol=1e-5)
        # every step's stored value = the critic on the full stacked obs of that step. The two
        # paths run different f32 GEMM kernels (the rollout's HIP MFMA kernel at N rows vs
        # hipBLASLt at (T+1)N rows); obs features up to 210 put hidden units at O(100), so the
        # summation-order difference is ~1e-7 x that per layer
        T, N = a.T, a.N
        full = a.agent.get_value(a.obs[:T + 1].float().view((T + 1) * N, *a.obs_shape))
        torch.testing.assert_close(a.values, full.view(T + 1, N), rtol=1e-4, atol=1e-4)
    b, _ = run_iters(small_args(encoder_dims=(32, 64, 48), decoder_dims=(64,),
                                rollout_frame_cache=False), 2, dev)
    c, _ = run_iters(small_args(encoder_dims=(32, 64, 48), decoder_dims=(64,),
                                rollout_frame_cache=True), 2, dev)
    assert not b.frame_cache and c.frame_cache
    same = (c.actions == b.actions).float().mean().item()
    assert same > 0.99, same


def test_nhwc_conv_act_matches_module_forward_and_grads(dev):
    """NatureCNN in channels_last through _ConvAct (bias-less NHWC conv + HIP bias/ReLU forward,
    HIP ReLU-backward/bias-grad backward) == nn.Conv2d/nn.ReLU autograd, and the HIP path runs."""
    from oc_cleanrl_amd import agents
    from oc_cleanrl_amd.agents import make_agent

    torch.manual_seed(0)
    ag = make_agent("PPO", (4, 84, 84), 4, dev).to(dev).to(memory_format=torch.channels_last)
    x = torch.randint(0, 256, (16, 4, 84, 84), device=dev).float()
    x = x.contiguous(memory_format=torch.channels_last)
    assert agents._conv_act_ok(x, ag.network[1])
    feat = ag.network[:7](x)  # the last conv's ReLU output: flatten + Linear read it as NHWC
    assert agents._flat_nhwc_ok(feat, ag.network[7], ag.network[8])
    h1 = ag.network(x)
    h2 = ag.trunk(x)
    torch.testing.assert_close(h2, h1, rtol=1e-5, atol=1e-5)
    g = torch.randn_like(h1)
    ps = list(ag.network.parameters())
    gr1 = torch.autograd.grad(h1, ps, g)
    gr2 = torch.autograd.grad(h2, ps, g)
    for a, b in zip(gr1, gr2):
        torch.testing.assert_close(b, a, rtol=1e-4, atol=1e-5 * float(a.abs().max()))


def test_eval_harness_generic_eval_semantics(dev):
    """evaluate(agent, make_env, n, device) (generic_eval.py:7-29): n finished episodes'
    returns, equal to a hand-rolled loop over the same env and the same sampling stream."""
    from oc_cleanrl_amd.agents import make_agent
    from oc_cleanrl_amd.evals import EvalEnv, evaluate, make_env

    torch.manual_seed(0)
    ag = make_agent("PPO_OBJ", (4, 12), 6, dev, (32, 64), (64,)).to(dev)
    torch.manual_seed(1)
    rets = evaluate(ag, make_env, 2, dev, env_id="ALE/Pong-v5", seed=3)
    assert len(rets) == 2 and all(np.isfinite(r) for r in rets)
    torch.manual_seed(1)
    env = EvalEnv("ALE/Pong-v5", seed=3, device=dev)
    obs, mine = env.reset(), []
    with torch.no_grad():
        while len(mine) < 2:
            obs, fin = env.step(ag.get_action_and_value(obs)[0])
            mine += fin
    assert mine == rets


def test_two_minibatch_updates_match_reference_golden(dev):
    """The whole learner step against the reference's own update block (ppo_atari_oc.py:566-610,
    exec'd with a real PPObj, torch Adam and clip_grad_norm_; tests/golden/update_2mb.npz): our
    fused-trunk forward, HIP fused loss, autograd into the flat buffer and HIP clip + Adam give
    the reference's parameters after each of two consecutive minibatch updates."""
    from conftest import golden
    from oc_cleanrl_amd import ops
    from oc_cleanrl_amd.agents import make_agent

    z = golden("update_2mb.npz")
    ag = make_agent("PPO_OBJ", (4, 6), 6, dev, (32, 64), (32,)).to(dev)
    sd = lambda i: {k.split("::", 1)[1]: torch.from_numpy(z[k]) for k in z  # noqa: E731
                    if k.startswith(f"sd{i}::")}
    ag.load_state_dict(sd(0))
    opt = ops.FlatAdam(ag.parameters(), lr=2.5e-4, eps=1e-5, max_grad_norm=0.5)
    T = lambda k, dt=None: torch.from_numpy(z[k]).to(dev) if dt is None else \
        torch.from_numpy(z[k]).to(dev, dt)  # noqa: E731
    b_obs, acts = T("b_obs"), T("b_actions")
    lp, adv, ret, val = T("b_logprobs"), T("b_advantages"), T("b_returns"), T("b_values")
    perm, M = T("perm"), int(z["M"])
    for i, start in enumerate((0, M)):
        idx = perm[start:start + M].contiguous()
        logits, value = ag.logits_and_value(ops.gather_rows(b_obs, idx))
        _, dl, dv = ops.ppo_loss_fwd_bwd(logits.detach(), value.detach().view(-1), acts, lp, adv,
                                         ret, val, mb_inds=idx, clip_coef=0.1, ent_coef=0.01,
                                         vf_coef=0.5, norm_adv=True, clip_vloss=True)
        torch.autograd.backward([logits, value], [dl, dv.view(-1, 1)])
        gn = float(torch.linalg.vector_norm(opt.grads.double()))
        assert abs(gn - z["grad_norms"][i]) <= 1e-5 * z["grad_norms"][i]
        opt.step()
        # Adam normalises each gradient element (m / (sqrt(v) + eps)): where |g| is near eps the
        # step is sensitive to the f32 summation order of g (MFMA / split-K vs the reference's
        # CPU GEMMs), so the bound is 1 % of one step (lr), and almost every element is exact
        # to 2e-7
        for k, ref in sd(i + 1).items():
            got = ag.state_dict()[k].cpu()
            torch.testing.assert_close(got, ref, rtol=0, atol=0.01 * 2.5e-4)
            assert float(((got - ref).abs() > 2e-7).float().mean()) < 0.01


def test_two_minibatch_updates_match_reference_golden_naturecnn(dev):
    """The NatureCNN learner step (channels_last agent, NHWC u8 gather with NormalizeImg folded
    in, _ConvAct convolutions, HIP loss, clip + Adam) against two updates of the reference's
    update block with PPODefault (tests/golden/update_2mb_cnn.npz; the 3136->512 weight is
    compared on a fixed sample of 4096 elements)."""
    from conftest import golden
    from oc_cleanrl_amd import ops
    from oc_cleanrl_amd.agents import make_agent

    z = golden("update_2mb_cnn.npz")
    torch.manual_seed(22)  # the fixture's seeded reference init, re-created (pinned by checksums)
    ag = make_agent("PPO", (4, 84, 84), 4).to(dev)
    for k, v in ag.state_dict().items():
        s = z[f"sum0::{k}"]
        vd = v.double()
        # init runs on the host CPU: its LAPACK QR (orthogonal_) differs from the fixture
        # machine's in the last bits, hence the same tolerance as test_models_cpu's init check
        np.testing.assert_allclose(float(vd.sum()), s[0], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(float((vd ** 2).sum()), s[1], rtol=1e-6)
    ag = ag.to(memory_format=torch.channels_last)
    opt = ops.FlatAdam(ag.parameters(), lr=2.5e-4, eps=1e-5, max_grad_norm=0.5)
    T = lambda k: torch.from_numpy(z[k]).to(dev)  # noqa: E731
    b_obs, acts = T("b_obs"), T("b_actions")
    lp, adv, ret, val = T("b_logprobs"), T("b_advantages"), T("b_returns"), T("b_values")
    perm, M = T("perm"), int(z["M"])
    for i, start in enumerate((0, M)):
        idx = perm[start:start + M].contiguous()
        x = torch.empty((M, 4, 84, 84), device=dev, memory_format=torch.channels_last)
        ops.gather_rows(b_obs, idx, x, scale255=True)
        logits, value = ag.logits_and_value(x, prescaled=True)
        _, dl, dv = ops.ppo_loss_fwd_bwd(logits.detach(), value.detach().view(-1), acts, lp, adv,
                                         ret, val, mb_inds=idx, clip_coef=0.1, ent_coef=0.01,
                                         vf_coef=0.5, norm_adv=True, clip_vloss=True)
        opt.zero_grad()  # conv grads are accumulated by autograd (not written in place)
        torch.autograd.backward([logits, value], [dl, dv.view(-1, 1)])
        gn = float(torch.linalg.vector_norm(opt.grads.double()))
        assert abs(gn - z["grad_norms"][i]) <= 1e-4 * z["grad_norms"][i]
        opt.step()
        for k, v in ag.state_dict().items():
            got = v.detach().cpu().contiguous().view(-1)
            ref = torch.from_numpy(z[f"sd{i + 1}::{k}"]).view(-1)
            if f"pick::{k}" in z:
                got = got[torch.from_numpy(z[f"pick::{k}"])]
            torch.testing.assert_close(got, ref, rtol=0, atol=0.01 * 2.5e-4)


def _reference_perms(seed, B, E, iterations, epochs_run=None):
    """The reference's shuffle stream (ppo_atari_oc.py:558-561): b_inds = arange every
    iteration, one np.random.shuffle per executed epoch, legacy global RNG seeded with `seed`."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(iterations):
        b = np.arange(B)
        perms = []
        for _ in range(E if epochs_run is None else epochs_run):
            rng.shuffle(b)
            perms.append(b.copy())
        out.append(np.concatenate(perms))
    return out


def test_shuffle_stream_matches_reference(dev):
    from oc_cleanrl_amd.trainer import PPOTrainer

    a = small_args()
    tr = PPOTrainer(a, dev)
    ref = _reference_perms(a.seed, a.local_batch_size, a.update_epochs, 3)
    for it in range(3):
        tr.train_iteration()
        assert np.array_equal(tr.perm_dev.cpu().numpy(), ref[it]), it


@pytest.mark.parametrize("graphs", [True, False])
def test_target_kl_early_stop(dev, graphs):
    """target_kl (:616-617): approx_kl >= 0 always exceeds -1, so every iteration stops after its
    first epoch. Metrics come from the executed minibatches only (no stale rows of skipped ones),
    and the np RNG advances by one shuffle per executed epoch, as the reference's does."""
    from oc_cleanrl_amd.trainer import PPOTrainer

    a = small_args(target_kl=-1.0, cuda_graphs=graphs)
    tr = PPOTrainer(a, dev)
    ref = _reference_perms(a.seed, a.local_batch_size, a.update_epochs, 3, epochs_run=1)
    B = a.local_batch_size
    for it in range(3):
        tr.stats.fill_(float("nan"))  # rows a skipped minibatch would leave stale
        m = tr.train_iteration()
        assert tr.executed_mb == a.num_minibatches
        assert np.array_equal(tr.perm_dev[:B].cpu().numpy(), ref[it]), it
        st = tr.stats.cpu().numpy()
        n = a.num_minibatches
        assert np.isfinite(st[:n]).all() and np.isnan(st[n:]).all()
        assert m["losses/loss"] == float(st[n - 1, 0])
        assert m["losses/approx_kl"] == float(st[n - 1, 5])
        assert abs(m["losses/clipfrac"] - float(np.mean(st[:n, 6]))) < 1e-7
    # without target_kl every epoch runs
    tr2 = PPOTrainer(small_args(cuda_graphs=graphs), dev)
    tr2.train_iteration()
    assert tr2.executed_mb == a.update_epochs * a.num_minibatches


def test_rollout_fusion_matches_unfused_rollout(dev):
    """store + first encoder layers in one launch and the cache shift in the last encoder layer's
    epilogue: same rollout buffers (obs, rewards, dones bit for bit; the last layer runs on the HIP
    MFMA kernel instead of hipBLASLt, so values / logprobs agree to f32 summation order)."""
    runs = []
    for fusion in (False, True):
        tr, _ = run_iters(small_args(encoder_dims=(32, 64, 48, 40), decoder_dims=(64,),
                                     rollout_fusion=fusion), 1, dev)
        with torch.no_grad():
            tr._rollout()  # a rollout under the same weights (after one identical update)
        torch.cuda.synchronize()
        assert tr.rollout_fusion == fusion
        runs.append(tr)
    a, b = runs
    # sampled actions steer the synthetic env, so a rare flipped sample (logits differ ~1e-6)
    # changes that env's later frames: compare by fraction
    same = (a.actions == b.actions).float().mean().item()
    assert same > 0.99, same
    same_obs = (a.obs == b.obs).flatten(2).all(-1).float().mean().item()
    assert same_obs > 0.99, same_obs
    close = ((a.values - b.values).abs() <= 1e-4 + 1e-4 * a.values.abs()).float().mean().item()
    assert close > 0.99, close


def test_rollout_cache_ring_is_bitwise_the_shifted_cache(dev):
    """The frame-encoding cache as a ring (newest encoding over the oldest slot, the decoder reading
    the slots rotated) gives bit for bit the rollout of the shifted cache: same kernels, same
    products in the same order, only addresses differ."""
    runs = []
    for ring in (False, True):
        tr, _ = run_iters(small_args(encoder_dims=(32, 64, 48, 64), decoder_dims=(64,),
                                     rollout_cache_ring=ring, num_steps=18), 2, dev)
        torch.cuda.synchronize()
        assert tr.rollout_fusion and tr.cache_ring == ring
        runs.append(tr)
    a, b = runs
    for k in ("obs", "actions", "logprobs", "values", "rewards", "dones", "advantages"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.cache_logical(a.T), b.cache_logical(b.T))
    for p, q in zip(a.agent.parameters(), b.agent.parameters()):
        assert torch.equal(p, q)


def test_head_env_fusion_is_bitwise_the_two_launch_step(dev):
    """trainer.FUSED_HEAD_ENV: the synthetic env's step in the policy head's launch leaves the
    rollout buffers and the parameters bit for bit where the two-launch step does (two iterations,
    captured rollouts), and the fused launch is the one that ran."""
    from oc_cleanrl_amd import ops as _ops, trainer

    runs = []
    for on in (False, True):
        old, real, calls = trainer.FUSED_HEAD_ENV, _ops.policy_head_env_step, []

        def spy(*a, **k):
            calls.append(1)
            return real(*a, **k)

        trainer.FUSED_HEAD_ENV, _ops.policy_head_env_step = on, spy
        try:
            tr, _ = run_iters(small_args(encoder_dims=(32, 64, 48, 64), decoder_dims=(256,),
                                         num_steps=18, cuda_graphs=True), 2, dev)
            torch.cuda.synchronize()
        finally:
            trainer.FUSED_HEAD_ENV, _ops.policy_head_env_step = old, real
        assert bool(calls) == on
        runs.append(tr)
    a, b = runs
    for k in ("obs", "actions", "logprobs", "values", "rewards", "dones", "advantages"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.env.ep_state, b.env.ep_state)
    assert a.param_checksum() == b.param_checksum()


def test_fused_heads_loss_updates_match_reference_golden(dev):
    """The update tail as ONE HIP op (heads forward + PPO loss + heads backward with the decoder's
    ReLU mask): two minibatch updates against the reference's own update block
    (ppo_atari_oc.py:566-610 exec'd on a PPObj with a 64-wide decoder, update_2mb_h64.npz)."""
    from conftest import golden
    from oc_cleanrl_amd import ops
    from oc_cleanrl_amd.agents import make_agent

    z = golden("update_2mb_h64.npz")
    ag = make_agent("PPO_OBJ", (4, 6), 6, dev, (32, 64), (64,)).to(dev)
    sd = lambda i: {k.split("::", 1)[1]: torch.from_numpy(z[k]) for k in z  # noqa: E731
                    if k.startswith(f"sd{i}::")}
    ag.load_state_dict(sd(0))
    opt = ops.FlatAdam(ag.parameters(), lr=2.5e-4, eps=1e-5, max_grad_norm=0.5)
    T = lambda k: torch.from_numpy(z[k]).to(dev)  # noqa: E731
    b_obs, acts = T("b_obs"), T("b_actions")
    lp, adv, ret, val = T("b_logprobs"), T("b_advantages"), T("b_returns"), T("b_values")
    perm, M = T("perm"), int(z["M"])
    for i, start in enumerate((0, M)):
        idx = perm[start:start + M].contiguous()
        hidden = ag.trunk(ops.gather_rows(b_obs, idx))
        box = hidden._ocppo_box
        box["premasked"] = True
        gp, *_ = ops.heads_loss_fwd_bwd(
            hidden.detach(), ag.actor.weight, ag.actor.bias, ag.critic.weight, ag.critic.bias,
            acts[idx], lp[idx], adv[idx], ret[idx], val[idx],
            adv_stats=ops.minibatch_adv_stats(adv, idx, M)[0], clip_coef=0.1, ent_coef=0.01,
            vf_coef=0.5, norm_adv=True, clip_vloss=True, db_h=box["bias"].grad,
            dwa=ag.actor.weight.grad, dwc=ag.critic.weight.grad, dba=ag.actor.bias.grad,
            dbc=ag.critic.bias.grad)
        torch.autograd.backward(hidden, gp)
        gn = float(torch.linalg.vector_norm(opt.grads.double()))
        assert abs(gn - z["grad_norms"][i]) <= 1e-5 * z["grad_norms"][i]
        opt.step()
        for k, ref in sd(i + 1).items():
            got = ag.state_dict()[k].cpu()
            torch.testing.assert_close(got, ref, rtol=0, atol=0.01 * 2.5e-4)
            assert float(((got - ref).abs() > 2e-7).float().mean()) < 0.01


def test_fused_heads_loss_trainer_matches_unfused(dev):
    """Trainer with and without the fused update tail: same minibatch stats and parameters up to
    f32 reduction order after two iterations (64-wide decoder)."""
    runs = []
    for fused in (False, True):
        tr, ms = run_iters(small_args(decoder_dims=(64,), fused_heads_loss=fused), 2, dev)
        assert tr.fused_heads_loss == fused
        runs.append((tr, ms))
    (a, ma), (b, mb) = runs
    for k in ("losses/value_loss", "losses/policy_loss", "losses/entropy", "losses/approx_kl"):
        assert ma[0][k] == pytest.approx(mb[0][k], rel=1e-4, abs=1e-6), k
    for p, q in zip(a.agent.parameters(), b.agent.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-3, atol=2e-5)


@pytest.mark.parametrize("graphs,mode", [(True, "kernel"), (False, "kernel"), (True, "head"),
                                         (False, "head"), (True, "torch"), (False, "torch")])
def test_per_step_noise_is_the_reference_sampling_stream(dev, graphs, mode):
    """The rollout's Exp(1) draws are exactly the [N, A] draws the reference's
    Categorical.sample makes step after step (ppo_atari_oc.py:506) from the device generator
    seeded like the trainer -- eager and graph-replayed iterations alike; drawn inside the
    sampling kernel (the default, ops.TorchExpStream: torch's Philox stream restated) or by
    torch's exponential_ per step."""
    from oc_cleanrl_amd.trainer import PPOTrainer

    a = small_args(sampling_noise=mode, cuda_graphs=graphs)
    tr = PPOTrainer(a, dev)
    assert (tr.exp_stream is not None) == (mode in ("kernel", "head"))
    got = []
    for _ in range(3):
        tr.train_iteration()
        got.append(tr.noise.clone())
    torch.cuda.synchronize()
    torch.manual_seed(tr.seed)
    for it in range(3):
        for t in range(a.num_steps):
            ref = torch.empty(a.local_num_envs, tr.A, device=dev).exponential_()
            assert torch.equal(got[it][t], ref), (it, t)


_GEMM_CHILD = r"""
import sys, torch
sys.path.insert(0, {root!r})
sys.path.insert(0, {root!r} + "/tests")
from conftest import golden
from test_config2_golden_gpu import config2_trainer, full_permutation
z = golden("update_config2.npz")
tr = config2_trainer(torch.device("cuda:0"), z)
assert tr.gemm_table == {on}, tr.gemm_table
tr.advantages.view(-1).copy_(torch.from_numpy(z["advantages"]).cuda())
tr.returns.view(-1).copy_(torch.from_numpy(z["returns"]).cuda())
tr.load_permutation(full_permutation(z, tr.E, tr.B))
tr._prepare_minibatches()
for j in range(2):
    tr._forward_backward(j)
    tr._opt_step()
torch.cuda.synchronize()
torch.save(torch.cat([p.detach().flatten() for p in tr.agent.parameters()]).cpu(), {out!r})
"""


def test_gemm_table_is_deterministic_and_matches_default(tmp_path):
    """The shipped hipBLASLt solution table (gemm_table.py, TunableOp read-only) under the default
    torch_deterministic=True, on the config-2 reference fixture's two minibatch updates (the
    bench's update chain, test_config2_golden_gpu): two runs with the table are bitwise
    identical, and a run with the default heuristic (OCPPO_GEMM_TABLE=0) agrees within the
    fixture's bound (1 % of an Adam step). One child process per run: TunableOp's state is
    process-wide."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    root = str(Path(__file__).resolve().parent.parent)
    outs = []
    for i, on in enumerate((True, True, False)):
        out = str(tmp_path / f"p{i}.pt")
        env = dict(os.environ, OCPPO_GEMM_TABLE="1" if on else "0")
        r = subprocess.run([sys.executable, "-c", _GEMM_CHILD.format(root=root, on=on, out=out)],
                           env=env, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(torch.load(out, weights_only=True))
    assert torch.equal(outs[0], outs[1]), "the table's picks are not run-to-run deterministic"
    # each run is within 1 % of an Adam step of the reference (test_config2_golden_gpu), so
    # within 2 % of each other; almost every element is identical
    torch.testing.assert_close(outs[0], outs[2], rtol=0, atol=0.02 * 2.5e-4)
    assert float(((outs[0] - outs[2]).abs() > 2e-7).float().mean()) < 0.01


def test_two_trainers_keep_their_own_update_gemm_route(dev):
    """Args.x6_gemm is per-trainer state (agents.set_update_gemm on its own agent): a trainer
    built with x6 off and one built after it with x6 on run their own routes, in either order,
    at config-2 sizes (the x6 products need >= 256 output tiles)."""
    from oc_cleanrl_amd import ops
    from oc_cleanrl_amd.trainer import KernelTimer, PPOTrainer

    def sites(tr):
        timer = KernelTimer(enabled=True)
        ops.TIMER = timer
        try:
            tr.train_iteration(collect_metrics=False)
            torch.cuda.synchronize()
        finally:
            ops.TIMER = None
        return sorted(n for n in timer.sites if n.startswith("gemm_x6_"))

    kw = dict(num_envs=128, num_steps=128, encoder_dims=(256, 512, 1024, 512),
              decoder_dims=(512,), update_epochs=1, cuda_graphs=False)
    off = PPOTrainer(small_args(x6_gemm=False, **kw), dev)
    on = PPOTrainer(small_args(x6_gemm=True, **kw), dev)
    assert len(sites(on)) >= 8
    assert sites(off) == []
    assert len(sites(on)) >= 8


@pytest.mark.parametrize("graphs", [False, True])
def test_weight_planes_are_bitwise_the_in_kernel_split(dev, graphs):
    """The update with the weights split into bf16 planes once per minibatch (Args.
    x6_weight_planes, ops.WeightPlanes) is bitwise the update with the split in gemm_x6's K loop:
    same rollouts, same parameters after three iterations at config-2 dims."""
    kw = dict(num_envs=128, num_steps=128, encoder_dims=(256, 512, 1024, 512),
              decoder_dims=(512,), update_epochs=1, cuda_graphs=graphs)
    from oc_cleanrl_amd import ops

    ops.PLANE_USES.clear()
    a, _ = run_iters(small_args(x6_weight_planes=True, **kw), 3, dev)
    used = dict(ops.PLANE_USES)
    b, _ = run_iters(small_args(x6_weight_planes=False, **kw), 3, dev)
    assert a.wplanes is not None and b.wplanes is None
    assert len(a.wplanes.jobs) >= 3
    # every plane set a refresh writes is read by some product (the decoder's dX planes too: its
    # backward runs on autograd's device thread, outside the trainer's weight_planes() scope)
    nk = {(n, k) for (_, n, k) in used}
    for w, trans, _ in a.wplanes.jobs:
        want = (w.shape[1], w.shape[0]) if trans else (w.shape[0], w.shape[1])
        assert want in nk, (tuple(w.shape), trans, sorted(used))
    for p, q in zip(a.agent.parameters(), b.agent.parameters()):
        assert torch.equal(p, q)


@pytest.mark.parametrize("graphs", [False, True])
def test_optimizer_written_planes_are_bitwise_the_split_launch(dev, monkeypatch, graphs):
    """The weights' planes written by the optimizer step (trainer.ADAM_WRITES_PLANES: one split
    launch per iteration) leave training bitwise where a split launch per minibatch does."""
    from oc_cleanrl_amd import trainer as trm

    kw = dict(num_envs=128, num_steps=128, encoder_dims=(256, 512, 1024, 512),
              decoder_dims=(512,), update_epochs=2, cuda_graphs=graphs, x6_weight_planes=True)
    monkeypatch.setattr(trm, "ADAM_WRITES_PLANES", True)
    a, _ = run_iters(small_args(**kw), 3, dev)
    monkeypatch.setattr(trm, "ADAM_WRITES_PLANES", False)
    b, _ = run_iters(small_args(**kw), 3, dev)
    assert a.planes_by_opt and not b.planes_by_opt
    for p, q in zip(a.agent.parameters(), b.agent.parameters()):
        assert torch.equal(p, q)


def test_sample_records_are_bitwise_the_soa_gather(dev):
    """GAE's 16-B sample records feeding the minibatch gather (Args.sample_records) leave the
    training bitwise unchanged: same parameters after three iterations with graphs."""
    a, _ = run_iters(small_args(sample_records_min=0, cuda_graphs=True), 3, dev)
    b, _ = run_iters(small_args(sample_records_min=-1, cuda_graphs=True), 3, dev)
    assert a.records is not None and b.records is None
    for p, q in zip(a.agent.parameters(), b.agent.parameters()):
        assert torch.equal(p, q)


@pytest.mark.parametrize("toggle", ["decode_gather", "wgrad_after_first_layer", "index_in_gather"])
def test_gathered_decoder_matches_the_expanded_one(dev, toggle):
    """The trainer's decoder reading its rows straight from the frame encodings
    (frames.FUSED_DECODE_GATHER: ocppo_gemm_x6_gather forward and weight gradient, no
    frames_expand copy), and the second encoder layer's weight gradient deferred past the first
    layer's rows launch so that launch's finish rides in its combine
    (agents.DEFER_WGRAD_AFTER_FIRST_LAYER), each leave the parameters bitwise where the plain path
    does: same products in the same order, over two iterations at config 2's network."""
    from oc_cleanrl_amd import agents, frames
    from oc_cleanrl_amd.args import Args, finalize
    from oc_cleanrl_amd.trainer import PPOTrainer

    mod, name = {"decode_gather": (frames, "FUSED_DECODE_GATHER"),
                 "index_in_gather": (frames, "FUSED_INDEX_IN_GATHER"),
                 "wgrad_after_first_layer": (agents, "DEFER_WGRAD_AFTER_FIRST_LAYER")}[toggle]

    from oc_cleanrl_amd import ops

    # the switched path must actually run at these sizes: count its own entry's calls
    probe = {"decode_gather": "dw_x6_parts_gather", "index_in_gather": "frames_gather_linear",
             "wgrad_after_first_layer": "relu_bias_wgrad"}[toggle]

    def run(on):
        setattr(mod, name, on)
        fused = agents.FUSED_L1_IN_DX
        agents.FUSED_L1_IN_DX = False  # the fused first-layer backward bypasses both paths
        real, calls = getattr(ops, probe), []

        def spy(*a, **k):
            if (probe == "dw_x6_parts_gather" or k.get("defer") is not None
                    or k.get("index") is not None):
                calls.append(1)
            return real(*a, **k)

        setattr(ops, probe, spy)
        try:
            # config 2's minibatch (11520 distinct frames): the sizes where the encoder's dX
            # products run on gemm_x6 with the lower layer's ReLU backward claimed
            args = finalize(Args(env_id="ALE/Pong-v5", obs_mode="obj", architecture="PPO_OBJ",
                                 num_envs=128, num_steps=128, num_minibatches=4, update_epochs=1,
                                 num_features=12, total_timesteps=128 * 128 * 4,
                                 save_model=False), 1)
            tr = PPOTrainer(args, dev, log=False)
            for _ in range(2):
                tr.train_iteration()
            torch.cuda.synchronize()
            tr.probe_calls = len(calls)
            return tr
        finally:
            setattr(mod, name, True)
            agents.FUSED_L1_IN_DX = fused
            setattr(ops, probe, real)

    a, b = run(True), run(False)
    assert a.probe_calls > 0 and b.probe_calls == 0, (a.probe_calls, b.probe_calls)
    assert a.param_checksum() == b.param_checksum()
    assert torch.equal(a.stats, b.stats)


def test_first_layer_backward_in_second_layer_dx(dev):
    """agents.FUSED_L1_IN_DX: the second encoder layer's dX runs the first layer's backward in its
    epilogue (ocppo_gemm_x6_wgrad; dX never stored, no rows launch) — the same sums in another
    order, so the parameters after two iterations at config 2's network agree to f32 rounding
    carried through two Adam steps, and the fused kernel is the one that ran."""
    from oc_cleanrl_amd import agents, ops
    from oc_cleanrl_amd.args import Args, finalize
    from oc_cleanrl_amd.trainer import PPOTrainer

    def run(on):
        old = agents.FUSED_L1_IN_DX
        agents.FUSED_L1_IN_DX = on
        calls = []
        real = ops.dx_x6_wgrad

        def spy(*a, **k):
            calls.append(a[0].shape)
            return real(*a, **k)

        ok_real = ops.dx_x6_wgrad_ok
        seen = []

        def ok_spy(g, w, mask, x):
            r = ok_real(g, w, mask, x)
            seen.append((tuple(g.shape), tuple(w.shape), tuple(x.shape), g.stride(), r))
            return r

        ops.dx_x6_wgrad = spy
        ops.dx_x6_wgrad_ok = ok_spy
        try:
            # config 2's minibatch (11520 distinct frames): the sizes where the encoder's dX
            # products run on gemm_x6 with the lower layer's ReLU backward claimed
            args = finalize(Args(env_id="ALE/Pong-v5", obs_mode="obj", architecture="PPO_OBJ",
                                 num_envs=128, num_steps=128, num_minibatches=4, update_epochs=1,
                                 num_features=12, total_timesteps=128 * 128 * 4,
                                 save_model=False), 1)
            tr = PPOTrainer(args, dev, log=False)
            for _ in range(2):
                tr.train_iteration()
            torch.cuda.synchronize()
            return tr, (calls, seen)
        finally:
            agents.FUSED_L1_IN_DX = old
            ops.dx_x6_wgrad = real
            ops.dx_x6_wgrad_ok = ok_real

    (a, ca), (b, cb) = run(True), run(False)
    assert ca[0] and not cb[0], (ca, cb)
    for p, q in zip(a.agent.parameters(), b.agent.parameters()):
        assert (p - q).abs().max().item() < 2e-5
    assert torch.allclose(a.stats, b.stats, rtol=1e-3, atol=1e-3)  # a clip flip: 1/4096


def test_lagged_metrics_are_the_synced_ones(dev):
    """train_iteration(lag=True) returns the previous iteration's metrics, gathered on the device
    behind its work: the same scalars as the synchronous path, one call later."""
    from oc_cleanrl_amd.args import Args, finalize
    from oc_cleanrl_amd.trainer import PPOTrainer

    def run(lag):
        args = finalize(Args(env_id="ALE/Pong-v5", obs_mode="obj", architecture="PPO_OBJ",
                             num_envs=16, num_steps=16, num_features=12, seed=3,
                             save_model=False), 1)
        tr = PPOTrainer(args, dev)
        out = [tr.train_iteration(collect_metrics=True, lag=lag) for _ in range(3)]
        return out + [tr.flush_metrics()]

    sync, lagged = run(False), run(True)
    assert lagged[0] == {} and sync[3] == {}
    for a, b in zip(sync[:3], lagged[1:]):
        assert a.keys() == b.keys()
        for k in a:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), (k, a[k], b[k])


def test_lagged_metrics_survive_a_gpu_that_has_caught_up(dev):
    """The lagged read of iteration k happens after iteration k+1's non-blocking copy is queued.
    With the GPU drained before every read (torch.cuda.synchronize: k+1's copy has landed), the
    values read are still iteration k's -- the two pinned vectors are used in turn."""
    from oc_cleanrl_amd.args import Args, finalize
    from oc_cleanrl_amd.trainer import PPOTrainer

    def run(lag):
        args = finalize(Args(env_id="ALE/Pong-v5", obs_mode="obj", architecture="PPO_OBJ",
                             num_envs=16, num_steps=16, num_features=12, seed=4,
                             save_model=False), 1)
        tr = PPOTrainer(args, dev)
        if lag:
            orig = tr._metrics_from

            def drained(pend):
                torch.cuda.synchronize()
                return orig(pend)
            tr._metrics_from = drained
        out = [tr.train_iteration(collect_metrics=True, lag=lag) for _ in range(4)]
        return out + [tr.flush_metrics()]

    sync, lagged = run(False), run(True)
    for a, b in zip(sync[:4], lagged[1:]):
        assert a.keys() == b.keys()
        for k in a:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), (k, a[k], b[k])


def test_pixel_rollout_reads_the_u8_stacks(dev):
    """Config-3-like pixel rollout: the first convolution from the rollout buffer's u8 slot
    (trainer.U8_ROLLOUT_CONV) against the f32 network copy path — same actions and values up to
    the f32 rounding of NormalizeImg's quotient (the u8 path divides the products instead)."""
    from oc_cleanrl_amd import trainer as trm
    from oc_cleanrl_amd.args import Args, finalize

    def run(flag):
        trm.U8_ROLLOUT_CONV = flag
        try:
            args = finalize(Args(env_id="ALE/Breakout-v5", obs_mode="dqn", architecture="PPO",
                                 num_envs=256, num_steps=8, update_epochs=1, seed=5,
                                 save_model=False, cuda_graphs=False), 1)
            tr = trm.PPOTrainer(args, dev)
            assert tr.u8_rollout == flag
            tr._rollout()
            torch.cuda.synchronize()
            return tr.actions.clone(), tr.values.clone()
        finally:
            trm.U8_ROLLOUT_CONV = True

    a1, v1 = run(True)
    a0, v0 = run(False)
    assert float((v1 - v0).abs().max()) <= 1e-4 * float(v0.abs().max() + 1)
    assert float((a1 == a0).float().mean()) >= 0.99


def test_rollout_flatten_linear_reads_the_nhwc_activation(dev):
    """agents.linear_act_nhwc_infer (inside agents.rollout_inference, the trainer's rollout): the
    NatureCNN's Flatten -> Linear on the channels_last activation against a cached column-permuted
    weight, no flatten copy -- the same hidden state as the plain no-grad trunk up to the f32
    summation order, and the cache refreshed when a new rollout begins after the weights change."""
    from oc_cleanrl_amd import agents
    from oc_cleanrl_amd.agents import make_agent

    torch.manual_seed(0)
    ag = make_agent("PPO", (4, 84, 84), 4, dev).to(dev).to(memory_format=torch.channels_last)
    x = torch.randint(0, 256, (256, 4, 84, 84), device=dev).float().contiguous(
        memory_format=torch.channels_last)
    with torch.no_grad():
        ref = ag.trunk(x)
        with agents.rollout_inference():
            got = ag.trunk(x)
        # the Flatten's successor Linear: its weight carries the rollout form
        assert any("nhwc" in getattr(m.weight, "_ocppo_rollout", {}) for m in ag.network
                   if isinstance(m, torch.nn.Linear))
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)
        lin = [m for m in ag.network if isinstance(m, torch.nn.Linear)][0]
        lin.weight.mul_(0.5)  # an update between rollouts (in place, as FlatAdam's)
        ref2 = ag.trunk(x)
        with agents.rollout_inference():
            got2 = ag.trunk(x)
        torch.testing.assert_close(got2, ref2, rtol=1e-5, atol=1e-5)
        assert not torch.allclose(ref2, ref)


def _nature_trunk_operands(dev, seed):
    from oc_cleanrl_amd.agents import make_agent

    torch.manual_seed(seed)
    ag = make_agent("PPO", (4, 84, 84), 4, dev).to(dev).to(memory_format=torch.channels_last)
    x = torch.randint(0, 256, (256, 4, 84, 84), device=dev).float().contiguous(
        memory_format=torch.channels_last)
    lin = [m for m in ag.network if isinstance(m, torch.nn.Linear)][0]
    return ag, x, lin


def test_rollout_forms_belong_to_their_parameter(dev):
    """A weight's rollout form (agents._rollout_form) hangs on the weight: two agents get two,
    and nothing in the package keeps one alive once its agent is gone."""
    import gc
    import weakref

    from oc_cleanrl_amd import agents

    a, x, lin_a = _nature_trunk_operands(dev, 0)
    b, _, lin_b = _nature_trunk_operands(dev, 1)
    with torch.no_grad():
        for ag in (a, b):
            with agents.rollout_inference():
                ag.trunk(x)
    fa = lin_a.weight._ocppo_rollout["nhwc"][0]
    fb = lin_b.weight._ocppo_rollout["nhwc"][0]
    assert fa is not fb and fa.data_ptr() != fb.data_ptr()
    assert fa.shape == lin_a.weight.shape and not torch.equal(fa, fb)
    ref = weakref.ref(fa)
    del fa, lin_a, a, ag
    gc.collect()
    assert ref() is None
    assert lin_b.weight._ocppo_rollout["nhwc"][0] is fb


def test_rollout_forms_keep_their_address_across_rollouts(dev):
    """The rollout graph holds a form's pointer: every rollout refills the same tensor in place,
    and the output follows the weights' in-place updates between rollouts -- the Flatten Linear's
    permuted weight (trunk) and the first convolution's tap-order copy (trunk_frames: the same
    first-layer bits in and out of the scope, then the same Flatten Linear difference)."""
    from oc_cleanrl_amd import agents

    ag, x, lin = _nature_trunk_operands(dev, 0)
    conv = [m for m in ag.network if isinstance(m, torch.nn.Conv2d)][0]
    frames = x.to(torch.uint8).contiguous()
    idx = torch.arange(frames.shape[0], device=dev)
    assert ag.trunk_frames_ok(frames, idx.numel())
    ptrs, outs = [], []
    with torch.no_grad():
        for _ in range(3):
            ref, ref_u8 = ag.trunk(x), ag.trunk_frames(frames, idx)
            with agents.rollout_inference():
                got, got_u8 = ag.trunk(x), ag.trunk_frames(frames, idx)
            torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(got_u8, ref_u8, rtol=1e-5, atol=1e-5)
            ptrs.append({(n, k): e[0].data_ptr() for n, p in ag.named_parameters()
                         for k, e in getattr(p, "_ocppo_rollout", {}).items()})
            outs.append((ref, ref_u8))
            lin.weight.mul_(0.5)  # an update between rollouts (in place, as FlatAdam's)
            conv.weight.mul_(0.5)
    assert sorted(k for _, k in ptrs[0]) == ["contig", "nhwc"]
    assert ptrs[0] == ptrs[1] == ptrs[2]
    for i in (0, 1):
        assert not torch.allclose(outs[i][0], outs[i + 1][0])
        assert not torch.allclose(outs[i][1], outs[i + 1][1])


def test_pixel_rollout_graph_replay_is_bitwise_eager(dev):
    """The pixel trainer's captured rollout refills the weights' rollout forms inside the graph
    (the refresh copies are captured with step 0): three iterations with hipGraphs leave bitwise
    the parameters of three eager ones."""
    runs = []
    for graphs in (False, True):
        args = small_args(env_id="ALE/Breakout-v5", obs_mode="dqn", architecture="PPO",
                          num_envs=256, num_steps=8, update_epochs=1, cuda_graphs=graphs)
        tr, _ = run_iters(args, 3, dev)
        assert tr.graphs_ready == graphs
        runs.append(tr)
    a, b = runs
    assert torch.equal(a.actions, b.actions)
    for (n, p), q in zip(a.agent.named_parameters(), b.agent.parameters()):
        assert torch.equal(p, q), n


def test_conv_relu_backward_in_the_flattened_linear_dx(dev, monkeypatch):
    """agents.CONV_RELU_IN_FLAT_DX: the last convolution's ReLU backward and bias gradient ride
    in the dX epilogue of the Linear reading its flattened channels_last output (ops.dx_x6_relu,
    the activation as the mask) -- the gradients of the whole trunk match the unfused chain
    (relu_bias_grad over that layer's gradient) to f32 level."""
    from oc_cleanrl_amd import agents, ops
    from oc_cleanrl_amd.agents import make_agent

    torch.manual_seed(3)
    ag = make_agent("PPO", (4, 84, 84), 4, dev).to(dev).to(memory_format=torch.channels_last)
    ops.FlatAdam(ag.parameters(), lr=1e-4)  # in-place grads, as in the trainer
    x = torch.randint(0, 256, (2048, 4, 84, 84), device=dev).float().contiguous(
        memory_format=torch.channels_last)
    g = torch.randn(2048, 512, device=dev)
    grads = []
    for on in (True, False):
        monkeypatch.setattr(agents, "CONV_RELU_IN_FLAT_DX", on)
        for p in ag.parameters():
            p.grad.zero_()
        h = ag.trunk(x)
        h.backward(g)
        torch.cuda.synchronize()
        grads.append([p.grad.clone() for p in ag.parameters()])
    for a, b in zip(*grads):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5 * float(b.abs().max()))
