"""The TD3 / DDPG kernels (csrc/ocppo_td3.hip) against the scripts' fixtures and the NumPy twins
(tests/td3_util.py): DESIGN 11's rule (error relative to the twin's largest element at most max(3 x
the f32 reference's own error, 4 * 2^-23)) unless a test says bitwise."""
import numpy as np
import pytest
import torch

import td3_util as U
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SHAPES = [(B, A, D) for B in (1, 33, 64, 256) for A, D in ((1, 3), (6, 5))]


@pytest.fixture(scope="module")
def ops():
    from oc_cleanrl_amd import ops

    return ops


def _bounds(A, dev):
    lo, hi = (torch.tensor(v, device=dev) for v in U.BOUNDS[A])
    return lo, hi, (hi - lo) / 2.0, (hi + lo) / 2.0


# ---- replay ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,A,D", [(1, 1, 3), (5, 6, 5)])
def test_replay_contents_wrap_final_obs_and_samples_bitwise(ops, dev, E, A, D):
    size, B, seed = 4, 33, 11
    rb = ops.ContReplayBuffer(size, E, D, A, dev, seed=seed)
    g = torch.Generator().manual_seed(E)
    want = {k: np.zeros(s, np.float32) for k, s in (
        ("obs", (size, E, D)), ("next", (size, E, D)), ("act", (size, E, A)), ("rew", (size, E)),
        ("done", (size, E)))}
    obs = torch.randn(E, D, generator=g).to(dev)
    for step in range(7):  # wraps at 4
        nxt, fin = torch.randn(E, D, generator=g), torch.randn(E, D, generator=g)
        act, rew = torch.randn(E, A, generator=g), torch.randn(E, generator=g)
        done = ((torch.arange(E) + step) % 3 == 0).float()
        term = ((torch.arange(E) + step) % 2 == 0).float() * done
        pos = step % size
        want["obs"][pos] = obs.cpu().numpy()
        want["next"][pos] = torch.where(done[:, None] > 0, fin, nxt).numpy()
        want["act"][pos], want["rew"][pos], want["done"][pos] = act.numpy(), rew.numpy(), term.numpy()
        carry = step % 2 == 0
        rb.add(obs, nxt.to(dev), fin.to(dev), done.to(dev), act.to(dev), rew.to(dev), term.to(dev),
               carry=carry)
        if carry:
            assert torch.equal(obs.cpu(), nxt)  # obs <- next_obs, not the terminal observation
        else:
            obs = nxt.to(dev)
        assert rb.state.tolist() == [(step + 1) % size, int(step + 1 >= size)]
        if step in (2, 6):  # partly filled, then full
            ctr = int(rb.counter)
            d = rb.sample(B, with_indices=True)
            idx = U.replay_indices_ref(seed, ctr, B, (step + 1) % size, step + 1 >= size, size, E)
            assert np.array_equal(d["indices"].cpu().numpy(), idx) and int(rb.counter) == ctr + 1
            i, e = idx[:, 0], idx[:, 1]
            assert np.array_equal(d["observations"].cpu().numpy(), want["obs"][i, e])
            assert np.array_equal(d["actions"].cpu().numpy(), want["act"][i, e])
            assert np.array_equal(d["next_observations"].cpu().numpy(), want["next"][i, e])
            assert np.array_equal(d["rewards"].cpu().numpy()[:, 0], want["rew"][i, e])
            assert np.array_equal(d["dones"].cpu().numpy()[:, 0], want["done"][i, e])
            assert (d["next_obs_act"][:, D:] == 0).all()  # left for td3_target_actions
            assert d["observations"].data_ptr() == d["obs_act"].data_ptr()
    for k, t in (("obs", rb.obs), ("next", rb.next_obs), ("act", rb.actions), ("rew", rb.rewards),
                 ("done", rb.dones)):
        assert np.array_equal(t.cpu().numpy(), want[k]), k
    # no done flags: next_obs as given and zeros as the done flag
    rb.add(obs, obs + 1, None, None, act.to(dev), rew.to(dev))
    assert torch.equal(rb.next_obs[3], obs + 1) and (rb.dones[3] == 0).all()
    with pytest.raises(ValueError, match="come together"):
        rb.add(obs, obs + 1, obs, None, act.to(dev), rew.to(dev))


# ---- acting ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,A", [(1, 1), (5, 6), (5, 1), (1, 6)])
def test_act_both_phases(ops, dev, E, A):
    from oc_cleanrl_amd import td3

    H, seed, ls, en = 256, 5, 10, 0.1
    lo, hi, scale, bias = _bounds(A, dev)
    g = torch.Generator().manual_seed(E + 10 * A)
    h = torch.relu(torch.randn(E, H, generator=g)).to(dev)
    w = (torch.randn(A, H, generator=g) / 16).to(dev)
    b = (0.1 * torch.randn(A, generator=g)).to(dev)
    step = torch.tensor([7], device=dev)
    # the uniform phase (t = 7, 9 < 10): low + (high - low) * u, inside [low, high)
    for k in (0, 2):
        a = ops.td3_act(h, w, b, scale, bias, lo, hi, seed, step, ls, en, step_offset=k)
        u = U.unit24(U.act_words(seed, 7 + k, E, A)[..., 0])
        assert np.array_equal(ops.td3_noise(seed, step, E, A, k, uniform=True).cpu().numpy(), u)
        assert torch.equal(a, lo + (hi - lo) * torch.from_numpy(u).to(dev))
        assert (a >= lo).all() and (a < hi).all()
    # the actor phase (t = 10): against the f64 twin of the same words, the f32 restatement's error
    a = ops.td3_act(h, w, b, scale, bias, lo, hi, seed, step, ls, en, step_offset=3)
    words = U.act_words(seed, 10, E, A)
    z = ops.td3_noise(seed, step, E, A, 3)
    U.check("z", z, U.box_muller(words, np.float32), U.box_muller(words, np.float64))

    def ref(dtype, zz):
        c = lambda v: v.detach().cpu().to(dtype)  # noqa: E731
        act = torch.tanh(c(h) @ c(w).t() + c(b)) * c(scale) + c(bias)
        return torch.clamp(act + (c(scale) * en) * torch.as_tensor(zz).to(dtype), c(lo), c(hi))

    z64 = U.box_muller(words, np.float64)
    U.check("action", a, ref(torch.float32, U.box_muller(words, np.float32)), ref(torch.float64, z64))
    # ... and bitwise the unfused path's restatement on the kernel's own draws
    mu = td3.act_mu(h, w, b)
    assert torch.equal(a, torch.clamp(torch.tanh(mu) * scale + bias + (scale * en) * z, lo, hi))


def test_uniform_phase_stays_below_high_and_normal_moments(ops, dev):
    lo, hi = torch.tensor([-2.0, 0.1], device=dev), torch.tensor([2.0, 0.3], device=dev)
    E, A = 2 ** 15, 2
    h, w, b = torch.zeros(E, 64, device=dev), torch.zeros(A, 64, device=dev), torch.zeros(A, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    a = ops.td3_act(h, w, b, (hi - lo) / 2, (hi + lo) / 2, lo, hi, 3, step, 1, 0.1)
    assert (a >= lo).all() and (a < hi).all()
    assert abs(float(a[:, 0].mean())) < 5 * 4 / 12 ** 0.5 / E ** 0.5
    n = E * A  # 2^16 draws
    z = ops.td3_noise(3, step, E, A).double()
    assert torch.isfinite(z).all()
    assert abs(float(z.mean())) < 5 / n ** 0.5
    assert abs(float(z.var()) - 1) < 5 * (2 / n) ** 0.5
    zt = ops.td3_target_noise(3, step, E, A).double()
    assert abs(float(zt.mean())) < 5 / n ** 0.5 and abs(float(zt.var()) - 1) < 5 * (2 / n) ** 0.5
    assert not torch.equal(z, zt)


# ---- the update kernels against the fixtures ------------------------------------------------------------------
def _fixture(algo, B, A):
    with np.load(GOLDEN / U.fixture_name(algo, B, A)) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("algo", ["td3", "ddpg"])
@pytest.mark.parametrize("case", U.CASES, ids=lambda c: "B%d_A%d_D%d" % c)
def test_update_kernels_against_the_fixtures(ops, dev, algo, case):
    """The fused update of td3.TD3Trainer's train step on the fixture's batch and stub networks:
    each kernel's output, and the parameter gradients that flow from them."""
    B, A, D = case
    twin = algo == "td3"
    fx, h = _fixture(algo, B, A), U.HYPER
    nets = {k: v.to(dev) for k, v in U.package_networks(B, A, D, twin).items()}
    t = {k: v.to(dev) for k, v in U.stub_batch(B, A, D).items()}
    ac, ta = nets["actor"], nets["target_actor"]
    xa = torch.cat([t["obs"], t["actions"]], 1)
    nxa = torch.cat([t["next_obs"], torch.zeros_like(t["actions"])], 1)
    chk = lambda k, got: U.check(f"{algo} {k}", got, fx["f32_" + k], fx["f64_" + k])  # noqa: E731
    with torch.no_grad():
        mu_t = ta.pre(t["next_obs"])
        if twin:
            # the fixture holds torch's recorded draw z, not the library's stream: the kernel's
            # noise-free action plus the script's expression of that z (the kernel's own noisy
            # path is checked bitwise in test_target_actions_noise_and_noise_free)
            noise = (t["z"] * h["policy_noise"]).clamp(-h["noise_clip"], h["noise_clip"]) * ta.action_scale
            ops.td3_target_actions(mu_t, ta.action_scale, ta.action_bias, nxa)
            nxa[:, D:] = (nxa[:, D:] + noise).clamp(float(t["low"][0]), float(t["high"][0]))
        else:
            ops.td3_target_actions(mu_t, ta.action_scale, ta.action_bias, nxa)
        chk("next_actions", nxa[:, D:])
        q1t = nets["qf1_target"].q_values(nxa)
        q2t = nets["qf2_target"].q_values(nxa) if twin else None
    q1 = nets["qf1"].q_values(xa)
    q2 = nets["qf2"].q_values(xa) if twin else None
    y = torch.zeros(B, device=dev)
    stats, dq1, dq2 = ops.td3_critic_loss_fwd_bwd(
        q1t, q2t, q1.detach(), q2.detach() if twin else None, t["rewards"], t["dones"], h["gamma"],
        y_out=y)
    chk("next_q_value", y)
    chk("dq1", dq1.view(-1))
    grads = {}
    if twin:
        chk("dq2", dq2.view(-1))
        torch.autograd.backward([q1, q2], [dq1, dq2])
        grads.update({("qf2", k): p.grad.clone() for k, p in nets["qf2"].named_parameters()})
    else:
        assert dq2 is None and stats[1] == 0 and stats[3] == 0
        q1.backward(dq1)
    grads.update({("qf1", k): p.grad.clone() for k, p in nets["qf1"].named_parameters()})
    mu = ac.pre(t["obs"])
    mu.retain_grad()
    qa = nets["qf1"].q_values(ops.td3_policy_actions(mu, xa, ac.action_scale, ac.action_bias))
    torch.autograd.backward([qa], [torch.full_like(qa, -1.0 / B)], inputs=list(ac.parameters()) + [mu])
    chk("dmu", mu.grad)
    grads.update({("actor", k): p.grad for k, p in ac.named_parameters()})
    losses = [stats[0]] + ([stats[1]] if twin else []) + [-qa.mean()]
    chk("losses", torch.stack(losses))
    chk("grads", torch.cat([grads[k].reshape(-1) for k in U.grad_names(nets)]))
    pairs = [(ac.fc_mu.bias.detach().clone(), ta.fc_mu.bias.detach().clone()),
             (nets["qf1"].fc3.weight.detach().reshape(-1).clone(),
              nets["qf1_target"].fc3.weight.detach().reshape(-1).clone())]
    ops.polyak_(pairs, h["tau"])
    chk("polyak", torch.cat([p[1] for p in pairs]))
    # the mean q values (not in the fixtures): the f64 mean of the f32 outputs
    assert abs(float(stats[2]) - float(q1.double().mean())) <= 2.0 ** -22 * float(q1.abs().max())


@pytest.mark.parametrize("B,A,D", SHAPES)
def test_target_actions_noise_and_noise_free(ops, dev, B, A, D):
    lo, hi, scale, bias = _bounds(A, dev)
    g = torch.Generator().manual_seed(B + A)
    mu = (1.5 * torch.randn(B, A, generator=g)).to(dev)
    nxa = torch.full((B, D + A), 7.0, device=dev)
    ctr = torch.tensor([5], device=dev)
    pn, nc, l0, h0 = 0.5, 0.5, float(lo[0]), float(hi[0])
    ops.td3_target_actions(mu, scale, bias, nxa, 9, ctr, pn, nc, l0, h0)
    assert (nxa[:, :D] == 7).all()  # only the action columns are written
    words = U.target_words(9, 5, B, A)
    z = ops.td3_target_noise(9, ctr, B, A)
    U.check("z", z, U.box_muller(words, np.float32), U.box_muller(words, np.float64))
    # bitwise the script's expression on the kernel's own draws
    want = (torch.tanh(mu) * scale + bias + (z * pn).clamp(-nc, nc) * scale).clamp(l0, h0)
    assert torch.equal(nxa[:, D:], want)
    # policy_noise = 0: no stream (no counter needed) and no clamp to the bounds
    ops.td3_target_actions(mu, scale, bias, nxa)
    assert torch.equal(nxa[:, D:], torch.tanh(mu) * scale + bias)
    if A == 6:
        assert (nxa[:, D:] > h0).any()  # other dimensions' bounds are wider: nothing clamped them


@pytest.mark.parametrize("B", [1, 33, 64, 256, 1000])
def test_critic_loss_twin_single_and_repeatable(ops, dev, B):
    g = torch.Generator().manual_seed(B)
    q1t, q2t, q1, q2, r = (torch.randn(B, 1, generator=g).to(dev) for _ in range(5))
    d = (torch.arange(B, device=dev) % 2).float().view(B, 1)
    y = torch.zeros(B, device=dev)
    s, dq1, dq2 = ops.td3_critic_loss_fwd_bwd(q1t, q2t, q1, q2, r, d, 0.99, y_out=y)
    # elementwise parts: bitwise the script's expressions
    yw = r.flatten() + (1 - d.flatten()) * 0.99 * torch.min(q1t, q2t).view(-1)
    assert torch.equal(y, yw)
    norm = torch.tensor(2.0 / B, device=dev)
    assert torch.equal(dq1.view(-1), norm * (q1.view(-1) - yw))
    assert torch.equal(dq2.view(-1), norm * (q2.view(-1) - yw))
    ref = lambda q: float(((q.double().view(-1) - yw.double()) ** 2).mean())  # noqa: E731
    own = lambda q: float(torch.nn.functional.mse_loss(q.view(-1), yw))       # noqa: E731
    for i, q in ((0, q1), (1, q2)):
        assert abs(float(s[i]) - ref(q)) <= max(3 * abs(own(q) - ref(q)), U.FLOOR * ref(q))
    # run to run
    s2, _, _ = ops.td3_critic_loss_fwd_bwd(q1t, q2t, q1, q2, r, d, 0.99)
    assert torch.equal(s, s2)
    # the twin kernel fed q2 = q1 against the single-critic form
    st, e1, e2 = ops.td3_critic_loss_fwd_bwd(q1t, q1t, q1, q1, r, d, 0.99)
    ss, f1, f2 = ops.td3_critic_loss_fwd_bwd(q1t, None, q1, None, r, d, 0.99)
    assert f2 is None and torch.equal(e1, f1) and torch.equal(e2, f1)
    assert torch.equal(st[[0, 2]], ss[[0, 2]]) and torch.equal(st[[1, 3]], st[[0, 2]])
    assert (ss[[1, 3]] == 0).all()


@pytest.mark.parametrize("B,A,D", SHAPES)
def test_policy_actions_forward_and_backward(ops, dev, B, A, D):
    lo, hi, scale, bias = _bounds(A, dev)
    g = torch.Generator().manual_seed(B + 3 * A)
    mu = torch.randn(B, A, generator=g).to(dev).requires_grad_()
    xa = torch.randn(B, D + A, generator=g).to(dev)
    dxa = torch.randn(B, D + A, generator=g).to(dev)
    out = ops.td3_policy_actions(mu, xa, scale, bias)
    out.backward(dxa)
    mu2 = mu.detach().clone().requires_grad_()
    want = torch.cat([xa[:, :D], torch.tanh(mu2) * scale + bias], 1)
    want.backward(dxa)
    assert torch.equal(out, want) and out.data_ptr() != xa.data_ptr()
    assert torch.equal(mu.grad, mu2.grad)
    m64 = mu.detach().double().cpu().requires_grad_()
    (torch.tanh(m64) * scale.double().cpu() + bias.double().cpu()).backward(dxa[:, D:].double().cpu())
    U.check("dmu", mu.grad, mu2.grad, m64.grad)


@pytest.mark.parametrize("n", [1, 63, 70000])
def test_polyak_bitwise(ops, dev, n):
    g = torch.Generator().manual_seed(n)
    pairs = [(torch.randn(k, generator=g).to(dev), torch.randn(k, generator=g).to(dev))
             for k in (n, 3, n + 1, 64)]
    for tau in (0.005, 1.0):
        want = [tau * p + (1.0 - tau) * t for p, t in pairs]
        keep = [p.clone() for p, _ in pairs]
        ops.polyak_(pairs, tau)
        for (p, t), w, k in zip(pairs, want, keep):
            assert torch.equal(t, w) and torch.equal(p, k)
    ops.polyak_(pairs[:1], 0.5)
    with pytest.raises(ValueError, match="pairs"):
        ops.polyak_(pairs + pairs[:1], 0.5)
    with pytest.raises(ValueError, match="targets"):
        ops.polyak_([(pairs[0][0], pairs[1][1])], 0.5)
