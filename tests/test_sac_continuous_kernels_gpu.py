"""The continuous-SAC kernels (csrc/ocppo_sac_cont.hip) against the script's fixtures, the NumPy
twins (tests/sac_continuous_util.py) and torch's expressions in the kernels' restated order
(sac_continuous.squash, log_std_of): DESIGN 11's rule (error relative to the twin's largest element
at most max(3 x the f32 reference's own error, 4 * 2^-23)) unless a test says bitwise."""
import numpy as np
import pytest
import torch

import sac_continuous_util as U
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BS = (1, 255, 256, 257)  # the edges of the 256-thread row loop
AD = ((1, 3), (6, 5), (64, 2))
SEED = 9


@pytest.fixture(scope="module")
def ops():
    from oc_cleanrl_amd import ops

    return ops


@pytest.fixture(scope="module")
def sc():
    from oc_cleanrl_amd import sac_continuous

    return sac_continuous


def _bounds(A, dev):
    if A in U.BOUNDS:
        lo, hi = (torch.tensor(v, device=dev) for v in U.BOUNDS[A])
    else:
        lo = -(1.0 + torch.arange(A, device=dev) / A)
        hi = 0.5 + torch.arange(A, device=dev) / 8.0
    return lo, hi, (hi - lo) / 2.0, (hi + lo) / 2.0


def _heads(B, A, dev, seed=0):
    """mean, r [B, A]: x on both sides of tanh's saturation, log_std over its whole range."""
    g = torch.Generator().manual_seed(1000 * B + A + seed)
    return (1.5 * torch.randn(B, A, generator=g)).to(dev), (2.0 * torch.randn(B, A, generator=g)).to(dev)


def _temp(ops, dev, autotune=True, log_alpha=-0.5, lr=1e-3, A=1):
    t = ops.SacTemperature(dev, autotune, 0.2, lr=lr, target_entropy=-float(A), eps=1e-8)
    if autotune:
        t.log_alpha.fill_(log_alpha)
        t.alpha.copy_(t.log_alpha.exp())
    return t


# ---- acting ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("E,A", [(1, 1), (5, 6), (3, 64)])
def test_act_both_phases(ops, sc, dev, E, A, H):
    from oc_cleanrl_amd import td3

    seed, ls = 5, 10
    lo, hi, scale, bias = _bounds(A, dev)
    g = torch.Generator().manual_seed(E + 10 * A + H)
    h = torch.relu(torch.randn(E, H, generator=g)).to(dev)
    wm, wl = ((torch.randn(A, H, generator=g) / H ** 0.5).to(dev) for _ in range(2))
    bm, bl = ((0.1 * torch.randn(A, generator=g)).to(dev) for _ in range(2))
    step = torch.tensor([7], device=dev)
    act = lambda k: ops.csac_act(h, wm, bm, wl, bl, scale, bias, lo, hi, seed, step, ls,  # noqa: E731
                                 step_offset=k)
    # the uniform phase (t = 7, 9 < 10): bitwise low + (high - low) * u, inside [low, high)
    for k in (0, 2):
        a = act(k)
        u = U.unit24(U.act_words(seed, 7 + k, E, A)[..., 0])
        assert np.array_equal(ops.csac_noise(seed, step, E, A, offset=k, uniform=True).cpu().numpy(), u)
        assert torch.equal(a, lo + (hi - lo) * torch.from_numpy(u).to(dev))
        assert (a >= lo).all() and (a < hi).all()
    # the actor phase (t = 10): the draw against its twins, the action against the f64 expression
    a = act(3)
    words = U.act_words(seed, 10, E, A)
    z = ops.csac_noise(seed, step, E, A, offset=3)
    U.check("z", z, U.box_muller(words, np.float32), U.box_muller(words, np.float64))

    def ref(dtype, zz):
        c = lambda v: v.detach().cpu().to(dtype)  # noqa: E731
        mean, r = c(h) @ c(wm).t() + c(bm), c(h) @ c(wl).t() + c(bl)
        x = mean + torch.exp(sc.log_std_of(r)) * torch.as_tensor(zz).to(dtype)
        return torch.tanh(x) * c(scale) + c(bias)

    U.check("action", a, ref(torch.float32, U.box_muller(words, np.float32)),
            ref(torch.float64, U.box_muller(words, np.float64)))
    # ... and bitwise the unfused path's expression on the kernel's own draws
    mean, r = td3.act_mu(h, wm, bm), td3.act_mu(h, wl, bl)
    assert torch.equal(a, torch.tanh(mean + torch.exp(sc.log_std_of(r)) * z) * scale + bias)
    # a second launch, and a replayed graph
    assert torch.equal(a, act(3))
    out = torch.zeros_like(a)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        ops.csac_act(h, wm, bm, wl, bl, scale, bias, lo, hi, seed, step, ls, out, step_offset=3)
    out.zero_()
    gr.replay()
    assert torch.equal(out, a)
    step.fill_(2)  # the branch is on the device counter: the same graph now acts at random
    gr.replay()
    assert torch.equal(out, act(3)) and (out >= lo).all() and (out < hi).all()
    assert not torch.equal(out, a)


def test_uniform_phase_stays_below_high_and_draws_differ(ops, dev):
    lo, hi = torch.tensor([-2.0, 0.1], device=dev), torch.tensor([2.0, 0.3], device=dev)
    E, A = 2 ** 15, 2
    h, w, b = torch.zeros(E, 64, device=dev), torch.zeros(A, 64, device=dev), torch.zeros(A, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    a = ops.csac_act(h, w, b, w, b, (hi - lo) / 2, (hi + lo) / 2, lo, hi, 3, step, 1)
    assert (a >= lo).all() and (a < hi).all()
    assert abs(float(a[:, 0].mean())) < 5 * 4 / 12 ** 0.5 / E ** 0.5
    n = E * A  # 2^16 draws
    zs = [ops.csac_noise(3, step, E, A).double()] + \
        [ops.csac_noise(3, step, E, A, draw=d).double() for d in (0, 1, 2)]
    for z in zs:
        assert torch.isfinite(z).all()
        assert abs(float(z.mean())) < 5 / n ** 0.5 and abs(float(z.var()) - 1) < 5 * (2 / n) ** 0.5
    for i in range(4):  # the acting stream and the draw indices at one counter all differ
        for j in range(i):
            assert not torch.equal(zs[i], zs[j])
    w = U.update_words(3, 0, 2, 4, A)
    U.check("z", zs[3][:4], U.box_muller(w, np.float32), U.box_muller(w, np.float64))
    with pytest.raises(ValueError, match="acting stream"):
        ops.csac_noise(3, step, E, A, draw=1, uniform=True)


# ---- get_action ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A,D", AD)
@pytest.mark.parametrize("B", BS)
def test_sample_forward_bitwise_and_backward_under_the_rule(ops, sc, dev, B, A, D):
    lo, hi, scale, bias = _bounds(A, dev)
    mean, r = _heads(B, A, dev)
    mean.requires_grad_()
    r.requires_grad_()
    g = torch.Generator().manual_seed(B + A)
    obs_act = torch.randn(B, D + A, generator=g).to(dev)
    dxa, dlogp = torch.randn(B, D + A, generator=g).to(dev), torch.randn(B, 1, generator=g).to(dev)
    ctr = torch.tensor([5], device=dev)
    draw = ops.csac_policy_draw(1)
    xa, logp, y, z, ls = ops.csac_sample(mean, r, obs_act, scale, bias, SEED, ctr, draw, aux=True)
    words = U.update_words(SEED, 5, draw, B, A)
    assert torch.equal(z, ops.csac_noise(SEED, ctr, B, A, draw=draw))
    U.check("z", z, U.box_muller(words, np.float32), U.box_muller(words, np.float64))
    # bitwise the torch expression in the restated order, on the kernel's own draws
    m2, r2 = mean.detach().clone().requires_grad_(), r.detach().clone().requires_grad_()
    act, lp = sc.squash(m2, r2, z, scale, bias)
    assert xa.data_ptr() != obs_act.data_ptr() and torch.equal(xa[:, :D], obs_act[:, :D])
    assert torch.equal(xa[:, D:], act) and torch.equal(logp, lp) and logp.shape == (B, 1)
    assert torch.equal(ls, sc.log_std_of(r2)) and torch.equal(y, torch.tanh(m2 + torch.exp(ls) * z))
    # the forward-only mode: the same log_prob; with xa only the action columns are written
    nxa = torch.full((B, D + A), 7.0, device=dev)
    lp_only = ops.csac_sample_forward(mean.detach(), r.detach(), scale, bias, SEED, ctr, draw)
    lp_xa = ops.csac_sample_forward(mean.detach(), r.detach(), scale, bias, SEED, ctr, draw, xa=nxa)
    assert torch.equal(lp_only, logp) and torch.equal(lp_xa, logp)
    assert (nxa[:, :D] == 7).all() and torch.equal(nxa[:, D:], act)
    # backward: against autograd of the restated forward in f64, torch's f32 autograd as its own
    torch.autograd.backward([xa, logp], [dxa, dlogp])
    torch.autograd.backward([act, lp], [dxa[:, D:], dlogp])
    m64 = mean.detach().double().cpu().requires_grad_()
    r64 = r.detach().double().cpu().requires_grad_()
    a64, l64 = sc.squash(m64, r64, z.double().cpu(), scale.double().cpu(), bias.double().cpu())
    torch.autograd.backward([a64, l64], [dxa[:, D:].double().cpu(), dlogp.double().cpu()])
    U.check("dmean", mean.grad, m2.grad, m64.grad)
    U.check("dr", r.grad, r2.grad, r64.grad)
    # a second launch
    xa2, logp2 = ops.csac_sample(mean, r, obs_act, scale, bias, SEED, ctr, draw)
    assert torch.equal(xa2, xa) and torch.equal(logp2, logp)


def test_sample_and_alpha_step_in_a_replayed_graph(ops, dev):
    B, A, D = 257, 6, 5
    lo, hi, scale, bias = _bounds(A, dev)
    mean, r = _heads(B, A, dev)
    ctr = torch.tensor([5], device=dev)
    nxa = torch.zeros(B, D + A, device=dev)
    temp, loss = _temp(ops, dev, A=A), torch.zeros(1, device=dev)
    lp = torch.zeros(B, 1, device=dev)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        lp.copy_(ops.csac_sample_forward(mean, r, scale, bias, SEED, ctr, 2, xa=nxa))
        ops.csac_alpha_step(lp, temp, loss=loss)
    for c in (5, 6):  # the counter is read on the device: the replay at 6 draws afresh
        ctr.fill_(c)
        t2 = _temp(ops, dev, A=A)
        for k in ("log_alpha", "alpha", "exp_avg", "exp_avg_sq", "step"):
            getattr(t2, k).copy_(getattr(temp, k))
        gr.replay()
        want_xa = torch.zeros_like(nxa)
        want = ops.csac_sample_forward(mean, r, scale, bias, SEED, ctr, 2, xa=want_xa)
        l2 = ops.csac_alpha_step(want, t2)
        assert torch.equal(lp, want) and torch.equal(nxa, want_xa) and torch.equal(loss, l2)
        for k in ("log_alpha", "alpha", "exp_avg", "exp_avg_sq", "step"):
            assert torch.equal(getattr(t2, k), getattr(temp, k)), k
        prev = lp.clone() if c == 5 else prev
    assert not torch.equal(prev, lp) and int(temp.step) == 2


# ---- the losses ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BS)
def test_critic_loss_bitwise_rows_and_td3_equivalence(ops, dev, B):
    g = torch.Generator().manual_seed(B)
    q1t, q2t, q1, q2, r, nlp = (torch.randn(B, 1, generator=g).to(dev) for _ in range(6))
    d = (torch.arange(B, device=dev) % 2).float().view(B, 1)
    alpha = torch.tensor([0.37], device=dev)
    y = torch.zeros(B, device=dev)
    s, dq1, dq2 = ops.csac_critic_loss_fwd_bwd(q1t, q2t, q1, q2, r, d, nlp, alpha, 0.99, y_out=y)
    # elementwise parts: bitwise the script's expressions (:268-269, mse_loss's backward)
    m = torch.min(q1t, q2t) - alpha * nlp
    yw = r.flatten() + (1 - d.flatten()) * 0.99 * m.view(-1)
    assert torch.equal(y, yw)
    norm = torch.tensor(2.0 / B, device=dev)
    assert torch.equal(dq1.view(-1), norm * (q1.view(-1) - yw))
    assert torch.equal(dq2.view(-1), norm * (q2.view(-1) - yw))
    ref = lambda q: float(((q.double().view(-1) - yw.double()) ** 2).mean())  # noqa: E731
    own = lambda q: float(torch.nn.functional.mse_loss(q.view(-1), yw))       # noqa: E731
    for i, q in ((0, q1), (1, q2)):
        assert abs(float(s[i]) - ref(q)) <= max(3 * abs(own(q) - ref(q)), U.FLOOR * ref(q))
        assert abs(float(s[2 + i]) - float(q.double().mean())) <= 2.0 ** -22 * float(q.abs().max())
    # run to run
    s2, _, _ = ops.csac_critic_loss_fwd_bwd(q1t, q2t, q1, q2, r, d, nlp, alpha, 0.99)
    assert torch.equal(s, s2)
    # alpha = 0 (and q2 = q1): bitwise TD3's twin kernel, stats included
    zero = torch.zeros(1, device=dev)
    for b2t, b2 in ((q2t, q2), (q1t, q1)):
        sa, e1, e2 = ops.csac_critic_loss_fwd_bwd(q1t, b2t, q1, b2, r, d, nlp, zero, 0.99)
        st, f1, f2 = ops.td3_critic_loss_fwd_bwd(q1t, b2t, q1, b2, r, d, 0.99)
        assert torch.equal(sa, st) and torch.equal(e1, f1) and torch.equal(e2, f2)


@pytest.mark.parametrize("B", BS)
def test_actor_loss_against_autograd_bitwise_with_ties(ops, dev, B):
    g = torch.Generator().manual_seed(B + 1)
    q1, q2, lp = (torch.randn(B, 1, generator=g).to(dev) for _ in range(3))
    q2[::3] = q1[::3]  # ties: half the gradient each
    alpha = torch.tensor([0.37], device=dev)
    loss, dq1, dq2, dlogp = ops.csac_actor_loss_fwd_bwd(q1, q2, lp, alpha)
    a, b, c = (t.clone().requires_grad_() for t in (q1, q2, lp))
    own = ((alpha * c) - torch.min(a, b)).mean()  # :289-290
    own.backward()
    assert torch.equal(dq1, a.grad) and torch.equal(dq2, b.grad) and torch.equal(dlogp, c.grad)
    ref = float((alpha.double() * lp.double() - torch.min(q1, q2).double()).mean())
    scale = float((alpha * lp - torch.min(q1, q2)).abs().max())
    assert abs(float(loss) - ref) <= max(3 * abs(float(own.detach()) - ref), U.FLOOR * scale)
    l2, *_ = ops.csac_actor_loss_fwd_bwd(q1, q2, lp, alpha)
    assert torch.equal(loss, l2)


@pytest.mark.parametrize("B", BS)
def test_temperature_three_steps_against_torch_adam_f64(ops, dev, B):
    A, lr, la0 = 6, 1e-3, 0.0  # the script's initial log_alpha: the steps are all of it
    temp = _temp(ops, dev, log_alpha=la0, lr=lr, A=A)
    g = torch.Generator().manual_seed(B + 2)
    lps = [(3.0 * torch.randn(B, 1, generator=g) + 4.0 * (k - 1)) for k in range(3)]
    got, losses = [], []
    for lp in lps:
        losses.append(ops.csac_alpha_step(lp.to(dev), temp).clone())
        got.append(torch.cat([temp.log_alpha, temp.alpha]).cpu())
        assert torch.equal(temp.alpha, temp.log_alpha.exp())
    assert int(temp.step) == 3

    def ref(dtype):
        la = torch.tensor([la0], dtype=dtype, requires_grad=True)
        opt = torch.optim.Adam([la], lr=lr)
        out, ls = [], []
        for lp in lps:
            loss = (-la.exp() * (lp.to(dtype) + (-float(A)))).mean()  # :299
            opt.zero_grad()
            loss.backward()
            opt.step()
            out.append(torch.cat([la.detach(), la.detach().exp()]))
            ls.append(loss.detach().view(1))
        return torch.stack(out), torch.cat(ls)

    (o32, l32), (o64, l64) = ref(torch.float32), ref(torch.float64)
    U.check("log_alpha", torch.stack(got)[:, 0], o32[:, 0], o64[:, 0])
    U.check("alpha", torch.stack(got)[:, 1], o32[:, 1], o64[:, 1])
    U.check("alpha_loss", torch.cat(losses), l32, l64)


def test_autotune_off_leaves_the_temperature_untouched(ops, dev):
    temp = _temp(ops, dev, autotune=False)
    before = [getattr(temp, k).clone() for k in ("log_alpha", "alpha", "exp_avg", "exp_avg_sq", "step")]
    assert float(temp.alpha) == pytest.approx(0.2)
    with pytest.raises(ValueError, match="autotune off"):
        ops.csac_alpha_step(torch.zeros(4, 1, device=dev), temp)
    for k, b in zip(("log_alpha", "alpha", "exp_avg", "exp_avg_sq", "step"), before):
        assert torch.equal(getattr(temp, k), b), k


# ---- the update kernels against the fixtures ------------------------------------------------------------------
@pytest.mark.parametrize("case", U.CASES, ids=lambda c: "B%d_A%d_D%d" % c)
def test_update_kernels_against_the_fixtures(ops, sc, dev, case):
    """The fused update of sac_continuous.ContSACTrainer's train step on the fixture's batch and
    stub networks: each kernel's output, and the parameter gradients that flow from them. The
    fixture holds recorded draws, not the library's stream, so the sampling kernels read them
    (z=); their own draws are checked above."""
    B, A, D = case
    with np.load(GOLDEN / U.fixture_name(B, A)) as f:
        fx = {k: f[k] for k in f.files}
    h = U.HYPER
    nets, t = U.package_case(B, A, D)
    nets, t = {k: v.to(dev) for k, v in nets.items()}, {k: v.to(dev) for k, v in t.items()}
    chk = lambda k, got: U.check(k, got, fx["f32_" + k], fx["f64_" + k])  # noqa: E731
    ac = nets["actor"]
    temp = _temp(ops, dev, log_alpha=h["log_alpha"], lr=h["q_lr"], A=A)
    xa = torch.cat([t["obs"], t["actions"]], 1)
    nxa = torch.cat([t["next_obs"], torch.zeros_like(t["actions"])], 1)
    with torch.no_grad():
        nlp = ops.csac_sample_forward(*ac.heads(t["next_obs"]), ac.action_scale, ac.action_bias,
                                      xa=nxa, z=t["z_target"])
        chk("next_actions", nxa[:, D:])
        chk("next_log_pi", nlp.view(-1))
        q1t, q2t = nets["qf1_target"].q_values(nxa), nets["qf2_target"].q_values(nxa)
    q1, q2 = nets["qf1"].q_values(xa), nets["qf2"].q_values(xa)
    y = torch.zeros(B, device=dev)
    stats, dq1, dq2 = ops.csac_critic_loss_fwd_bwd(q1t, q2t, q1.detach(), q2.detach(), t["rewards"],
                                                   t["dones"], nlp, temp.alpha, h["gamma"], y_out=y)
    chk("next_q_value", y)
    chk("dq1", dq1.view(-1))
    chk("dq2", dq2.view(-1))
    torch.autograd.backward([q1, q2], [dq1, dq2])
    grads = {(m, k): p.grad.clone() for m in ("qf1", "qf2") for k, p in nets[m].named_parameters()}
    mean, r = ac.heads(t["obs"])
    mean.retain_grad()
    r.retain_grad()
    pxa, lp = ops.csac_sample(mean, r, xa, ac.action_scale, ac.action_bias, z=t["z_pi"])
    q1p, q2p = nets["qf1"].q_values(pxa), nets["qf2"].q_values(pxa)
    pi_loss, dqa1, dqa2, dlogp = ops.csac_actor_loss_fwd_bwd(q1p.detach(), q2p.detach(),
                                                             lp.detach(), temp.alpha)
    torch.autograd.backward([q1p, q2p, lp], [dqa1, dqa2, dlogp],
                            inputs=list(ac.parameters()) + [mean, r])
    chk("dmean", mean.grad)
    chk("dr", r.grad)
    grads.update({("actor", k): p.grad for k, p in ac.named_parameters()})
    chk("grads", torch.cat([grads[k].reshape(-1) for k in U.grad_names(nets)]))
    with torch.no_grad():
        lp2 = ops.csac_sample_forward(*ac.heads(t["obs"]), ac.action_scale, ac.action_bias,
                                      z=t["z_alpha"])
    alpha_loss = ops.csac_alpha_step(lp2, temp)
    chk("losses", torch.cat([stats[:2], pi_loss, alpha_loss]))
    chk("temp", torch.cat([temp.log_alpha, temp.alpha]))
    pairs = [(nets["qf1"].fc3.weight.detach().reshape(-1).clone(),
              nets["qf1_target"].fc3.weight.detach().reshape(-1).clone())]
    ops.polyak_(pairs, h["tau"])
    chk("polyak", pairs[0][1])
