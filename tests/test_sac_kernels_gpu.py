"""The three discrete-SAC launches (csrc/ocppo_sac.hip) against the float64 twin of
tests/sac_util.py by the error rule (lstm_util.check), over every action count and every batch
size around the wave and the workgroup (256 threads), and the acting stream against its
restatement in Python integers."""
import numpy as np
import pytest
import torch

import sac_util as su

pytestmark = pytest.mark.gpu

WG = 256  # kSacThreads
ACTIONS = [1, 2, 6, 18]
BATCHES = [1, 2, 63, 64, 65, WG - 1, WG, WG + 1]
ALPHAS = [1e-3, 0.2, 5.0]
GAMMA = float(np.float32(0.99))  # the kernel rounds gamma to f32 once: the twin's input is that


def te_of(A: int) -> float:
    """The trainer's target entropy for A actions (sac_atari.py:228), an f32 value."""
    return float(-0.89 * torch.log(1 / torch.tensor(A)))


LEAD_ALONE = -1


def make_inputs(B: int, A: int, seed: int = 0):
    """f32 CPU inputs: dones alternate 0 / 1; with more than one row, row 0's top logit leads by
    90 (p underflows, logp stays finite). Alone in a batch that row would leave a gradient whose
    every element lies in f32's subnormal range (p ~ 8e-40), where the format's precision is
    absolute (2^-149) and the rule's relative floor 4 * 2^-23 does not describe it:
    test_lead_row_alone covers that batch."""
    g = torch.Generator().manual_seed(1000 * A + B + seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    z = dict(next_logits=2 * r(B, A), logits=2 * r(B, A), q1t=r(B, A), q2t=r(B, A), q1=r(B, A),
             q2=r(B, A), actions=torch.randint(0, A, (B,), generator=g),
             rewards=torch.sign(r(B)) * (torch.rand(B, generator=g) < 0.5),
             dones=(torch.arange(B) % 2).float())
    if B > 1 or seed == LEAD_ALONE:
        for k in ("next_logits", "logits"):
            z[k][0] = 0.0
            z[k][0, B % A] = 90.0
    return z


def log_of(alpha: float):
    """The f32 log_alpha the tests start from (an input: the same value on both sides)."""
    return torch.log(torch.tensor([alpha], dtype=torch.float32))


def assert_alpha_is_exp(alpha, log_alpha):
    """alpha = exp(log_alpha): two f32 evaluations of exp on one f32 argument, each within an ulp
    of the true value, differ by at most 2 ulp."""
    a, e = alpha.item(), float(torch.exp(log_alpha.double().cpu()))
    assert abs(a - e) <= 2.0 ** -22 * e, (a, e)


@pytest.fixture(scope="module")
def cases():
    """Inputs and both references (the f64 twin, the f32 torch computation), computed once."""
    out = {}
    for A in ACTIONS:
        for B in BATCHES:
            z = make_inputs(B, A)
            ref = {}
            for alpha in ALPHAS:
                for dt in (torch.float64, torch.float32):
                    c = lambda k: z[k].to(dt)  # noqa: E731
                    a_in = float(np.float32(alpha))
                    ref[alpha, dt, "critic"] = su.critic_ref(
                        c("next_logits"), c("q1t"), c("q2t"), c("q1"), c("q2"), z["actions"],
                        c("rewards"), c("dones"), GAMMA if dt == torch.float64 else 0.99, a_in)
                    ref[alpha, dt, "actor"] = su.actor_ref(
                        c("logits"), c("q1"), c("q2"), a_in, log_of(alpha).to(dt), te_of(A))
            out[A, B] = (z, ref)
    return out


def temperature(dev, alpha: float, autotune: bool, A: int):
    from oc_cleanrl_amd import ops

    t = ops.SacTemperature(dev, autotune, alpha, 3e-4, te_of(A))
    t.alpha.fill_(alpha)
    t.log_alpha.copy_(log_of(alpha))
    return t


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("A", ACTIONS)
def test_critic_kernel(dev, cases, A, B):
    from oc_cleanrl_amd import ops

    z, ref = cases[A, B]
    d = {k: v.to(dev) for k, v in z.items()}
    for alpha in ALPHAS:
        al = torch.tensor([alpha], dtype=torch.float32, device=dev)
        y = torch.full((B,), float("nan"), device=dev)
        stats, dq1, dq2 = ops.sac_critic_loss_fwd_bwd(
            d["next_logits"], d["q1t"], d["q2t"], d["q1"], d["q2"], d["actions"], d["rewards"],
            d["dones"], 0.99, al, y=y)
        twin, f32 = ref[alpha, torch.float64, "critic"], ref[alpha, torch.float32, "critic"]
        got = dict(y=y, qf1_loss=stats[0], qf2_loss=stats[1], qf1_values=stats[2],
                   qf2_values=stats[3], dq1=dq1, dq2=dq2)
        for k, v in got.items():
            assert torch.isfinite(v).all(), (k, alpha)
            su.check(f"critic A={A} B={B} alpha={alpha} {k}", v, f32[k], twin[k])
        # exact zeros away from the taken action
        mask = torch.ones(B, A, dtype=torch.bool, device=dev)
        mask[torch.arange(B, device=dev), d["actions"]] = False
        assert not dq1[mask].any() and not dq2[mask].any()
        assert al.item() == np.float32(alpha)  # read only
        # a done row's target is its reward
        assert torch.equal(y[1::2], d["rewards"][1::2])


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("A", ACTIONS)
def test_actor_kernel_losses_and_gradient(dev, cases, A, B):
    """autotune off: every output against the twin, alpha and log_alpha bit-unchanged."""
    from oc_cleanrl_amd import ops

    z, ref = cases[A, B]
    d = {k: v.to(dev) for k, v in z.items()}
    ck = su.Checks()
    for alpha in ALPHAS:
        twin, f32 = ref[alpha, torch.float64, "actor"], ref[alpha, torch.float32, "actor"]
        t = temperature(dev, alpha, False, A)
        a0, la0 = t.alpha.clone(), t.log_alpha.clone()
        stats, dl = ops.sac_actor_alpha_fwd_bwd(d["logits"], d["q1"], d["q2"], t)
        assert torch.isfinite(stats).all() and torch.isfinite(dl).all()
        ck.check(f"actor A={A} B={B} alpha={alpha} loss", stats[0], f32["actor_loss"],
                 twin["actor_loss"])
        ck.check(f"actor A={A} B={B} alpha={alpha} dlogits", dl, f32["dlogits"], twin["dlogits"])
        ck.check(f"actor A={A} B={B} alpha={alpha} entropy", stats[3], f32["entropy"],
                 twin["entropy"])
        assert stats[1].item() == 0.0  # no temperature loss without autotune
        assert torch.equal(t.alpha, a0) and torch.equal(t.log_alpha, la0)
        assert stats[2].item() == a0.item() and t.step.item() == 0
        assert not t.exp_avg.any() and not t.exp_avg_sq.any()
        # autotune on, one launch: the temperature loss and the same policy outputs
        t = temperature(dev, alpha, True, A)
        stats2, dl2 = ops.sac_actor_alpha_fwd_bwd(d["logits"], d["q1"], d["q2"], t)
        assert torch.equal(dl2, dl) and torch.equal(stats2[0], stats[0])
        ck.check(f"actor A={A} B={B} alpha={alpha} alpha_loss", stats2[1], f32["alpha_loss"],
                 twin["alpha_loss"])
        assert t.alpha.item() == stats2[2].item()
        assert_alpha_is_exp(t.alpha, t.log_alpha)
        assert t.step.item() == 1
    ck.done()


@pytest.mark.parametrize("A,B", [(6, 64), (18, WG + 1), (2, 1)])
def test_temperature_adam_state_over_three_launches(dev, A, B):
    """Three consecutive launches carry exp_avg / exp_avg_sq / step: log_alpha follows
    torch.optim.Adam([log_alpha], lr, eps=1e-4) on the CPU; alpha = exp(log_alpha) after each."""
    from oc_cleanrl_amd import ops

    lr = 3e-4
    batches = [make_inputs(B, A, seed=s) for s in (1, 2, 3)]

    def reference(dt):
        la = torch.zeros(1, dtype=dt, requires_grad=True)
        opt = torch.optim.Adam([la], lr=lr, eps=1e-4)
        hist = []
        for z in batches:
            logp, p = su.get_action_ref(z["logits"].to(dt))
            loss = (p * (-la.exp() * (logp + te_of(A)))).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            st = opt.state[la]
            hist.append(dict(loss=loss.detach(), log_alpha=la.detach().clone(),
                             alpha=la.detach().exp(), exp_avg=st["exp_avg"].clone(),
                             exp_avg_sq=st["exp_avg_sq"].clone()))
        return hist

    twin, f32 = reference(torch.float64), reference(torch.float32)
    t = ops.SacTemperature(dev, True, 0.2, lr, te_of(A))
    assert t.alpha.item() == 1.0 and t.log_alpha.item() == 0.0
    for i, z in enumerate(batches):
        d = {k: v.to(dev) for k, v in z.items()}
        stats, _ = ops.sac_actor_alpha_fwd_bwd(d["logits"], d["q1"], d["q2"], t)
        assert t.step.item() == i + 1
        got = dict(loss=stats[1], log_alpha=t.log_alpha, alpha=t.alpha, exp_avg=t.exp_avg,
                   exp_avg_sq=t.exp_avg_sq)
        for k, v in got.items():
            su.check(f"temperature A={A} B={B} step {i + 1} {k}", v, f32[i][k], twin[i][k])
        assert t.alpha.item() == stats[2].item()
        assert_alpha_is_exp(t.alpha, t.log_alpha)
    assert t.log_alpha.item() != 0.0


@pytest.mark.parametrize("A", [2, 6, 18])
def test_lead_row_alone(dev, A):
    """A batch of the one row whose top logit leads by 90: nothing is NaN or infinite, the outputs
    of ordinary size follow the rule, and the gradient w.r.t. the logits and the entropy, whose
    true values are below f32's smallest normal number, are no larger than that."""
    from oc_cleanrl_amd import ops

    z = make_inputs(1, A, seed=LEAD_ALONE)
    assert float(z["logits"].max()) == 90.0 and z["dones"][0] == 0
    d = {k: v.to(dev) for k, v in z.items()}
    tiny = float(np.finfo(np.float32).tiny)
    for alpha in ALPHAS:
        al = torch.tensor([alpha], dtype=torch.float32, device=dev)
        y = torch.empty(1, device=dev)
        stats, dq1, dq2 = ops.sac_critic_loss_fwd_bwd(
            d["next_logits"], d["q1t"], d["q2t"], d["q1"], d["q2"], d["actions"], d["rewards"],
            d["dones"], 0.99, al, y=y)
        t = temperature(dev, alpha, True, A)
        pst, dl = ops.sac_actor_alpha_fwd_bwd(d["logits"], d["q1"], d["q2"], t)
        for v in (stats, dq1, dq2, y, pst, dl, t.alpha, t.log_alpha):
            assert torch.isfinite(v).all()
        ref = {}
        for dt in (torch.float64, torch.float32):
            c = lambda k: z[k].to(dt)  # noqa: E731
            a_in = float(np.float32(alpha))
            ref[dt] = dict(
                su.critic_ref(c("next_logits"), c("q1t"), c("q2t"), c("q1"), c("q2"),
                              z["actions"], c("rewards"), c("dones"),
                              GAMMA if dt == torch.float64 else 0.99, a_in),
                **su.actor_ref(c("logits"), c("q1"), c("q2"), a_in, log_of(alpha).to(dt),
                               te_of(A)))
        got = dict(y=y, qf1_loss=stats[0], qf2_loss=stats[1], dq1=dq1, dq2=dq2,
                   actor_loss=pst[0], alpha_loss=pst[1])
        for k, v in got.items():
            su.check(f"lead row A={A} alpha={alpha} {k}", v, ref[torch.float32][k],
                     ref[torch.float64][k])
        # |dlogits| <= p (|g| + |s|) with p < tiny off the top (and g = s to rounding at it),
        # |g| <= alpha * 91 + |q|; entropy: A - 1 terms p |logp| with |logp| < 100
        small = tiny * (alpha * 91 + 10)
        assert float(ref[torch.float64]["dlogits"].abs().max()) < small
        assert float(dl.abs().max()) < small and abs(pst[3].item()) < A * 100 * tiny


def test_critic_reads_the_alpha_the_actor_launch_wrote(dev):
    from oc_cleanrl_amd import ops

    z = {k: v.to(dev) for k, v in make_inputs(8, 6).items()}
    t = ops.SacTemperature(dev, True, 0.2, 0.05, te_of(6))
    args = (z["next_logits"], z["q1t"], z["q2t"], z["q1"], z["q2"], z["actions"], z["rewards"],
            z["dones"], 0.99)
    y0 = torch.empty(8, device=dev)
    ops.sac_critic_loss_fwd_bwd(*args, t.alpha, y=y0)
    ops.sac_actor_alpha_fwd_bwd(z["logits"], z["q1"], z["q2"], t)
    y1 = torch.empty(8, device=dev)
    ops.sac_critic_loss_fwd_bwd(*args, t.alpha, y=y1)
    assert t.alpha.item() != 1.0
    assert not torch.equal(y0[0::2], y1[0::2]) and torch.equal(y0[1::2], y1[1::2])


@pytest.mark.parametrize("n", [1, 3, 64, 1025])
def test_flat_adam_exact_follows_torch_adam(dev, n):
    """ops.FlatAdamExact over a weight and a bias that starts at zero, four steps with eps 1e-4:
    parameters and both moments against torch.optim.Adam on the CPU by the rule. Gradients from
    far below eps to far above it."""
    from oc_cleanrl_amd import ops

    g = torch.Generator().manual_seed(n)
    w0 = torch.randn(n, 3, generator=g)
    grads = [(torch.randn(n, 3, generator=g) * 10.0 ** torch.randint(-6, 1, (n, 3), generator=g),
              torch.randn(n, generator=g) * 10.0 ** torch.randint(-6, 1, (n,), generator=g))
             for _ in range(4)]

    def reference(dt):
        ps = [w0.to(dt).clone().requires_grad_(), torch.zeros(n, dtype=dt, requires_grad=True)]
        opt = torch.optim.Adam(ps, lr=3e-4, eps=1e-4)
        for gw, gb in grads:
            ps[0].grad, ps[1].grad = gw.to(dt), gb.to(dt)
            opt.step()
        return [p.detach() for p in ps] + [opt.state[p][k] for p in ps
                                           for k in ("exp_avg", "exp_avg_sq")]

    twin, f32 = reference(torch.float64), reference(torch.float32)
    ps = [torch.nn.Parameter(w0.clone().to(dev)), torch.nn.Parameter(torch.zeros(n, device=dev))]
    opt = ops.FlatAdamExact(ps, lr=3e-4, eps=1e-4)
    for gw, gb in grads:
        ps[0].grad.copy_(gw)
        ps[1].grad.copy_(gb)
        opt.step()
    offs, _ = ops.flat_offsets(ps)
    moments = [buf[o:o + p.numel()].view_as(p) for p, o in zip(ps, offs)
               for buf in (opt.exp_avg, opt.exp_avg_sq)]
    names = ["weight", "bias", "weight exp_avg", "weight exp_avg_sq", "bias exp_avg",
             "bias exp_avg_sq"]
    for name, got, a, b in zip(names, [p.detach() for p in ps] + moments, f32, twin):
        su.check(f"FlatAdamExact n={n} {name}", got, a, b)
    assert opt.scalars[0].item() >= 0 and torch.isfinite(opt.scalars).all()


# ---- acting -----------------------------------------------------------------------------------------
E_ACT, LS, SEED = 4096, 100, 5


def act_logits(A: int):
    return 2 * torch.randn(E_ACT, A, generator=torch.Generator().manual_seed(1234 + A))


@pytest.mark.parametrize("A", [2, 6, 18])
def test_act_matches_the_stream_restatement(dev, A):
    from oc_cleanrl_amd import ops

    logits = act_logits(A)
    lg = logits.to(dev)
    step = torch.tensor([LS - 1], dtype=torch.int64, device=dev)
    # random phase: exact
    rnd = ops.sac_act(lg, SEED, step, LS).cpu().tolist()
    want, _ = su.act_ref(logits, SEED, LS - 1, LS)
    assert rnd == want
    # the same launch arguments, only the device counter differs: the other branch
    step.add_(1)
    got = ops.sac_act(lg, SEED, step, LS).cpu().tolist()
    want, gaps = su.act_ref(logits, SEED, LS, LS)
    clear = [g > 1e-4 for g in gaps]
    print(f"A={A}: {clear.count(False)} rows within 1e-4")
    assert clear.count(False) <= 4
    assert [g for g, c in zip(got, clear) if c] == [w for w, c in zip(want, clear) if c]
    assert got != rnd
    # step_offset is added to the counter: t = LS - 1 again
    assert ops.sac_act(lg, SEED, step, LS, step_offset=-1).cpu().tolist() == rnd
    # another seed, another stream
    assert ops.sac_act(lg, SEED + 1, step, LS).cpu().tolist() != got


@pytest.mark.parametrize("A", [2, 6, 18])
def test_act_with_a_lead_of_90_is_the_argmax(dev, A):
    from oc_cleanrl_amd import ops

    logits = act_logits(A)
    top = torch.randint(0, A, (E_ACT,), generator=torch.Generator().manual_seed(A))
    logits[torch.arange(E_ACT), top] = logits.max() + 90.0
    step = torch.tensor([LS], dtype=torch.int64, device=dev)
    got = ops.sac_act(logits.to(dev), SEED, step, LS)
    assert torch.equal(got.cpu(), top)


def test_act_one_action_and_graph_replay(dev):
    from oc_cleanrl_amd import ops

    step = torch.tensor([LS + 3], dtype=torch.int64, device=dev)
    assert not ops.sac_act(torch.zeros(5, 1, device=dev), SEED, step, LS).any()
    lg = act_logits(6).to(dev)
    out = torch.empty(E_ACT, dtype=torch.int64, device=dev)
    ops.sac_act(lg, SEED, step, LS, out)
    eager = out.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.sac_act(lg, SEED, step, LS, out)
    out.zero_()
    g.replay()
    assert torch.equal(out, eager)
    step.add_(1)  # the captured launch reads the counter on the device
    g.replay()
    assert not torch.equal(out, eager)
