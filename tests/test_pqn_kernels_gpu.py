"""The PQN kernels (csrc/ocppo_pqn.hip, ocppo_clip_radam_step) against the plain-torch twins of
tests/pqn_util.py: bitwise where the kernel restates torch's f32 ops one by one (Q(lambda), the
greedy value, the exploration draw, the zeros of dq), else by the DESIGN 11 rule -- error against
the f64 twin, relative to the twin's largest element, <= max(3 x the f32 torch computation's own
error, 4 * 2^-23)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import pqn_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from oc_cleanrl_amd import ops

    return ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- Q(lambda) -----------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 5])
def test_q_lambda_is_bitwise_the_f32_loop(ops, dev, T):
    g = _gen(100 + T)
    for N in (1, 3, 64, 65):
        for A in (1, 6):
            rewards = torch.randn(T, N, generator=g)
            values = torch.randn(T, N, generator=g) * 3
            next_q = torch.randn(N, A, generator=g) * 3
            rnd = (torch.rand(T, N, generator=g) < 0.3).float()
            rnd_next = (torch.rand(N, generator=g) < 0.3).float()
            zT, zN = torch.zeros(T, N), torch.zeros(N)
            last = zT.clone()
            last[T - 1] = 1.0
            patterns = {"none": (zT, zN), "all": (zT + 1, zN + 1), "last": (last, zN),
                        "next": (zT, zN + 1), "random": (rnd, rnd_next)}
            for name, (dones, next_done) in patterns.items():
                for lam in (0.0, 0.65, 1.0):
                    want = U.q_lambda_ref(rewards, values, dones, next_q, next_done, 0.99, lam)
                    got = ops.q_lambda(rewards.to(dev), values.to(dev), dones.to(dev),
                                       next_q.to(dev), next_done.to(dev), 0.99, lam)
                    assert torch.equal(got.cpu(), want), (T, N, A, name, lam)


# ---- LayerNorm + ReLU ----------------------------------------------------------------------------
LN_E = [1, 2, 63, 64, 65, 255, 256, 257, 512, 1023, 1024]


def _ln_check(ops, dev, x, w, b, dy, relu=True, eps=1e-5, tag=""):
    y, mean, rstd = ops.ln_relu_fwd(x.to(dev), w.to(dev), b.to(dev), eps, relu)
    dx, dw, db = ops.ln_relu_bwd(dy.to(dev), x.to(dev), y, w.to(dev), mean, rstd, relu)
    got = dict(y=y, mean=mean, rstd=rstd, dx=dx, dw=dw, db=db)
    f32 = U.ln_relu_case(x, w, b, dy, eps, relu, torch.float32)
    twin = U.ln_relu_case(x, w, b, dy, eps, relu, torch.float64)
    for k in got:
        U.check(f"ln_relu{tag} {tuple(x.shape)} {k}", got[k], f32[k], twin[k])
    return got


@pytest.mark.parametrize("E", LN_E)
def test_ln_relu_by_the_rule_and_deterministic(ops, dev, E):
    g = _gen(200 + E)
    for R in (1, 3, 17):
        x = torch.randn(R, E, generator=g) * 2 + 0.5
        w = torch.rand(E, generator=g) + 0.5
        b = torch.randn(E, generator=g) * 0.5
        dy = torch.randn(R, E, generator=g)
        for relu in (True, False):
            a = _ln_check(ops, dev, x, w, b, dy, relu, tag=f" relu={int(relu)}")
            again = _ln_check(ops, dev, x, w, b, dy, relu, tag=f" relu={int(relu)} again")
            for k in a:  # two runs, bit for bit
                assert torch.equal(a[k], again[k]), k
            if relu:
                assert bool((a["y"] >= 0).all())


def test_ln_relu_autograd_function(ops, dev):
    g = _gen(7)
    x = torch.randn(3, 5, 65, generator=g)  # leading dims are rows
    w, b = torch.rand(65, generator=g) + 0.5, torch.randn(65, generator=g)
    dy = torch.randn(3, 5, 65, generator=g)
    xs, ws, bs = (t.to(dev).requires_grad_() for t in (x, w, b))
    y = ops.ln_relu(xs, ws, bs)
    y.backward(dy.to(dev))
    f32 = U.ln_relu_case(x, w, b, dy, 1e-5, True, torch.float32)
    twin = U.ln_relu_case(x, w, b, dy, 1e-5, True, torch.float64)
    for k, got in (("y", y.detach()), ("dx", xs.grad), ("dw", ws.grad), ("db", bs.grad)):
        U.check(f"ln_relu autograd {k}", got, f32[k], twin[k])


@pytest.mark.parametrize("E", [65, 1024])
def test_ln_relu_special_rows(ops, dev, E):
    g = _gen(300 + E)
    w = torch.rand(E, generator=g) + 0.5
    b = torch.randn(E, generator=g) * 0.5
    dy = torch.randn(3, E, generator=g)
    # a constant row: variance 0, rstd = eps^-1/2, finite output
    x = torch.randn(3, E, generator=g)
    x[1] = 0.7
    got = _ln_check(ops, dev, x, w, b, dy, tag=" const")
    assert abs(float(got["rstd"][1]) - 1e-5 ** -0.5) <= 1e-5 ** -0.5 * 2.0 ** -20
    assert bool(torch.isfinite(got["y"]).all()) and bool(torch.isfinite(got["dx"]).all())
    # a row of 1000 + small noise: the variance is taken about the mean
    x = torch.randn(3, E, generator=g)
    x[2] = 1000.0 + 1e-2 * torch.randn(E, generator=g)
    _ln_check(ops, dev, x, w, b, dy, tag=" offset")
    _ln_check(ops, dev, x[2:3].contiguous(), w, b, dy[2:3].contiguous(), tag=" offset alone")
    # all-negative pre-activations: y = 0 and dx = 0 exactly
    x = torch.randn(3, E, generator=g)
    neg = -(w * 6 + 1)  # the normalised rows stay within [-6, 6] (checked): xhat w + neg <= -1
    assert float(((x - x.mean(-1, keepdim=True)) / x.std(-1, keepdim=True)).abs().max()) < 6
    y, mean, rstd = ops.ln_relu_fwd(x.to(dev), w.to(dev), neg.to(dev), 1e-5, True)
    dx, dw, db = ops.ln_relu_bwd(dy.to(dev), x.to(dev), y, w.to(dev), mean, rstd, True)
    assert bool((y == 0).all()) and bool((dx == 0).all())
    assert bool((dw == 0).all()) and bool((db == 0).all())


# ---- the acting step ------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [4, 1024])
@pytest.mark.parametrize("A", [1, 6, 18])
def test_pqn_act(ops, dev, A, H):
    g = _gen(400 + A + H)
    seed = 1234
    for N in (1, 63, 64, 65):
        hidden = torch.randn(N, H, generator=g)
        wq = torch.randn(A, H, generator=g) * H ** -0.5
        bq = torch.randn(A, generator=g) * 0.1
        if A >= 6:  # tied maxima: actions 2 and 4 share a row and a bias, and dominate
            wq[4] = wq[2]
            bq[2] = bq[4] = 50.0
        assert ops.pqn_act_ok(hidden.to(dev), wq.to(dev))
        step = torch.zeros(1, dtype=torch.int64, device=dev)
        q_out = torch.empty(N, A, device=dev)
        eps = torch.empty(1, device=dev)
        h, w, b = hidden.to(dev), wq.to(dev), bq.to(dev)
        # a schedule past its duration with end_e = 0: all greedy
        act, val = ops.pqn_act(h, w, b, seed, step, 1.0, 0.0, 10.0, epsilon_out=eps,
                               step_offset=11, q_out=q_out)
        f32 = hidden @ wq.t() + bq
        twin = hidden.double() @ wq.double().t() + bq.double()
        U.check(f"pqn_act q N={N} A={A} H={H}", q_out, f32, twin)
        q = q_out.cpu()
        assert torch.equal(val.cpu(), q.max(1).values)
        assert torch.equal(act.cpu(), torch.argmax(q, dim=1))  # CPU argmax: the lowest index
        if A >= 6:
            assert bool((act == 2).all())
        assert float(eps) == 0.0
        # the same seed and step: ops.epsilon_greedy's actions on those Q values, exactly
        for t in range(6):
            act, _ = ops.pqn_act(h, w, b, seed, step, 1.0, 0.05, 8.0, epsilon_out=eps,
                                 step_offset=t)
            want = ops.epsilon_greedy(q_out, seed, step, 1.0, 0.05, 8.0, step_offset=t)
            assert torch.equal(act, want), (N, A, H, t)
            assert abs(float(eps) - U.linear_schedule(1.0, 0.05, 8.0, t)) <= 1e-7
        # start_e = 1 at step 0: every env explores, actions within [0, A)
        act, _ = ops.pqn_act(h, w, b, seed, step, 1.0, 0.01, 100.0)
        assert int(act.min()) >= 0 and int(act.max()) < A
        if A == 18 and N >= 63:
            assert len(set(act.cpu().tolist())) > 1  # random actions, not one greedy index


def test_pqn_act_ok_contract(ops, dev):
    f = lambda n, h: torch.zeros(n, h, device=dev)  # noqa: E731
    assert ops.pqn_act_ok(f(4, 32), f(18, 32)) and ops.pqn_act_ok(f(4, 1024), f(1, 1024))
    assert not ops.pqn_act_ok(f(4, 32), f(19, 32))
    assert not ops.pqn_act_ok(f(4, 30), f(6, 30))
    assert not ops.pqn_act_ok(f(4, 1028), f(6, 1028))
    assert not ops.pqn_act_ok(f(4, 32), f(6, 64))
    assert not ops.pqn_act_ok(f(4, 33)[:, 1:], f(6, 32))
    with pytest.raises(ValueError, match="pqn_act_ok"):
        ops.pqn_act(f(4, 30), f(6, 30), f(1, 6)[0], 0, torch.zeros(1, dtype=torch.int64,
                                                                  device=dev), 1.0, 0.1, 10.0)


# ---- the loss -------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [1, 2, 18])
def test_pqn_loss(ops, dev, A):
    g = _gen(500 + A)
    for M in (1, 2, 255, 256, 257):
        q = torch.randn(M, A, generator=g) * 2
        actions = torch.randint(0, A, (M,), generator=g)
        returns = torch.randn(M, generator=g) * 2
        stats, dq = ops.pqn_loss_fwd_bwd(q.to(dev), actions.to(dev), returns.to(dev))
        l32, m32, d32 = U.mse_step(q, actions, returns)
        l64, m64, d64 = U.mse_step(q.double(), actions, returns.double())
        U.check(f"pqn_loss M={M} A={A} mse", stats[0], l32, l64)
        U.check(f"pqn_loss M={M} A={A} mean q", stats[1], m32, m64)
        U.check(f"pqn_loss M={M} A={A} dq", dq, d32, d64)
        off = torch.ones(M, A, dtype=torch.bool)
        off[torch.arange(M), actions] = False
        assert bool((dq.cpu()[off] == 0).all())


# ---- RAdam ----------------------------------------------------------------------------------------
NUMELS = (1, 63, 64, 65, 1025)
LRS = (1e-2, 1e-2, 5e-3, 5e-3, 2e-2, 1e-3, 1e-2, 7e-3)  # changed on the device between steps


def _radam_inputs(seed, scale):
    g = _gen(seed)
    params = [torch.randn(n, generator=g) for n in NUMELS]
    grads = [[torch.randn(n, generator=g) * scale for n in NUMELS] for _ in range(8)]
    return params, grads


def _twin(params, grads, max_norm, dtype):
    """8 clipped steps on `dtype` CPU copies: (params, exp_avg, exp_avg_sq) after the last."""
    ps = [p.to(dtype).clone() for p in params]
    ref = U.RAdamRef(ps, LRS[0])
    for s in range(8):
        ref.lr = float(np.float32(LRS[s]))
        gs = [g.to(dtype) for g in grads[s]]
        c, _ = U.clip_coef(gs, max_norm)
        ref.step([g * c for g in gs])
    return ref.params, ref.m, ref.v


def _views(ops, opt):
    offs, _ = ops.flat_offsets(opt.param_list)
    cut = lambda buf: [buf[o:o + p.numel()].cpu() for p, o in zip(opt.param_list, offs)]  # noqa: E731
    return cut(opt.params), cut(opt.exp_avg), cut(opt.exp_avg_sq)


def _padding_is_zero(ops, opt):
    offs, n = ops.flat_offsets(opt.param_list)
    pad = torch.ones(n, dtype=torch.bool)
    for p, o in zip(opt.param_list, offs):
        pad[o:o + p.numel()] = False
    assert int(pad.sum()) > 0
    for buf in (opt.params, opt.exp_avg, opt.exp_avg_sq):
        assert bool((buf.cpu()[pad] == 0).all())


def _run_flat(ops, dev, cls, params, grads, max_norm, graph=False, **kw):
    ps = [torch.nn.Parameter(p.clone().to(dev)) for p in params]
    opt = cls(ps, lr=LRS[0], max_grad_norm=max_norm, **kw)
    offs, _ = ops.flat_offsets(opt.param_list)
    staged = torch.zeros_like(opt.grads)
    g = None
    if graph:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            opt.grads.copy_(staged)
            opt.step()
        # the capture ran nothing: state and step count are as constructed
    for sidx in range(8):
        opt.lr.fill_(LRS[sidx])
        staged.zero_()
        for gr, o in zip(grads[sidx], offs):
            staged[o:o + gr.numel()] = gr.to(dev)
        if graph:
            g.replay()
        else:
            opt.grads.copy_(staged)
            opt.step()
    torch.cuda.synchronize()
    return opt


@pytest.mark.parametrize("clipping", [True, False])
def test_flat_radam(ops, dev, clipping):
    """8 steps across the rectification boundary (step 6), several parameters with FLAT_ALIGN
    padding between them, lr changed on the device, clipping active or not."""
    max_norm = 10.0
    params, grads = _radam_inputs(11, 5.0 if clipping else 0.05)
    norms = [float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs))) for gs in grads]
    assert all(n > max_norm for n in norms) if clipping else all(n < max_norm for n in norms)
    opt = _run_flat(ops, dev, ops.FlatRAdam, params, grads, max_norm)
    f32 = _twin(params, grads, max_norm, torch.float32)
    twin = _twin(params, grads, max_norm, torch.float64)
    got = _views(ops, opt)
    for name, gl, fl, tl in zip(("param", "exp_avg", "exp_avg_sq"), got, f32, twin):
        for n, a, b, c in zip(NUMELS, gl, fl, tl):
            U.check(f"radam clip={clipping} {name}[{n}]", a, b, c)
    _padding_is_zero(ops, opt)
    sc = opt.scalars.cpu()
    assert float(sc[0]) == 8.0 and float(sc[5]) > 0  # 8 steps taken, the last one rectified
    assert abs(float(sc[1]) - norms[-1]) <= 1e-5 * norms[-1]
    # captured and replayed: bitwise the eager run
    cap = _run_flat(ops, dev, ops.FlatRAdam, params, grads, max_norm, graph=True)
    for a, b in ((opt.params, cap.params), (opt.exp_avg, cap.exp_avg),
                 (opt.exp_avg_sq, cap.exp_avg_sq), (opt.scalars, cap.scalars)):
        assert torch.equal(a, b)


def test_flat_radam_first_steps_are_unrectified(ops, dev):
    params, grads = _radam_inputs(13, 0.05)
    ps = [torch.nn.Parameter(p.clone().to(dev)) for p in params]
    opt = ops.FlatRAdam(ps, lr=1e-2, max_grad_norm=10.0)
    offs, _ = ops.flat_offsets(opt.param_list)
    rect = []
    for s in range(8):
        for gr, o in zip(grads[s], offs):
            opt.grads[o:o + gr.numel()] = gr.to(dev)
        opt.step()
        rect.append(float(opt.scalars[5]) > 0)
    assert rect == [False] * 5 + [True] * 3
    with pytest.raises(ValueError, match="planes"):
        opt.write_planes([(ps[0], 0, None)])


def test_flat_adam_is_unchanged_beside_radam(ops, dev):
    """FlatAdam on the same inputs against torch.optim.Adam, with the bound the existing tests put
    on it (tests/test_trainer_gpu.py: 1 % of one step of lr on a parameter), now that
    ocppo_clip_radam_step shares its norm kernel. The moments against the f64 run to 2e-5: the
    Adam kernel (unchanged here) forms 1 - beta2 in f32, 1.3e-5 off torch's double 0.001, which
    is all of exp_avg_sq's error (measured 1.296e-5; torch's own f32 error is 4e-8)."""
    max_norm = 10.0
    params, grads = _radam_inputs(11, 5.0)
    opt = _run_flat(ops, dev, ops.FlatAdam, params, grads, max_norm, eps=1e-5)

    def adam(dtype):
        ps = [p.to(dtype).clone().requires_grad_() for p in params]
        o = torch.optim.Adam(ps, lr=LRS[0], eps=1e-5)
        for s in range(8):
            o.param_groups[0]["lr"] = float(np.float32(LRS[s]))
            gs = [g.to(dtype) for g in grads[s]]
            c, _ = U.clip_coef(gs, max_norm)
            for p, g in zip(ps, gs):
                p.grad = g * c
            o.step()
        return ([p.detach() for p in ps], [o.state[p]["exp_avg"] for p in ps],
                [o.state[p]["exp_avg_sq"] for p in ps])

    f32, twin = adam(torch.float32), adam(torch.float64)
    got = _views(ops, opt)
    for n, a, b in zip(NUMELS, got[0], f32[0]):
        print(f"adam param[{n}]: max abs diff {float((a - b).abs().max()):.3g}")
        torch.testing.assert_close(a, b, rtol=0, atol=0.01 * min(LRS))
    for name, gl, tl in zip(("exp_avg", "exp_avg_sq"), got[1:], twin[1:]):
        for n, a, c in zip(NUMELS, gl, tl):
            e = U.rel_err(a, c)
            print(f"adam {name}[{n}]: {e:.3g}")
            assert e <= 2e-5, (name, n, e)
    _padding_is_zero(ops, opt)
