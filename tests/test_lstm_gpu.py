"""The LSTM kernels (csrc/ocppo_lstm.hip) on the GPU: ops.lstm_seq forward and every gradient, and
T calls of ops.lstm_step, against the float64 twin (tests/lstm_util.py) under the error rule of
DESIGN.md 11; the bitwise properties that follow from the fixed per-environment order; the fused
agent against the reference's fixture.

A workgroup of the sequence kernels takes ONE environment, so B = 2 is "just past" it; the step
kernel takes 4, so B = 7 spans two workgroups with a ragged tail and B = 5 is just past one.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest
import torch

import lstm_util as U
from conftest import golden

pytestmark = pytest.mark.gpu

DONE_KINDS = ("zero", "one", "first", "last", "random")


def done_pattern(kind, T, B, rng):
    d = np.zeros((T, B), np.float32)
    if kind == "one":
        d[:] = 1
    elif kind == "first":
        d[0] = 1
    elif kind == "last":
        d[T - 1] = 1
    elif kind == "random":
        d[rng.random((T, B)) < 0.25] = 1
    return d


def make_case(T, B, I, H, kind, zero_state, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))  # noqa: E731
    k = 1.0 / np.sqrt(H)
    return dict(T=T, B=B, I=I, H=H, x=f(T, B, I), w_ih=f(4 * H, I) * k, b_ih=f(4 * H) * k,
                w_hh=f(4 * H, H) * k, b_hh=f(4 * H) * k,
                done=torch.from_numpy(done_pattern(kind, T, B, rng)),
                h0=torch.zeros(B, H) if zero_state else f(B, H) * 0.5,
                c0=torch.zeros(B, H) if zero_state else f(B, H) * 0.5, g=f(T, B, H))


def refs(c):
    a = {k: c[k] for k in ("T", "B", "I", "H", "done", "h0", "c0", "x", "w_ih", "b_ih", "w_hh",
                            "b_hh", "g")}
    return U.seq_case(**a, dtype=torch.float32), U.seq_case(**a, dtype=torch.float64)


def run_fused(c, dev):
    """ops.lstm_seq on pre = linear_act(x): outputs and every gradient."""
    from oc_cleanrl_amd import ops
    from oc_cleanrl_amd.agents import linear_act

    T, B, I, H = c["T"], c["B"], c["I"], c["H"]
    p = {k: c[k].to(dev).requires_grad_() for k in ("x", "w_ih", "b_ih", "w_hh", "b_hh")}
    pre = linear_act(p["x"].view(T * B, I), SimpleNamespace(weight=p["w_ih"], bias=p["b_ih"]),
                     False).view(T, B, 4 * H)
    pre.retain_grad()
    h_out, (hT, cT) = ops.lstm_seq(pre, p["w_hh"], p["b_hh"], c["done"].to(dev), c["h0"].to(dev),
                                   c["c0"].to(dev))
    (h_out * c["g"].to(dev)).sum().backward()
    return dict(h_out=h_out.detach(), hT=hT, cT=cT, dpre=pre.grad, dx=p["x"].grad,
                dw_ih=p["w_ih"].grad, db_ih=p["b_ih"].grad, dw_hh=p["w_hh"].grad,
                db_hh=p["b_hh"].grad)


CASES = [  # (T, B, I, H, done, zero initial state)
    (1, 1, 5, 32, "zero", True), (1, 3, 64, 128, "one", False), (2, 2, 5, 128, "first", False),
    (2, 7, 64, 32, "last", True), (3, 3, 5, 32, "random", False), (3, 1, 64, 128, "zero", False),
    (17, 7, 5, 128, "random", False), (17, 3, 64, 32, "one", False), (17, 2, 64, 64, "random", True),
    (3, 5, 5, 128, "last", False), (17, 1, 5, 32, "first", True),
]


@pytest.mark.parametrize("T,B,I,H,kind,zero", CASES)
def test_lstm_seq_forward_and_gradients_match_the_twin(dev, T, B, I, H, kind, zero):
    c = make_case(T, B, I, H, kind, zero, seed=1000 + 31 * T + 7 * B + I + H)
    r32, r64 = refs(c)
    got = run_fused(c, dev)
    for k in ("h_out", "hT", "cT", "dpre", "dw_hh", "db_hh", "dw_ih", "db_ih", "dx"):
        U.check(f"{k} T={T} B={B} I={I} H={H} {kind}", got[k], r32[k], r64[k])


@pytest.mark.parametrize("T,B,I,H,kind,zero", CASES)
def test_lstm_step_matches_seq_and_the_twin(dev, T, B, I, H, kind, zero):
    from oc_cleanrl_amd import ops

    c = make_case(T, B, I, H, kind, zero, seed=2000 + 31 * T + 7 * B + I + H)
    r32, r64 = refs(c)
    d = {k: c[k].to(dev) for k in ("x", "w_ih", "b_ih", "w_hh", "b_hh", "done", "h0", "c0")}
    h, cc = d["h0"].clone(), d["c0"].clone()
    outs = []
    for t in range(T):
        ops.lstm_step(d["x"][t], d["w_ih"], d["b_ih"], d["w_hh"], d["b_hh"], d["done"][t], h, cc)
        outs.append(h.clone())
    outs = torch.stack(outs)
    U.check("step h_out", outs, r32["h_out"], r64["h_out"])
    U.check("step cT", cc, r32["cT"], r64["cT"])
    U.check("step hT", h, r32["hT"], r64["hT"])
    with torch.no_grad():
        pre = (d["x"].view(T * B, I) @ d["w_ih"].t() + d["b_ih"]).view(T, B, 4 * H)
        seq, hT, cT, _ = ops.lstm_seq_fwd(pre, d["w_hh"], d["b_hh"], d["done"], d["h0"], d["c0"],
                                          save=False)
    # against the sequence kernel, under the same rule (the torch loop's own error of that tensor)
    for name, got, ref in (("h_out", outs, seq), ("hT", h, hT), ("cT", cc, cT)):
        e, own = U.rel_err(got, ref), U.rel_err(r32[name], r64[name])
        print(f"step vs seq {name}: {e:.3g} / {own:.3g}")
        assert e <= U.bound(own), (name, e, own)


def _seq(c, dev, rows=None, steps=None):
    """(h_out, hT, cT, saved, dgates) of the sequence kernels on the environments `rows` and the
    time steps `steps` of the case. The input projection is made ONCE for the whole case and
    sliced, so that a sub-batch sees the same bits (a GEMM of another shape may sum otherwise)."""
    from oc_cleanrl_amd import ops

    T, B, I, H = c["T"], c["B"], c["I"], c["H"]
    sel = slice(None) if rows is None else rows
    ts = slice(None) if steps is None else steps
    d = {k: c[k].to(dev) for k in ("w_ih", "b_ih", "w_hh", "b_hh")}
    pre = (c["x"].to(dev).view(T * B, I) @ d["w_ih"].t() + d["b_ih"]).view(T, B, 4 * H)
    pre = pre[ts][:, sel].contiguous()
    done = c["done"][ts][:, sel].contiguous().to(dev)
    h0, c0 = c["h0"][sel].contiguous().to(dev), c["c0"][sel].contiguous().to(dev)
    h_out, hT, cT, saved = ops.lstm_seq_fwd(pre, d["w_hh"], d["b_hh"], done, h0, c0)
    c_out, gates, h_in = saved
    dg = ops.lstm_seq_bwd(c["g"][ts][:, sel].contiguous().to(dev), gates, c_out, c0, done,
                          d["w_hh"])
    return h_out, hT, cT, saved, dg


@pytest.mark.parametrize("H", [32, 128])
def test_an_environment_is_bitwise_the_same_alone_and_in_a_batch(dev, H):
    c = make_case(17, 7, 5, H, "random", False, seed=31 + H)
    full = _seq(c, dev)
    for b in (0, 3, 6):
        one = _seq(c, dev, rows=slice(b, b + 1))
        assert torch.equal(one[0][:, 0], full[0][:, b])
        assert torch.equal(one[1][0], full[1][b]) and torch.equal(one[2][0], full[2][b])
        assert torch.equal(one[4][:, 0], full[4][:, b])


@pytest.mark.parametrize("H", [32, 128])
def test_a_done_restarts_the_sequence_bitwise(dev, H):
    T, k = 9, 4
    c = make_case(T, 3, 64, H, "zero", False, seed=47 + H)
    c["done"][k] = 1.0
    full = _seq(c, dev)
    tail = dict(c, done=c["done"].clone(), h0=torch.zeros_like(c["h0"]),
                c0=torch.zeros_like(c["c0"]))
    tail["done"][k] = 0.0
    fresh = _seq(tail, dev, steps=slice(k, T))
    assert torch.equal(full[0][k:], fresh[0])
    assert torch.equal(full[1], fresh[1]) and torch.equal(full[2], fresh[2])
    assert torch.equal(full[4][k:], fresh[4])  # and no gradient crosses the reset
    # the steps before the reset get nothing from after it: dgates of steps < k depend on g[:k]
    c2 = dict(c, g=torch.cat([c["g"][:k], c["g"][k:] * 3.0]))
    assert torch.equal(_seq(c2, dev)[4][:k], full[4][:k])


def test_two_runs_are_bitwise_identical(dev):
    c = make_case(17, 7, 64, 128, "random", False, seed=5)
    a, b = _seq(c, dev), _seq(c, dev)
    for x, y in zip((a[0], a[1], a[2], *a[3], a[4]), (b[0], b[1], b[2], *b[3], b[4])):
        assert torch.equal(x, y)
    from oc_cleanrl_amd import ops

    d = {k: c[k].to(dev) for k in ("x", "w_ih", "b_ih", "w_hh", "b_hh", "done", "h0", "c0")}
    res = []
    for _ in range(2):
        h, cc = d["h0"].clone(), d["c0"].clone()
        ops.lstm_step(d["x"][0], d["w_ih"], d["b_ih"], d["w_hh"], d["b_hh"], d["done"][0], h, cc)
        res.append((h, cc))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


@pytest.mark.parametrize("H,B", [(32, 3), (128, 5)])
def test_rows_past_the_batch_keep_their_sentinel(dev, H, B):
    """The C entry points on over-allocated buffers of the test's own: every element past the
    tensor keeps the sentinel, every element of the tensor is written."""
    from oc_cleanrl_amd import ops
    from oc_cleanrl_amd._lib import call

    T, I = 3, 5
    c = make_case(T, B, I, H, "random", False, seed=77 + H)
    d = {k: c[k].to(dev).contiguous() for k in ("x", "w_ih", "b_ih", "w_hh", "b_hh", "done", "h0",
                                                "c0", "g")}
    pre = (d["x"].view(T * B, I) @ d["w_ih"].t() + d["b_ih"]).contiguous()
    S, extra = 12345.0, 2 * 4 * H
    sizes = dict(h_out=T * B * H, hT=B * H, cT=B * H, c_out=T * B * H, gates=T * B * 4 * H,
                 h_in=T * B * H, dgates=T * B * 4 * H)
    out = {k: torch.full((n + extra,), S, device=dev) for k, n in sizes.items()}
    stream = torch.cuda.current_stream(dev).cuda_stream
    ptr = lambda k: out[k].data_ptr()  # noqa: E731
    call("ocppo_lstm_seq_fwd", stream, pre.data_ptr(), d["w_hh"].data_ptr(), d["b_hh"].data_ptr(),
         d["done"].data_ptr(), d["h0"].data_ptr(), d["c0"].data_ptr(), T, B, H, ptr("h_out"),
         ptr("c_out"), ptr("gates"), ptr("h_in"), ptr("hT"), ptr("cT"))
    call("ocppo_lstm_seq_bwd", stream, d["g"].data_ptr(), ptr("gates"), ptr("c_out"),
         d["c0"].data_ptr(), d["done"].data_ptr(), d["w_hh"].data_ptr(), T, B, H, ptr("dgates"))
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert bool((out[k][n:] == S).all()), k
        assert not bool((out[k][:n] == S).any()), k
    ref = ops.lstm_seq_fwd(pre.view(T, B, 4 * H), d["w_hh"], d["b_hh"], d["done"], d["h0"],
                           d["c0"])
    assert torch.equal(out["h_out"][:T * B * H].view(T, B, H), ref[0])
    # the step kernel: a state buffer longer than N rows
    N = B
    hbuf, cbuf = torch.full((N + 3, H), S, device=dev), torch.full((N + 3, H), S, device=dev)
    hbuf[:N], cbuf[:N] = d["h0"], d["c0"]
    ops.lstm_step(d["x"][0], d["w_ih"], d["b_ih"], d["w_hh"], d["b_hh"], d["done"][0], hbuf[:N],
                  cbuf[:N])
    assert bool((hbuf[N:] == S).all()) and bool((cbuf[N:] == S).all())


@pytest.fixture(scope="module")
def ref_agent(dev):
    """The reference's network from the fixture's seed, its inputs, and its trunk output on the
    GPU (computed once, shared)."""
    from oc_cleanrl_amd import lstm
    from oc_cleanrl_amd.agents import EnvSpec

    fx = golden("lstm_ref_t4b3_mixed.npz")
    torch.manual_seed(int(fx["seed"]))
    cpu = lstm.LSTMAgent(EnvSpec((1, 84, 84), int(fx["n_actions"])), "PPO")
    torch.manual_seed(int(fx["seed"]))
    agent = lstm.LSTMAgent(EnvSpec((1, 84, 84), int(fx["n_actions"])), "PPO").to(dev)
    x = torch.from_numpy(fx["x"].astype(np.float32))
    hid = agent.trunk(x.to(dev)).detach()
    return fx, cpu, agent, x, hid


def _after_trunk(p, hid, fx, dtype):
    """Recurrence + heads + the fixture's loss on the trunk output `hid`, plain torch on the CPU in
    `dtype`: outputs, and the gradients at `hid` and at every parameter after the trunk."""
    t = lambda a: torch.as_tensor(a).detach().cpu().to(dtype)  # noqa: E731
    keys = [k for k in p if not k.startswith("network.")]
    q = {k: t(p[k]).requires_grad_() for k in keys}
    xh = t(hid).requires_grad_()
    T, B = int(fx["T"]), int(fx["B"])
    out, hT, cT = U.lstm_seq_ref(xh.view(T, B, -1), q["lstm.weight_ih_l0"], q["lstm.bias_ih_l0"],
                                 q["lstm.weight_hh_l0"], q["lstm.bias_hh_l0"],
                                 t(fx["done"]).view(T, B), t(fx["h0"])[0], t(fx["c0"])[0])
    hidden = out.reshape(T * B, -1)
    logits = hidden @ q["actor.weight"].t() + q["actor.bias"]
    value = hidden @ q["critic.weight"].t() + q["critic.bias"]
    loss = (logits * t(fx["wl"])).sum() + (value * t(fx["wv"])).sum()
    loss.backward()
    res = dict(hidden=hidden, hT=hT.unsqueeze(0), cT=cT.unsqueeze(0), logits=logits, value=value,
               loss=loss, **{"g:hid": xh.grad}, **{"g:" + k: q[k].grad for k in keys})
    return {k: v.detach() for k, v in res.items()}


def test_fused_agent_after_the_trunk_matches_the_twin(dev, ref_agent):
    """The reference's network on the fixture's inputs, everything after the trunk: the fused
    recurrence, the heads, the fixture's loss and every gradient (the LSTM's and the heads'
    parameters, and what flows into the trunk) against the float64 twin ON THE SAME TRUNK OUTPUT,
    with the plain-torch f32 loop on that output as the rule's "own". The trunk's own error is
    kept out of this bound (test_reference_trunk_matches_the_twin has it): on noise images it
    differs between machines and the recurrence amplifies it (the f64 recurrence on the GPU
    trunk's output is 2.0e-6 from the fixture's twin in `hidden`, the fixture's own f32 run
    0.46e-6, while the fused kernel is within 6.5e-8 of the f64 chain on its own input). The twin
    itself is tied to the reference's f64 run by tests/test_lstm_cpu.py."""
    from oc_cleanrl_amd import lstm

    fx, _, agent, _, hid = ref_agent
    p = {k: v.detach() for k, v in agent.state_dict().items()}
    own, twin = _after_trunk(p, hid, fx, torch.float32), _after_trunk(p, hid, fx, torch.float64)
    state = (torch.from_numpy(fx["h0"]).to(dev), torch.from_numpy(fx["c0"]).to(dev))
    done = torch.from_numpy(fx["done"]).to(dev)
    xh = hid.clone().requires_grad_()
    assert lstm.FUSED_LSTM and lstm.lstm_ok(xh, done, state, 128)
    agent.zero_grad()
    hidden, (hT, cT) = agent.recur(xh, state, done)
    logits, value = agent.heads(hidden)
    loss = (logits * torch.from_numpy(fx["wl"]).to(dev)).sum() + \
        (value * torch.from_numpy(fx["wv"]).to(dev)).sum()
    loss.backward()
    got = dict(hidden=hidden, hT=hT, cT=cT, logits=logits, value=value, loss=loss,
               **{"g:hid": xh.grad},
               **{"g:" + k: q.grad for k, q in agent.named_parameters()
                  if not k.startswith("network.")})
    assert set(got) == set(twin)
    for k in twin:
        U.check(k, got[k].detach(), own[k], twin[k])


def test_reference_trunk_matches_the_twin(dev, ref_agent):
    """The reference's 1-frame NatureCNN + Linear on the package's routes, with autograd and under
    no_grad (the rollout: a 1-channel first convolution is not the HIP rollout kernel's shape and
    takes the library's), forward and every trunk parameter gradient for a fixed upstream
    gradient: against the float64 twin under the rule of DESIGN.md 11, "own" being the plain torch
    modules `network(x / 255)` in f32 on the CPU."""
    fx, cpu, agent, x, hid = ref_agent
    g = torch.from_numpy(np.random.default_rng(9).standard_normal((12, 512)).astype(np.float32))
    p64 = {k: v.detach().double().requires_grad_() for k, v in cpu.state_dict().items()
           if k.startswith("network.")}
    t64 = U.trunk(p64, x.double(), True)
    (t64 * g.double()).sum().backward()
    cpu.zero_grad()
    t32 = cpu.network(x / 255.0)
    (t32 * g).sum().backward()
    U.check("trunk", hid, t32.detach(), t64.detach())
    with torch.no_grad():
        U.check("trunk (no_grad)", agent.trunk(x.to(dev)), t32.detach(), t64.detach())
    agent.zero_grad()
    (agent.trunk(x.to(dev)) * g.to(dev)).sum().backward()
    grads = dict(agent.named_parameters())
    for k, q in cpu.named_parameters():
        if k.startswith("network."):
            U.check("g:" + k, grads[k].grad, q.grad, p64[k].grad)
