"""ops.mha and ops.add_layernorm (csrc/ocppo_attn.hip), forward and backward, on the GPU: against
the float64 twin of tests/transformer_util.py under the project's error rule (at most
max(3 x torch's own f32 error, 4 * 2^-23) of the twin's largest element), exact zeros for excluded
keys, bitwise repeatability eager and as a replayed hipGraph, and the contract's error statuses.
Run with -s for the (measured / torch's own) pairs."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import transformer_util as tu

pytestmark = pytest.mark.gpu

HEADS = [(8, 16), (1, 64), (4, 8), (16, 32)]
MASKS = ("none", "tail", "hole", "one")


def _mha_case(dev, B, S, heads, dh, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    E = heads * dh
    qkv = torch.randn(B, S, 3 * E, generator=gen)
    dout = torch.randn(B, S, E, generator=gen)
    mask = tu.make_masks(kind, B, S, gen)
    return qkv.to(dev), dout.to(dev), None if mask is None else mask.to(dev)


def _ref(qkv, dout, mask, heads, dtype):
    q = qkv.detach().to(dtype).clone().requires_grad_(True)
    out = tu.mha_ref(q, mask, heads)
    out.backward(dout.to(dtype))
    return out.detach(), q.grad


@pytest.mark.parametrize("S", [1, 5, 16, 17, 64])
@pytest.mark.parametrize("heads,dh", HEADS)
def test_mha_matches_f64_twin(dev, S, heads, dh):
    from oc_cleanrl_amd import ops

    worst = (0.0, 0.0)
    for B in (1, 3, 67):
        for kind in MASKS:
            qkv, dout, mask = _mha_case(dev, B, S, heads, dh, kind, seed=S * 131 + B)
            kv = None if mask is None else mask.to(torch.uint8)
            q = qkv.clone().requires_grad_(True)
            out = ops.mha(q, kv, heads)
            out.backward(dout)
            o32, g32 = _ref(qkv, dout, mask, heads, torch.float32)
            o64, g64 = _ref(qkv, dout, mask, heads, torch.float64)
            tag = f"mha B{B} S{S} h{heads} dh{dh} {kind}"
            for name, got, f32, twin in (("out", out.detach(), o32, o64),
                                         ("dqkv", q.grad, g32, g64)):
                e, own = tu.rel_err(got, twin), tu.rel_err(f32, twin)
                worst = max(worst, (e, own))
                assert e <= tu.bound(own), (tag, name, e, own)
            if mask is not None:  # excluded keys: dK and dV exactly 0
                E = heads * dh
                dk, dv = q.grad[..., E:2 * E], q.grad[..., 2 * E:]
                assert not dk[~mask].any() and not dv[~mask].any(), tag
    print(f"mha S{S} h{heads} dh{dh}: worst {worst[0]:.3g} / {worst[1]:.3g}")


def test_mha_matches_torch_multihead_attention(dev):
    """Through torch's own module: in-proj -> ops.mha -> out-proj against
    nn.MultiheadAttention(key_padding_mask=...) in f32, the module in f64 as the twin."""
    from oc_cleanrl_amd import ops

    torch.manual_seed(5)
    B, S, E, heads = 7, 11, 128, 8
    mha = torch.nn.MultiheadAttention(E, heads, batch_first=True).to(dev)
    x = torch.randn(B, S, E, device=dev)
    mask = tu.make_masks("tail", B, S, torch.Generator().manual_seed(1)).to(dev)
    qkv = F.linear(x, mha.in_proj_weight, mha.in_proj_bias)
    got = F.linear(ops.mha(qkv, mask.to(torch.uint8), heads), mha.out_proj.weight,
                   mha.out_proj.bias)
    f32 = mha(x, x, x, key_padding_mask=~mask, need_weights=False)[0]
    m64 = torch.nn.MultiheadAttention(E, heads, batch_first=True).to(dev).double()
    m64.load_state_dict({k: v.double() for k, v in mha.state_dict().items()})
    xd = x.double()
    twin = m64(xd, xd, xd, key_padding_mask=~mask, need_weights=False)[0]
    tu.check("mha vs nn.MultiheadAttention", got.detach(), f32.detach(), twin.detach())


def test_mha_excluded_keys_have_weight_exactly_zero(dev):
    from oc_cleanrl_amd import ops

    B, S, heads, dh = 3, 17, 8, 16
    E = heads * dh
    qkv, _, mask = _mha_case(dev, B, S, heads, dh, "tail", seed=3)
    mask[0, 5:] = False
    kv = mask.to(torch.uint8)
    out, lse = ops.mha_fwd(qkv, kv, heads)
    pert = qkv.clone()
    rows = ~mask
    pert[..., E:][rows] = pert[..., E:][rows] * -37.0 + 1e4  # K and V rows of excluded keys
    out2, lse2 = ops.mha_fwd(pert, kv, heads)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)


def test_mha_bitwise_repeatable_eager_and_graph(dev):
    from oc_cleanrl_amd import ops

    B, S, heads, dh = 67, 17, 8, 16
    qkv, dout, mask = _mha_case(dev, B, S, heads, dh, "tail", seed=9)
    kv = mask.to(torch.uint8)

    def run():
        out, lse = ops.mha_fwd(qkv, kv, heads)
        return out, lse, ops.mha_bwd(qkv, kv, out, lse, dout, heads)

    a, b = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = run()
    for _ in range(2):
        for t in c:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(a, c))


def test_mha_contract_violations_return_an_error_status(dev):
    from oc_cleanrl_amd import _lib, ops

    L = _lib.LIB
    d = ctypes.c_void_p(256)
    bad = [(2, 65, 128, 8), (2, 0, 128, 8), (2, 6, 32, 8), (2, 6, 1024, 8), (2, 6, 130, 8),
           (0, 6, 128, 8), (2, 6, 128, 0)]
    for B, S, E, heads in bad:
        assert L.ocppo_mha_fwd(None, d, None, B, S, E, heads, d, d) == _lib.OCPPO_E_INVALID
        assert L.ocppo_mha_bwd(None, d, None, d, d, d, B, S, E, heads, d) == _lib.OCPPO_E_INVALID
    assert L.ocppo_mha_fwd(None, None, None, 2, 6, 128, 8, d, d) == _lib.OCPPO_E_INVALID
    assert b"null pointer" in L.ocppo_last_error()
    assert L.ocppo_add_layernorm_fwd(None, d, d, d, d, 4, 513, 1e-5, d, d, d) == \
        _lib.OCPPO_E_INVALID
    assert L.ocppo_add_layernorm_bwd(None, d, d, d, d, d, d, 4, 128, d, d, d, d, 16) == \
        _lib.OCPPO_E_WORKSPACE
    with pytest.raises(ValueError, match="mha_shape_ok"):
        ops.mha_fwd(torch.zeros(2, 65, 3 * 128, device=dev), None, 8)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.mha_fwd(torch.zeros(2, 6, 3 * 128), None, 8)


# ---- residual add + LayerNorm -------------------------------------------------------------------
def _ln_ref(x, res, w, b, dy, eps, dtype, torch_own=False):
    x, res, w, b = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, res, w, b))
    if torch_own:
        y = F.layer_norm(x + res, (x.shape[-1],), w, b, eps)
    else:
        y = tu.add_layernorm_ref(x, res, w, b, eps)
    y.backward(dy.to(dtype))
    return y.detach(), x.grad, res.grad, w.grad, b.grad


def _ln_check(dev, R, E, seed, offset=0.0, constant=False, eps=1e-5):
    from oc_cleanrl_amd import ops

    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(R, E, generator=gen)
    res = torch.randn(R, E, generator=gen) + offset
    if constant:  # row 0 of x + res constant: variance 0, rstd = 1 / sqrt(eps)
        x[0] = 0.75
        res[0] = -0.25
    w, b = torch.randn(E, generator=gen), torch.randn(E, generator=gen)
    dy = torch.randn(R, E, generator=gen)
    x, res, w, b, dy = (t.to(dev) for t in (x, res, w, b, dy))
    xs, rs, ws, bs = (t.clone().requires_grad_(True) for t in (x, res, w, b))
    y = ops.add_layernorm(xs, rs, ws, bs, eps)
    y.backward(dy)
    got = (y.detach(), xs.grad, rs.grad, ws.grad, bs.grad)
    assert torch.equal(xs.grad, rs.grad)
    f32 = _ln_ref(x, res, w, b, dy, eps, torch.float32, torch_own=True)
    twin = _ln_ref(x, res, w, b, dy, eps, torch.float64)
    tag = f"add_layernorm R{R} E{E} offset {offset:g}" + (" const" if constant else "")
    for name, g, f, t in zip(("y", "dx", "dres", "dgamma", "dbeta"), got, f32, twin):
        tu.check(f"{tag} {name}", g, f, t)
    return x, res, w, b, dy, got


@pytest.mark.parametrize("E", [32, 128, 512])
@pytest.mark.parametrize("R", [1, 5, 1027])
def test_add_layernorm_matches_f64_twin(dev, R, E):
    _ln_check(dev, R, E, seed=R + E)


def test_add_layernorm_constant_row(dev):
    from oc_cleanrl_amd import ops

    eps = 1e-5
    x, res, w, b, _, got = _ln_check(dev, 5, 128, seed=2, constant=True, eps=eps)
    _, mean, rstd = ops.add_layernorm_fwd(x, res, w, b, eps)
    assert float(mean[0]) == 0.5
    assert abs(float(rstd[0]) - eps ** -0.5) <= 2e-7 * eps ** -0.5
    assert torch.equal(got[0][0], b)  # (0 * rstd) * gamma + beta


@pytest.mark.parametrize("E", [32, 512])
def test_add_layernorm_large_common_offset(dev, E):
    """Rows of about 1e3 plus unit noise: E[x^2] - mean^2 in f32 loses the variance there; the
    variance about the mean does not."""
    _ln_check(dev, 67, E, seed=4, offset=1e3)


def test_add_layernorm_bitwise_repeatable(dev):
    from oc_cleanrl_amd import ops

    gen = torch.Generator().manual_seed(8)
    R, E = 1027, 128
    x, res, dy = (torch.randn(R, E, generator=gen).to(dev) for _ in range(3))
    w, b = torch.randn(E, generator=gen).to(dev), torch.randn(E, generator=gen).to(dev)

    def run():
        y, mean, rstd = ops.add_layernorm_fwd(x, res, w, b, 1e-5)
        return (y, mean, rstd) + ops.add_layernorm_bwd(dy, x, res, w, mean, rstd)

    a, c = run(), run()
    assert all(torch.equal(p, q) for p, q in zip(a, c))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d = run()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(a, d))
