"""ops.vit_attn (csrc/ocppo_vit_attn.hip, f32 MFMA) on the GPU: forward and dqkv against the
float64 twin tu.mha_ref(mask=None) under the project's error rule (at most max(3 x torch's own f32
error, 4 * 2^-23) of the twin's largest element), padded keys at weight exactly 0, bitwise
repeatability eager and as a replayed hipGraph, and the contract's error statuses. Run with -s
for the (measured / torch's own) pairs."""
import pytest
import torch

import transformer_util as tu

pytestmark = pytest.mark.gpu


def _case(dev, B, S, heads, dh, seed, qk_scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    I = heads * dh
    qkv = torch.randn(B, S, 3 * I, generator=gen)
    qkv[..., :2 * I] *= qk_scale
    return qkv.to(dev), torch.randn(B, S, I, generator=gen).to(dev)


def _ref(qkv, dout, heads, dtype):
    q = qkv.detach().to(dtype).clone().requires_grad_(True)
    out = tu.mha_ref(q, None, heads)
    out.backward(dout.to(dtype))
    return out.detach(), q.grad


def _lse_ref(qkv, heads, dtype):
    B, S, I3 = qkv.shape
    dh = I3 // 3 // heads
    q, k = (t.to(dtype).reshape(B, S, heads, dh).transpose(1, 2)
            for t in qkv.split(I3 // 3, dim=2)[:2])
    return torch.logsumexp(q @ k.transpose(-1, -2) / dh ** 0.5, dim=-1)


def _run(qkv, dout, heads):
    from oc_cleanrl_amd import ops

    q = qkv.clone().requires_grad_(True)
    out = ops.vit_attn(q, heads)
    out.backward(dout)
    return out.detach(), q.grad


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("heads,dh", [(1, 32), (3, 32), (8, 64)])
@pytest.mark.parametrize("S", [1, 16, 17, 49, 64])
def test_vit_attn_matches_f64_twin(dev, S, heads, dh, B):
    qkv, dout = _case(dev, B, S, heads, dh, seed=S * 131 + B)
    out, dqkv = _run(qkv, dout, heads)
    o32, g32 = _ref(qkv, dout, heads, torch.float32)
    o64, g64 = _ref(qkv, dout, heads, torch.float64)
    tu.check("out", out, o32, o64)
    tu.check("dqkv", dqkv, g32, g64)


@pytest.mark.parametrize("S", [17, 49])
def test_padded_keys_carry_weight_exactly_zero(dev, S):
    """Every real score is below -30 (q and k share a large common direction with opposite signs):
    a zero-filled pad row scoring 0 would take the whole softmax."""
    from oc_cleanrl_amd import ops

    heads, dh = 8, 64
    I = heads * dh
    qkv, dout = _case(dev, 2, S, heads, dh, seed=S, qk_scale=0.1)
    qkv[..., :I] += 4.0     # q . k = sum over dh of about 4 * -4: scaled score about -128
    qkv[..., I:2 * I] -= 4.0
    assert float(_lse_ref(qkv, heads, torch.float64).max()) < -30
    out, dqkv = _run(qkv, dout, heads)
    _, lse = ops.vit_attn_fwd(qkv, heads)
    o32, g32 = _ref(qkv, dout, heads, torch.float32)
    o64, g64 = _ref(qkv, dout, heads, torch.float64)
    tu.check("out", out, o32, o64)
    tu.check("lse", lse, _lse_ref(qkv, heads, torch.float32), _lse_ref(qkv, heads, torch.float64))
    tu.check("dqkv", dqkv, g32, g64)


def test_repeatable_eager_and_graph(dev):
    from oc_cleanrl_amd import ops

    heads = 8
    qkv, dout = _case(dev, 3, 49, heads, 64, seed=5)
    out, lse = ops.vit_attn_fwd(qkv, heads)
    dqkv = ops.vit_attn_bwd(qkv, out, lse, dout, heads)
    out2, lse2 = ops.vit_attn_fwd(qkv, heads)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    assert torch.equal(dqkv, ops.vit_attn_bwd(qkv, out, lse, dout, heads))
    go, gl, gd = torch.empty_like(out), torch.empty_like(lse), torch.empty_like(dqkv)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.vit_attn_fwd(qkv, heads, go, gl)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.vit_attn_fwd(qkv, heads, go, gl)
        ops.vit_attn_bwd(qkv, go, gl, dout, heads, gd)
    for _ in range(3):
        go.zero_(), gl.zero_(), gd.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(go, out) and torch.equal(gl, lse) and torch.equal(gd, dqkv)


@pytest.mark.parametrize("B,S,I,heads", [(2, 65, 512, 8), (2, 16, 64, 4), (2, 16, 576, 9),
                                         (0, 16, 512, 8)])
def test_contract_violations_return_invalid(dev, B, S, I, heads):
    """S = 65, dh = 16, I = 576, B = 0: OCPPO_E_INVALID, and the outputs stay untouched."""
    from oc_cleanrl_amd import _lib

    n = max(B, 1) * S
    qkv = torch.zeros(n * 3 * I, device=dev)
    out, lse, dq = torch.full((n * I,), 7.0, device=dev), torch.full((n * heads,), 7.0, device=dev), \
        torch.full((n * 3 * I,), 7.0, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    assert _lib.LIB.ocppo_vit_attn_fwd(st, qkv.data_ptr(), B, S, I, heads, out.data_ptr(),
                                       lse.data_ptr()) == _lib.OCPPO_E_INVALID
    assert _lib.LIB.ocppo_vit_attn_bwd(st, qkv.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                       out.data_ptr(), B, S, I, heads,
                                       dq.data_ptr()) == _lib.OCPPO_E_INVALID
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((lse == 7).all()) and bool((dq == 7).all())
