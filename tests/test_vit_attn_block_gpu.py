"""ops.vit_attn_block (csrc/ocppo_vit_attn_block.hip, f32 MFMA): y = x + to_out(attention(to_qkv(LN(x))))
and its five gradients against the float64 torch chain under the project's error rule
(transformer_util.check: at most max(3 x torch's own f32 error, 4 * 2^-23) of the twin's largest
element), constant and zero rows, a saturated softmax, bitwise repeatability eager and as a replayed
hipGraph, the contract's statuses and the agent's route. Run with -s for the (measured / torch's own)
pairs."""
import copy

import pytest
import torch
import torch.nn.functional as F

import transformer_util as tu

pytestmark = pytest.mark.gpu

NAMES = ("y", "dx", "dgamma", "dbeta", "dWqkv", "dWout")


def _case(dev, B, S, D, heads, seed):
    """[x, gamma, beta, Wqkv, Wout, dy] on dev."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    I = 64 * heads
    c = [r(B * S, D) * 2 + 0.5, 1 + 0.1 * r(D), 0.1 * r(D), r(3 * I, D) / D ** 0.5,
         r(D, I) / I ** 0.5, r(B * S, D)]
    return [t.to(dev) for t in c]


def _twin(c, S, dtype):
    x, g, b, Wqkv, Wout = (t.detach().to(dtype).clone().requires_grad_(True) for t in c[:5])
    B, heads = x.shape[0] // S, Wqkv.shape[0] // 192
    qkv = F.linear(F.layer_norm(x, x.shape[1:], g, b), Wqkv).view(B, S, -1)
    q, k, v = (t.reshape(B, S, heads, -1).transpose(1, 2) for t in qkv.chunk(3, dim=-1))
    o = torch.softmax(q @ k.transpose(-1, -2) * 64 ** -0.5, dim=-1) @ v
    y = x + F.linear(o.transpose(1, 2).reshape(B * S, -1), Wout)
    y.backward(c[5].to(dtype))
    return [y.detach(), x.grad, g.grad, b.grad, Wqkv.grad, Wout.grad]


def _run(c, S, out=None):
    from oc_cleanrl_amd import ops

    x, g, b, Wqkv, Wout, dy = c
    y, mean, rstd, lse = ops.vit_attn_block_fwd(x, g, b, Wqkv, Wout, S, 1e-5, True,
                                                *(out or [None] * 4)[:4])
    return [y, *ops.vit_attn_block_bwd(dy, x, mean, rstd, lse, g, b, Wqkv, Wout, S,
                                       out and tuple(out[4:]))]


def _check_all(c, S):
    got, f32, f64 = _run(c, S), _twin(c, S, torch.float32), _twin(c, S, torch.float64)
    for n, a, o, t in zip(NAMES, got, f32, f64):
        tu.check(n, a, o, t)
    return got


@pytest.mark.parametrize("D,heads", [(32, 1), (32, 2), (64, 3), (96, 2), (128, 8)])
@pytest.mark.parametrize("B,S", [(1, 1), (1, 16), (2, 17), (3, 49), (2, 64)])
def test_vit_attn_block_matches_f64_twin(dev, B, S, D, heads):
    _check_all(_case(dev, B, S, D, heads, seed=B * 7 + S + D + heads), S)


def test_more_samples_than_backward_parts(dev):
    """B = cap + 1: workgroup 0 walks two samples and the finish adds the full partial count."""
    from oc_cleanrl_amd import ops

    B = ops.VIT_ATTN_BLOCK_PART_TARGET + 1
    assert ops.vit_attn_block_parts(B, 1) == B - 1
    _check_all(_case(dev, B, 3, 32, 1, seed=3), 3)


def test_constant_and_zero_rows_saturated_softmax(dev):
    c = _case(dev, 2, 49, 128, 8, seed=9)
    x, Wqkv = c[0], c[3]
    x[5], x[60] = 3.25, 0.0
    Wqkv[2 * 64:3 * 64] *= 30.0        # head 2's q rows
    Wqkv[512 + 2 * 64:512 + 3 * 64] *= 30.0  # and its k rows: scores in the thousands
    got = _check_all(c, 49)
    assert all(bool(torch.isfinite(t).all()) for t in got)


def test_repeatable_eager_and_graph(dev):
    c, S = _case(dev, 3, 49, 128, 8, seed=5), 49
    ref = _run(c, S)
    assert all(torch.equal(a, b) for a, b in zip(ref, _run(c, S)))
    stats = [torch.empty(147, device=dev), torch.empty(147, device=dev),
             torch.empty(3, 8, 49, device=dev)]
    out = [torch.empty_like(ref[0]), *stats, *(torch.empty_like(t) for t in ref[1:])]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(c, S, out)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _run(c, S, out)
    for _ in range(3):
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(ref, [out[0], *out[4:]]))


@pytest.mark.parametrize("B,S,D,heads", [(2, 49, 48, 8), (2, 65, 128, 8), (2, 49, 128, 9),
                                         (0, 49, 128, 8), (2, 49, 128, 8)])
def test_contract_statuses_leave_outputs_untouched(dev, B, S, D, heads):
    """D = 48, S = 65, heads = 9: OCPPO_E_INVALID and no workspace size; B = 0: nothing launched; a
    workspace one byte short: OCPPO_E_WORKSPACE. The sentinel-filled outputs stay as they were."""
    from oc_cleanrl_amd import _lib

    L, n, I = _lib.LIB, 2 * 65, 64 * 9
    z = torch.zeros(3 * I * 128, device=dev)
    outs = [torch.full((k,), 7.0, device=dev) for k in (n * 128, n, n, n * 9, 128, 128, 3 * I * 128,
                                                        128 * I)]
    y, mean, rstd, lse, dg, db, dWqkv, dWout = (t.data_ptr() for t in outs)
    st, p = torch.cuda.current_stream().cuda_stream, z.data_ptr()
    bad = (D, S, heads) != (128, 49, 8)
    want = _lib.OCPPO_E_INVALID if bad else _lib.OCPPO_OK
    if B == 0 or bad:
        assert L.ocppo_vit_attn_block_fwd(st, p, p, p, p, p, B, S, D, heads, 1e-5, y, mean, rstd,
                                          lse) == want
    nb = L.ocppo_vit_attn_block_workspace_bytes(B, S, D, heads)
    assert (nb == 0) == bad
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
    rc = L.ocppo_vit_attn_block_bwd(st, p, p, p, p, p, p, p, p, p, B, S, D, heads, y, dg, db, dWqkv,
                                    dWout, ws.data_ptr(), max(nb - 1, 0))
    assert rc == (want if B == 0 or bad else _lib.OCPPO_E_WORKSPACE)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs)


def test_vit_agent_routes_through_fused_attn(dev, monkeypatch):
    from oc_cleanrl_amd import ops, vit
    from oc_cleanrl_amd.agents import EnvSpec

    torch.manual_seed(21)
    gen = torch.Generator().manual_seed(22)
    agent = vit.ViTAgent(EnvSpec((4, 84, 84), 6), emb_dim=32, num_heads=2, num_blocks=2).to(dev)
    src = torch.randint(0, 256, (3, 4, 84, 84), generator=gen, dtype=torch.uint8).to(dev)
    dl, dv = torch.randn(3, 6, generator=gen).to(dev), torch.randn(3, 1, generator=gen).to(dev)
    taken = []
    real = ops.vit_attn_block
    monkeypatch.setattr(ops, "vit_attn_block", lambda x, a, S: taken.append(
        ops.vit_attn_block_ok(x, a, S)) or real(x, a, S))

    def grads(fused, stacks, dtype=torch.float32):
        monkeypatch.setattr(vit, "FUSED_ATTN", fused)
        ag = copy.deepcopy(agent).to(dtype)
        hidden = ag.trunk_stacks(src, None) if stacks else ag.trunk(src)
        logits, value = ag.actor(hidden), ag.critic(hidden)
        torch.autograd.backward([logits, value], [dl.to(dtype), dv.to(dtype)])
        return {"logits": logits.detach(), "value": value.detach(),
                **{n: q.grad for n, q in ag.named_parameters()}}

    monkeypatch.setattr(ops, "VIT_ATTN_BLOCK_MIN_SAMPLES", 1)  # route B = 3 whatever the default
    monkeypatch.setattr(ops, "VIT_ATTN_BLOCK_MAX_SAMPLES", 3)
    assert agent.fused_ok(src)
    on = grads(True, True)
    assert taken == [True, True]
    off = grads(False, True)
    assert taken == [True, True]
    f32, twin = grads(False, False), grads(False, False, torch.float64)
    for name in twin:
        tu.check(name + " (on)", on[name], f32[name], twin[name])
        tu.check(name + " (off)", off[name], f32[name], twin[name])
    attn, x = agent.network[0].transformer.layers[0][0], torch.randn(147, 32, generator=gen).to(dev)
    with torch.no_grad():  # the rollout's call: no statistics, same values
        y = real(x, attn, 49)
    assert not y.requires_grad and torch.equal(y, real(x, attn, 49).detach())
