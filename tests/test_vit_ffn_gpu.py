"""ops.vit_ffn (csrc/ocppo_vit_ffn.hip, f32 MFMA): y = x + W2 gelu(W1 LN(x) + b1) + b2 and its eight
gradients against the float64 torch chain under the project's error rule (transformer_util.check:
at most max(3 x torch's own f32 error, 4 * 2^-23) of the twin's largest element), constant rows,
saturated GELU, identical dy rows, bitwise repeatability eager and as a replayed hipGraph, the
contract's statuses and the agent's route. Run with -s for the (measured / torch's own) pairs."""
import copy

import pytest
import torch
import torch.nn.functional as F

import transformer_util as tu

pytestmark = pytest.mark.gpu

NAMES = ("y", "dx", "dgamma", "dbeta", "dW1", "db1", "dW2", "db2")


def _case(dev, rows, D, H, seed):
    """[x, gamma, beta, W1, b1, W2, b2, dy] on dev."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    c = [r(rows, D) * 2 + 0.5, 1 + 0.1 * r(D), 0.1 * r(D), r(H, D) / D ** 0.5, 0.1 * r(H),
         r(D, H) / H ** 0.5, 0.1 * r(D), r(rows, D)]
    return [t.to(dev) for t in c]


def _twin(c, dtype):
    x, g, b, W1, b1, W2, b2 = (t.detach().to(dtype).clone().requires_grad_(True) for t in c[:7])
    y = x + F.linear(F.gelu(F.linear(F.layer_norm(x, x.shape[1:], g, b), W1, b1)), W2, b2)
    y.backward(c[7].to(dtype))
    return [y.detach(), x.grad, g.grad, b.grad, W1.grad, b1.grad, W2.grad, b2.grad]


def _run(c, out=None):
    from oc_cleanrl_amd import ops

    x, g, b, W1, b1, W2, b2, dy = c
    y, mean, rstd = ops.vit_ffn_fwd(x, g, b, W1, b1, W2, b2, 1e-5, True, *(out or [None] * 3)[:3])
    return [y, *ops.vit_ffn_bwd(dy, x, mean, rstd, g, b, W1, b1, W2, out and tuple(out[3:]))]


def _check_all(c):
    got, f32, f64 = _run(c), _twin(c, torch.float32), _twin(c, torch.float64)
    for n, a, o, t in zip(NAMES, got, f32, f64):
        tu.check(n, a, o, t)
    return got


def _many_parts_rows():
    """More tiles than the backward has workgroups: some own two tiles, the finish adds the cap."""
    from oc_cleanrl_amd import ops

    return ops.VIT_FFN_TILE_ROWS * (ops.VIT_FFN_MAX_PARTS + 1) + 1


@pytest.mark.parametrize("D,H", [(32, 32), (128, 128), (64, 96), (128, 32)])
@pytest.mark.parametrize("rows", [1, 49, 64, 65, 147])
def test_vit_ffn_matches_f64_twin(dev, rows, D, H):
    _check_all(_case(dev, rows, D, H, seed=rows * 7 + D + H))


def test_vit_ffn_more_tiles_than_workgroups(dev):
    _check_all(_case(dev, _many_parts_rows(), 32, 32, seed=3))


def test_constant_rows_saturated_gelu_identical_dy(dev):
    c = _case(dev, 96, 128, 128, seed=9)
    x, _, _, W1, b1, _, _, dy = c
    x[0], x[1], x[70] = 0.0, 200.0, -3.5
    W1[:3] = 0.0
    b1[:3] = torch.tensor([0.0, 12.0, -12.0], device=dev)  # z = 0, beyond +10, beyond -10
    dy[:] = dy[:1].clone()
    got = _check_all(c)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    y = got[0]  # u == beta on a constant row: what is added to x there is one and the same row
    assert torch.equal(y[1], y[0] + 200.0) and torch.equal(y[70], y[0] - 3.5)


def test_repeatable_eager_and_graph(dev):
    c = _case(dev, 147, 128, 128, seed=5)
    ref = _run(c)
    assert all(torch.equal(a, b) for a, b in zip(ref, _run(c)))
    mean, rstd = torch.empty(147, device=dev), torch.empty(147, device=dev)
    out = [torch.empty_like(ref[0]), mean, rstd, *(torch.empty_like(t) for t in ref[1:])]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(c, out)  # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _run(c, out)
    for _ in range(3):
        for t in out:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(ref, [out[0], *out[3:]]))


@pytest.mark.parametrize("rows,D,H", [(64, 48, 128), (64, 128, 160), (0, 128, 128), (64, 128, 128)])
def test_contract_statuses_leave_outputs_untouched(dev, rows, D, H):
    """D = 48, H = 160: OCPPO_E_INVALID; rows = 0: nothing launched; a workspace one byte short:
    OCPPO_E_WORKSPACE. The sentinel-filled outputs stay as they were."""
    from oc_cleanrl_amd import _lib

    L, n = _lib.LIB, 64
    z = torch.zeros(256 * 256, device=dev)
    outs = [torch.full((k,), 7.0, device=dev) for k in (n * D, n, n, D, D, H * D, H, D * H, D)]
    y, mean, rstd, dx, dg, db, dW1, db1, dW2 = (t.data_ptr() for t in outs)
    st, p = torch.cuda.current_stream().cuda_stream, z.data_ptr()
    bad = rows and (D, H) != (128, 128)
    want = _lib.OCPPO_E_INVALID if bad else _lib.OCPPO_OK
    if rows == 0 or bad:
        assert L.ocppo_vit_ffn_fwd(st, p, p, p, p, p, p, p, rows, D, H, 1e-5, y, mean, rstd) == want
    assert L.ocppo_vit_ffn_workspace_bytes(rows, D, H) == 0 if bad else True
    nb = 0 if bad else L.ocppo_vit_ffn_workspace_bytes(rows, D, H) - 1
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev)
    rc = L.ocppo_vit_ffn_bwd(st, p, p, p, p, p, p, p, p, p, rows, D, H, dx, dg, db, dW1, db1, dW2,
                             y, ws.data_ptr(), nb)
    assert rc == (want if rows == 0 or bad else _lib.OCPPO_E_WORKSPACE)
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in outs)


def test_vit_agent_routes_through_fused_ffn(dev, monkeypatch):
    from oc_cleanrl_amd import ops, vit
    from oc_cleanrl_amd.agents import EnvSpec

    torch.manual_seed(21)
    gen = torch.Generator().manual_seed(22)
    agent = vit.ViTAgent(EnvSpec((4, 84, 84), 6), emb_dim=32, num_heads=2, num_blocks=2).to(dev)
    src = torch.randint(0, 256, (3, 4, 84, 84), generator=gen, dtype=torch.uint8).to(dev)
    dl, dv = torch.randn(3, 6, generator=gen).to(dev), torch.randn(3, 1, generator=gen).to(dev)
    taken = []
    real = ops.vit_ffn
    monkeypatch.setattr(ops, "vit_ffn", lambda x, ff: taken.append(ops.vit_ffn_ok(x, ff)) or real(x, ff))

    def grads(fused_ffn, stacks, dtype=torch.float32):
        monkeypatch.setattr(vit, "FUSED_FFN", fused_ffn)
        ag = copy.deepcopy(agent).to(dtype)
        hidden = ag.trunk_stacks(src, None) if stacks else ag.trunk(src)
        logits, value = ag.actor(hidden), ag.critic(hidden)
        torch.autograd.backward([logits, value], [dl.to(dtype), dv.to(dtype)])
        return {"logits": logits.detach(), "value": value.detach(),
                **{n: q.grad for n, q in ag.named_parameters()}}

    monkeypatch.setattr(ops, "VIT_FFN_MIN_ROWS", 1)  # 3 x 49 rows: below the measured routing floor
    assert agent.fused_ok(src)
    on = grads(True, True)
    assert taken == [True, True]
    off = grads(False, True)
    assert taken == [True, True]
    f32, twin = grads(False, False), grads(False, False, torch.float64)
    for name in twin:
        tu.check(name + " (on)", on[name], f32[name], twin[name])
        tu.check(name + " (off)", off[name], f32[name], twin[name])
    ff, x = agent.network[0].transformer.layers[0][1], torch.randn(147, 32, generator=gen).to(dev)
    with torch.no_grad():  # the rollout's call: no statistics, same values
        y = real(x, ff)
    assert not y.requires_grad and torch.equal(y, real(x, ff).detach())
