"""ops.ln_chw_relu (csrc/ocppo_ln_chw.hip): relu(LayerNorm over [C, H, W]) with its backward in
both memory formats against F.layer_norm + F.relu in float64 on the CPU, by the DESIGN 11 rule
(pqn_util.check): error against the f64 twin, relative to the twin's largest element,
<= max(3 x the f32 torch computation's own error, 4 * 2^-23). Two runs are bitwise equal."""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

import pqn_util as U

pytestmark = pytest.mark.gpu

# smallest row; scalar path narrower than a wave; scalar path; the first width ops.ln_relu
# refuses; the script's three shapes; the contract's edge
SHAPES = [(1, 1, 1), (3, 1, 5), (5, 3, 3), (1, 1, 1025), (64, 7, 7), (64, 9, 9), (32, 20, 20),
          (64, 16, 16)]


@pytest.fixture(scope="module")
def ops():
    from oc_cleanrl_amd import ops

    return ops


def _twin(x, w, b, dy, eps, relu, dtype):
    """y, mean, rstd and the gradients of sum(y * dy) on `dtype` CPU copies."""
    x, w, b = (t.detach().cpu().to(dtype).requires_grad_() for t in (x, w, b))
    y = F.layer_norm(x, x.shape[1:], w, b, eps)
    y = F.relu(y) if relu else y
    (y * dy.to(dtype)).sum().backward()
    flat = x.detach().flatten(1)
    mean = flat.mean(1)
    var = ((flat - mean.unsqueeze(1)) ** 2).mean(1)
    return dict(y=y.detach(), mean=mean, rstd=1.0 / torch.sqrt(var + eps), dx=x.grad, dw=w.grad,
                db=b.grad)


def _run(ops, dev, x, w, b, dy, relu, cl, eps=1e-5):
    fmt = torch.channels_last if cl else torch.contiguous_format
    xd, dyd = (t.to(dev).contiguous(memory_format=fmt) for t in (x, dy))
    y, mean, rstd = ops.ln_chw_relu_fwd(xd, w.to(dev), b.to(dev), eps, relu)
    dx, dw, db = ops.ln_chw_relu_bwd(dyd, xd, y, w.to(dev), mean, rstd, relu)
    assert y.is_contiguous(memory_format=fmt) and dx.is_contiguous(memory_format=fmt)
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, dw=dw, db=db)


def _check(ops, dev, x, w, b, dy, relu, cl, tag):
    got = _run(ops, dev, x, w, b, dy, relu, cl)
    again = _run(ops, dev, x, w, b, dy, relu, cl)
    f32, twin = (_twin(x, w, b, dy, 1e-5, relu, t) for t in (torch.float32, torch.float64))
    for k in got:
        U.check(f"ln_chw {tag} {tuple(x.shape)} {k}", got[k], f32[k], twin[k])
        assert torch.equal(got[k], again[k]), k  # two runs, bit for bit
    return got


def _params(shape, g):
    return torch.rand(shape, generator=g) + 0.5, torch.randn(shape, generator=g) * 0.5


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("cl", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_parity_and_determinism(ops, dev, shape, cl, relu):
    g = torch.Generator().manual_seed(sum(shape))
    w, b = _params(shape, g)
    # past the partial cap (and the grid stride of the workgroups' rows) at the three smallest
    rows = (1, 3) + ((ops.LN_CHW_MAX_PARTS + 2,) if shape in SHAPES[:3] else ())
    for R in rows:
        x = torch.randn(R, *shape, generator=g) * 2 + 0.5
        dy = torch.randn(R, *shape, generator=g)
        got = _check(ops, dev, x, w, b, dy, relu, cl, f"R={R} cl={cl} relu={relu}")
        if relu:
            assert bool((got["y"] >= 0).all())


@pytest.mark.parametrize("shape", [(5, 3, 3), (64, 7, 7)], ids=str)
def test_special_rows(ops, dev, shape):
    g = torch.Generator().manual_seed(31)
    w, b = _params(shape, g)
    dy = torch.randn(3, *shape, generator=g)
    # a constant row: variance 0, rstd = eps^-1/2, finite output
    x = torch.randn(3, *shape, generator=g)
    x[1] = 0.7
    got = _check(ops, dev, x, w, b, dy, True, True, "const")
    assert abs(float(got["rstd"][1]) - 1e-5 ** -0.5) <= 1e-5 ** -0.5 * 2.0 ** -20
    assert bool(torch.isfinite(got["y"]).all()) and bool(torch.isfinite(got["dx"]).all())
    # a row of 1000 + small noise: the re-centring
    x = torch.randn(3, *shape, generator=g)
    x[2] = 1000.0 + 1e-2 * torch.randn(shape, generator=g)
    _check(ops, dev, x, w, b, dy, True, True, "offset")
    # all-negative pre-activations: exact zeros everywhere
    x = torch.randn(3, *shape, generator=g)
    neg = -(w * 6 + 1)  # the normalised rows stay within [-6, 6] (checked): xhat w + neg <= -1
    flat = x.flatten(1)
    assert float(((flat - flat.mean(1, keepdim=True)) / flat.std(1, keepdim=True)).abs().max()) < 6
    got = _run(ops, dev, x, w, neg, dy, True, True)
    for k in ("y", "dx", "dw", "db"):
        assert bool((got[k] == 0).all()), k


def test_autograd_channels_last(ops, dev):
    g = torch.Generator().manual_seed(7)
    shape = (64, 7, 7)
    w, b = _params(shape, g)
    x, dy = torch.randn(3, *shape, generator=g), torch.randn(3, *shape, generator=g)
    xs = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_()
    ws, bs = (t.to(dev).requires_grad_() for t in (w, b))
    y = ops.ln_chw_relu(xs, ws, bs)
    y.backward(dy.to(dev))  # an NCHW gradient: the function brings it to the input's format
    f32, twin = (_twin(x, w, b, dy, 1e-5, True, t) for t in (torch.float32, torch.float64))
    for k, got in (("y", y.detach()), ("dx", xs.grad), ("dw", ws.grad), ("db", bs.grad)):
        U.check(f"ln_chw autograd {k}", got, f32[k], twin[k])


def test_contract(ops, dev):
    from oc_cleanrl_amd import _lib

    L, E = _lib.LIB, ops.LN_CHW_MAX_E + 1
    ln = torch.nn.LayerNorm([1, 1, E]).to(dev)
    x = torch.zeros(2, 1, 1, E, device=dev)
    assert not ops.ln_chw_ok(x, ln)
    assert ops.ln_chw_ok(x[..., 1:], torch.nn.LayerNorm([1, 1, E - 1]).to(dev)) is False  # strided
    p, v = x.data_ptr(), ln.weight.data_ptr()
    # y = 1 where x = 0 and beta = 1: a refused call launches nothing, so y keeps its zeros
    y, st = torch.zeros_like(x), torch.zeros(2, device=dev)
    with torch.no_grad():
        ln.bias.fill_(1.0)
    assert L.ocppo_ln_chw_relu_fwd(None, p, v, ln.bias.data_ptr(), 2, 1, E, 0, 1e-5, 1,
                                   y.data_ptr(), st.data_ptr(), st.data_ptr()) == _lib.OCPPO_E_INVALID
    torch.cuda.synchronize()
    assert bool((y == 0).all())
    assert L.ocppo_ln_chw_workspace_bytes(2, E) == 0
    need = L.ocppo_ln_chw_workspace_bytes(2, 64)
    assert need == 2 * 2 * 64 * 4
    ws = torch.zeros(need // 4, device=dev)
    s = st.data_ptr()
    assert L.ocppo_ln_chw_relu_bwd(None, p, p, p, v, s, s, 2, 4, 16, 1, 1, y.data_ptr(), v,
                                   ln.bias.data_ptr(), ws.data_ptr(), need - 4) == _lib.OCPPO_E_WORKSPACE
