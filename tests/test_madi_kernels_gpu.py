"""ops.madi_mask / ops.madi_mask_bwd (csrc/ocppo_madi.hip) against the f64 twin of the torch
modules, measured beside the torch f32 modules on the same device.

Shapes (madi_util.CASES): H 1 and 3 (smaller than the halo), the forward tile edge 14 and the
backward's 10 with their neighbours (9 .. 15), 17, 29 (2 x 14 + 1 = 3 x 10 - 1), 33 and one 84;
1, 2 and 5 frames and 4-frame stacks; 16 and 32 filters. Every case's seed keeps the f64 twin's
ReLU pre-activations at |z| >= 1e-5 (asserted), so no unit flips between f32 and f64.

Bounds (the issue's): forward max|y - y64| <= 4 err_ref + one f32 ulp at 255, err_ref the torch f32
modules' same measure; backward, per tensor, |d - d64|_inf / |d64|_inf <= max(4 x torch f32
autograd's, 2^-20). The factor 4 is the margin for another accumulation order over K = 288."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import madi_util as U

pytestmark = pytest.mark.gpu

ULP_255 = float(np.spacing(np.float32(255.0)))
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")
DEV = "cuda"


def _dev(case):
    return case["x"].to(DEV), tuple(w.to(DEV) for w in case["weights"]), case["g"].to(DEV)


def _rel(d, d64):
    return float((d.double().cpu() - d64).abs().max() / d64.abs().max())


@pytest.mark.parametrize("shape", U.CASES, ids=lambda s: "b%dw%dh%df%d" % s)
def test_forward_and_backward_against_f64(shape):
    from oc_cleanrl_amd import ops

    case, y64, g64, zmin = U.case_and_twin(shape)
    assert zmin >= U.Z_MIN, zmin
    x, ws, g = _dev(case)
    y_ref, d_ref, _ = U.reference(case, torch.float32, DEV)
    y = ops.madi_mask(x, None, ws)
    err = float((y.double().cpu() - y64).abs().max())
    err_ref = float((y_ref.double().cpu() - y64).abs().max())
    print(f"fwd {shape}: err {err:.3e} ref {err_ref:.3e} ratio {err / max(err_ref, 1e-30):.2f}")
    assert err <= 4 * err_ref + ULP_255
    d = ops.madi_mask_bwd(x, None, ws, g)
    torch.cuda.synchronize()
    for n, a, b, c in zip(NAMES, d, d_ref, g64):
        ek, er = _rel(a, c), _rel(b, c)
        print(f"bwd {shape} {n}: kernel {ek:.3e} torch {er:.3e}")
        assert ek <= max(4 * er, 2.0 ** -20), n


def test_index_u8_f32_and_layouts_bitwise():
    from oc_cleanrl_amd import ops

    case, *_ = U.case_and_twin((1, 4, 17, 32))
    gen = torch.Generator().manual_seed(5)
    rows = torch.randint(0, 256, (6, 4, 17, 17), generator=gen).to(torch.uint8).to(DEV)
    _, ws, _ = _dev(case)
    idx = torch.tensor([4, 1, 1, 0, 5, 4], device=DEV)  # repeated, out of order
    ident = torch.arange(6, device=DEV)
    y_idx = ops.madi_mask(rows, idx, ws)
    y_f32 = ops.madi_mask(rows.float()[idx].contiguous(), None, ws)
    assert torch.equal(y_idx, y_f32)
    assert torch.equal(ops.madi_mask(rows, ident, ws), ops.madi_mask(rows, None, ws))
    assert torch.equal(ops.madi_mask(rows.float(), idx, ws), y_idx)
    y_cl = ops.madi_mask(rows, idx, ws, channels_last=True)
    assert y_cl.is_contiguous(memory_format=torch.channels_last) and torch.equal(y_cl, y_idx)
    # rows the index does not name are not read into the result
    other = rows.clone()
    other[2], other[3] = 255 - other[2], 0
    assert torch.equal(ops.madi_mask(other, idx, ws), y_idx)
    # the backward reads the same rows and both layouts of g
    g = torch.randn((6, 4, 17, 17), generator=gen).to(DEV)
    d = ops.madi_mask_bwd(rows, idx, ws, g)
    d_f32 = ops.madi_mask_bwd(rows.float()[idx].contiguous(), None, ws, g)
    d_cl = ops.madi_mask_bwd(other, idx, ws, g.contiguous(memory_format=torch.channels_last))
    for a, b, c in zip(d, d_f32, d_cl):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_backward_deterministic_and_workspace_bound():
    from oc_cleanrl_amd import _lib, ops

    case, *_ = U.case_and_twin((5, 1, 33, 32))
    x, ws, g = _dev(case)
    a = [t.clone() for t in ops.madi_mask_bwd(x, None, ws, g)]
    b = ops.madi_mask_bwd(x, None, ws, g)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    # 256 partial rows of the parameter count, whatever the number of frames
    for F in (16, 32):
        params = 9 * F + F + 9 * F * F + F + 9 * F + 1
        assert int(_lib.LIB.ocppo_madi_workspace_bytes(F)) == 256 * params * 4
        assert ops.madi_workspace(F, DEV).numel() == 256 * params
    assert int(_lib.LIB.ocppo_madi_workspace_bytes(8)) == 0
    # more tiles than workgroups: 300 frames of one 10 x 10 tile each through the same workspace
    big = x[:1, :, :10, :10].repeat(300, 1, 1, 1).contiguous()
    gb = g[:1, :, :10, :10].repeat(300, 1, 1, 1).contiguous()
    one = ops.madi_mask_bwd(big[:1].contiguous(), None, ws, gb[:1].contiguous())
    many = [t.clone() for t in ops.madi_mask_bwd(big, None, ws, gb)]
    again = ops.madi_mask_bwd(big, None, ws, gb)
    for s, t in zip(many, again):  # several tiles per workgroup: still bitwise
        assert torch.equal(s, t)
    for s, t in zip(one, many):
        assert torch.allclose(t, 300 * s, rtol=1e-4, atol=1e-6 * float(t.abs().max()))


def test_initial_weights_forward():
    """Delta-orthogonal initial weights (off-centre taps zero, zero biases): the same bound."""
    from oc_cleanrl_amd import madi, ops

    torch.manual_seed(3)
    m = madi.MaskerNet((4, 33, 33), 3, 32)
    x = torch.randint(0, 256, (2, 4, 33, 33)).to(torch.uint8)
    with torch.no_grad():
        y64 = U.masker(x.double(), tuple(w.double() for w in m.weights()))
        y_ref = U.masker(x.float().to(DEV), tuple(w.to(DEV) for w in m.weights()))
        y = ops.madi_mask(x.to(DEV), None, tuple(w.detach().to(DEV) for w in m.weights()))
    err = float((y.double().cpu() - y64).abs().max())
    err_ref = float((y_ref.double().cpu() - y64).abs().max())
    print(f"init fwd: err {err:.3e} ref {err_ref:.3e}")
    assert err <= 4 * err_ref + ULP_255


def test_refuses_bad_arguments():
    from oc_cleanrl_amd import _lib, ops

    case, *_ = U.case_and_twin((1, 1, 3, 16))
    x, ws, g = _dev(case)
    with pytest.raises(ValueError):
        ops.madi_mask(x[:, :, :, :2].contiguous(), None, ws)
    with pytest.raises(ValueError):
        ops.madi_mask(x.to(torch.int32), None, ws)
    with pytest.raises(ValueError):
        ops.madi_mask(x.cpu(), None, ws)
    with pytest.raises(_lib.OcppoError):  # refused before any launch
        ops.madi_mask_bwd(x, None, ws, g, workspace=torch.empty(8, device=DEV))
