"""ops.impala_resblock / ops.impala_conv_pool (csrc/ocppo_impala.hip), forward and backward,
against the f64 twin of the torch modules (F.conv2d / F.max_pool2d / autograd on the CPU), measured
beside torch's f32 on the same device and inputs.

Shapes (impala_util): images smaller than the halo (1 x 1, 2 x 3), one partial tile (11), 2 x 2
partial tiles (21, 17 x 23, non-square), whole tiles (42, 84), the tile edge 14 with its neighbours
(13 and 14 give 7 pooled rows, 15 gives 8), 16 and 32 channels, 3 and 4 input channels, 1 to 3
images, and 520 small images: more tiles than the 256 workgroups, so each takes two or three. Bound, per tensor: |d - d64|_inf / |d64|_inf <= max(4 x torch f32's, 2^-20)."""
from __future__ import annotations

import pytest
import torch

import impala_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ids(c):
    return "x".join(map(str, c))


@pytest.mark.parametrize("case", U.RES_CASES, ids=_ids)
def test_resblock_against_f64(case):
    from oc_cleanrl_amd import ops

    inputs, g, y64, g64 = U.res_case(case)
    y_ref, g_ref = U.run(U.res_block, inputs, g, torch.float32, DEV)
    y, gk = U.run(lambda *a: (ops.impala_resblock(*a),), inputs, g, torch.float32, DEV)
    assert y.shape == y64.shape and y.is_contiguous(memory_format=torch.channels_last)
    U.check(f"{case} y", y, y_ref, y64)
    for n, a, b, c in zip(("dx", "dw0", "db0", "dw1", "db1"), gk, g_ref, g64):
        U.check(f"{case} {n}", a, b, c)
    # no atomics: a second call is bitwise the first
    y2, gk2 = U.run(lambda *a: (ops.impala_resblock(*a),), inputs, g, torch.float32, DEV)
    assert torch.equal(y, y2) and all(torch.equal(a, b) for a, b in zip(gk, gk2))


@pytest.mark.parametrize("no_dx", (False, True), ids=("dx", "nodx"))
@pytest.mark.parametrize("case", U.CP_CASES, ids=_ids)
def test_conv_pool_against_f64(case, no_dx):
    from oc_cleanrl_amd import ops

    inputs, g, p64, g64 = U.cp_case(case)
    p_ref, g_ref = U.run(U.conv_pool, inputs, g, torch.float32, DEV, no_dx)
    p, gk = U.run(lambda *a: (ops.impala_conv_pool(*a),), inputs, g, torch.float32, DEV, no_dx)
    assert p.shape == p64.shape
    U.check(f"{case} p", p, p_ref, p64)
    names = ("dx", "dw", "db")[no_dx:]
    assert len(gk) == len(names)
    for n, a, b, c in zip(names, gk, g_ref, g64[no_dx:]):
        U.check(f"{case} {n}", a, b, c)


def test_scale_inference_and_refusals():
    from oc_cleanrl_amd import _lib, ops

    inputs, g, p64, _ = U.cp_case(U.CP_CASES[2])
    x, w, b = (t.to(DEV, torch.float32) for t in inputs)
    with torch.no_grad():
        p = ops.impala_conv_pool(x, w, b)
        # the scale is one f32 multiplication per element, bit for bit
        s = torch.tensor(1 / 255.0, dtype=torch.float32, device=DEV)
        assert torch.equal(ops.impala_conv_pool(x * 255.0, w, b, scale=float(s)),
                           ops.impala_conv_pool((x * 255.0) * s, w, b))
        # an NCHW input is copied to channels_last: the same result
        assert torch.equal(p, ops.impala_conv_pool(x.contiguous(), w, b))
    U.check("inference p", p, U.conv_pool(x, w, b)[0], p64)
    for cin, cout, res in ((16, 16, 1), (32, 32, 1), (4, 16, 0), (32, 32, 0)):
        params = 2 * (9 * cout * cout + cout) if res else 9 * cout * cin + cout
        assert int(_lib.LIB.ocppo_impala_workspace_bytes(cin, cout, res)) == 256 * params * 4
    assert int(_lib.LIB.ocppo_impala_workspace_bytes(16, 32, 1)) == 0
    assert int(_lib.LIB.ocppo_impala_workspace_bytes(8, 16, 0)) == 0
    conv = torch.nn.Conv2d(4, 16, 3, padding=1).to(DEV)
    assert ops.impala_ok(x, conv) and not ops.impala_ok(x.cpu(), conv)
    assert not ops.impala_ok(x, torch.nn.Conv2d(4, 16, 3).to(DEV))            # no padding
    assert not ops.impala_ok(x, torch.nn.Conv2d(4, 24, 3, padding=1).to(DEV))  # 24 channels
    with pytest.raises(ValueError):
        ops.impala_resblock(x, w, b, w, b)  # 4 channels, 4 -> 16 weights
    with pytest.raises(_lib.OcppoError):   # 8 input channels: refused before any launch
        ops.impala_conv_pool(x.repeat(1, 2, 1, 1), w.repeat(1, 2, 1, 1), b)
