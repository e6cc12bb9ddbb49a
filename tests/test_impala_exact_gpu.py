"""ops.impala_resblock / ops.impala_conv_pool (csrc/ocppo_impala.hip) against the f64 twin, bit
for bit and element by element, forward and backward, on small-integer inputs (impala_util, "the
exact cases"): every operation of the two units is then exact in f32 in any summation order, so
there is no tolerance anywhere in this file. What the margin-based cases of
test_impala_kernels_gpu.py assert away is the subject here:

  pool ties       which of several maximal window positions the gradient goes to (the first in
                  row-major order, as torch), in >= 5 % of the windows of every case
  ReLU at 0       x == 0 and a mid pre-activation == 0 (relu'(0) = 0) in the residual block
  instantiations  all six imp_cp_{fwd,bwd}_kernel<CI, CO>, input channels 1, 2, 3 and 4 (every
                  `left` of the partial load), both scales where they apply
  per element     a wrong value at one halo or clamped-duplicate position fails, however small
  NaN             the pool's `v != v` clause: a NaN in x reaches exactly the twin's outputs

Shapes: below the halo (1 x 1, 2 x 3), the tile edge 14 and its neighbours, 2 x 2 and 3 x 3 tiles
with partial ones (17 x 23, 29 x 29, 29 x 30), odd and even H and W, and 520 images on the 256
workgroups. Beside the kernel, torch's own f32 result on the device must equal the twin too (the
case really is exact), the NCHW and channels_last inputs must agree bitwise, and without dx the
parameter gradients must be bitwise those of the run with it."""
from __future__ import annotations

import pytest
import torch

import impala_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32


def _exact(checks):
    """U.assert_exact on every (name, got, twin); all the failures in one report."""
    errs = []
    for name, got, twin in checks:
        try:
            U.assert_exact(name, got, twin)
        except AssertionError as e:
            errs.append(str(e))
    assert not errs, "\n".join(errs)


def _bitwise(name, a, b):
    assert len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b)), name


@pytest.mark.parametrize("case", U.LATTICE_RES_CASES, ids=U.res_id)
def test_resblock_exact(case):
    from oc_cleanrl_amd import ops

    inputs, g, y64, g64, _ = U.lattice_res_case(case)
    names = ("dx", "dw0", "db0", "dw1", "db1")
    kernel = lambda *a: (ops.impala_resblock(*a),)  # noqa: E731
    y, gk = U.run(kernel, inputs, g, F32, DEV, channels_last=True)
    assert len(gk) == len(names)
    _exact([("y", y, y64)] + list(zip(names, gk, g64)))
    y_t, g_t = U.run(U.res_block, inputs, g, F32, DEV)
    _exact([("torch f32 y", y_t, y64)] + [("torch f32 " + n, a, b)
                                           for n, a, b in zip(names, g_t, g64)])
    y_n, g_n = U.run(kernel, inputs, g, F32, DEV)
    _bitwise("NCHW input", [y] + gk, [y_n] + g_n)


@pytest.mark.parametrize("case", U.LATTICE_CP_CASES, ids=U.cp_id)
def test_conv_pool_exact(case):
    from oc_cleanrl_amd import ops

    scale = case[5]
    inputs, g, p64, g64, _ = U.lattice_cp_case(case)
    names = ("dx", "dw", "db")
    kernel = lambda x, w, b: (ops.impala_conv_pool(x, w, b, scale),)  # noqa: E731
    p, gk = U.run(kernel, inputs, g, F32, DEV, channels_last=True)
    assert len(gk) == len(names)
    _exact([("p", p, p64)] + list(zip(names, gk, g64)))
    p_0, g_0 = U.run(kernel, inputs, g, F32, DEV, no_dx=True, channels_last=True)
    _exact([("no dx: p", p_0, p64)] + [("no dx: " + n, a, b)
                                        for n, a, b in zip(names[1:], g_0, g64[1:])])
    _bitwise("no dx", [p] + gk[1:], [p_0] + g_0)
    p_t, g_t = U.run(U.scaled_conv_pool(scale), inputs, g, F32, DEV)
    _exact([("torch f32 p", p_t, p64)] + [("torch f32 " + n, a, b)
                                           for n, a, b in zip(names, g_t, g64)])
    p_n, g_n = U.run(kernel, inputs, g, F32, DEV)
    _bitwise("NCHW input", [p] + gk, [p_n] + g_n)


@pytest.mark.parametrize("pair", U.NAN_CP_CASES, ids=lambda p: f"cin{p[0]}-cout{p[1]}")
def test_conv_pool_nan(pair):
    from oc_cleanrl_amd import ops

    inputs, p64 = U.nan_cp_case(pair)
    with torch.no_grad():
        p = ops.impala_conv_pool(*(t.to(DEV, F32) for t in inputs)).double().cpu()
    nan = p64.isnan()
    assert torch.equal(p.isnan(), nan), (int(p.isnan().sum()), int(nan.sum()))
    U.assert_exact("p off the NaNs", p.masked_fill(nan, 0.0), p64.masked_fill(nan, 0.0))
