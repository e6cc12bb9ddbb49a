"""ops.rnd_body_forward / ops.rnd_body (csrc/ocppo_rnd_body.hip) against the torch CPU f64 chain
and its autograd on the f64-normalised frame.

Tolerance rule: on the same inputs the CPU f32 torch chain (on the f32-rounded normalised frame,
the script's arithmetic) has a max-abs error e32 against the f64 reference; the kernel's must be
at most MARGIN x e32. Both are f32 sums of the same length in different orders."""
from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MARGIN = 4.0
P = 84 * 84


def _chain(x, p):
    h = F.leaky_relu(F.conv2d(x, p[0], p[1], stride=4))
    h = F.leaky_relu(F.conv2d(h, p[2], p[3], stride=2))
    return F.leaky_relu(F.conv2d(h, p[4], p[5], stride=1)).flatten(1)


def _inputs(R: int, seed: int = 0):
    """u8 stacks [R, 4, 84, 84], statistics under which some pixels clip at +-5, two networks."""
    from oc_cleanrl_amd import rnd

    g = torch.Generator().manual_seed(seed)
    stacks = torch.randint(0, 256, (R, 4, 84, 84), generator=g, dtype=torch.uint8)
    state = torch.cat([torch.rand(P, generator=g, dtype=torch.float64) * 60 + 100,
                       (torch.rand(P, generator=g, dtype=torch.float64) * 100 + 15) ** 2,
                       torch.tensor([R + 1e-4], dtype=torch.float64)])
    torch.manual_seed(seed + 1)
    model = rnd.RNDModel("RND")
    for m in list(model.predictor)[:5] + list(model.target)[:5]:
        if hasattr(m, "bias"):
            torch.nn.init.uniform_(m.bias, -0.5, 0.5)
    return stacks, state, model


def _norm64(stacks, state, idx):
    x = stacks[:, 3].reshape(-1, P).double()
    x = ((x - state[:P]) / state[P:2 * P].sqrt()).clip(-5, 5)
    assert float(x.abs().max()) == 5.0 and float((x.abs() < 5).double().mean()) > 0.5
    return (x if idx is None else x[idx]).view(-1, 1, 84, 84)


def _params(seq, dtype):
    return [p.detach().to(dtype) for m in (seq[0], seq[2], seq[4]) for p in (m.weight, m.bias)]


def _check(name, got, ref32, ref64):
    e32 = float((ref32.double() - ref64).abs().max())
    err = float((got.double().cpu() - ref64).abs().max())
    print(f"{name}: kernel {err:.3e}  cpu-f32 {e32:.3e}  scale {float(ref64.abs().max()):.3e}")
    assert err <= MARGIN * e32, (name, err, e32)


def _gpu(stacks, state, model, dev):
    from oc_cleanrl_amd import ops

    st = stacks.to(dev)
    model = model.to(dev)
    return (st.view(-1, 4, P)[:, 3], state.to(dev), ops.rnd_body_convs(model.predictor),
            ops.rnd_body_convs(model.target))


@pytest.mark.parametrize("R", [1, 3, 33])
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("indexed", [False, True])
def test_forward(dev, R, two, indexed):
    from oc_cleanrl_amd import ops

    stacks, state, model = _inputs(R)
    idx = torch.cat([torch.randperm(R), torch.tensor([R // 2])]) if indexed else None
    x64 = _norm64(stacks, state, idx)
    frames, dstate, pc, tc = _gpu(stacks, state, model, dev)
    didx = None if idx is None else idx.to(dev)
    got = ops.rnd_body_forward(frames, didx, dstate, pc, tc if two else None)
    again = ops.rnd_body_forward(frames, didx, dstate, pc, tc if two else None)
    model = model.cpu()
    for name, seq, g, g2 in zip(("predictor", "target"), (model.predictor, model.target),
                                got if two else (got,), again if two else (again,)):
        assert g.shape == (x64.shape[0], 3136) and torch.equal(g, g2)
        ref64 = _chain(x64, _params(seq, torch.float64))
        assert float(ref64.min()) < 0 < float(ref64.max())  # both LeakyReLU branches
        _check(f"fwd R={R} {name}", g, _chain(x64.float(), _params(seq, torch.float32)), ref64)


@pytest.mark.parametrize("off", [None, -1, 0, 1])  # R = 1, CHUNK - 1, CHUNK, CHUNK + 1
def test_backward(dev, off):
    from oc_cleanrl_amd import ops

    R = 1 if off is None else ops.RND_BODY_CHUNK + off
    stacks, state, model = _inputs(R, seed=R)
    dout = torch.randn(R, 3136, generator=torch.Generator().manual_seed(R))
    if R > 1:
        dout[1::3] = 0  # rows the update mask drops
    x64 = _norm64(stacks, state, None)
    refs = {}
    for dt in (torch.float64, torch.float32):
        p = [t.requires_grad_() for t in _params(model.predictor, dt)]
        refs[dt] = torch.autograd.grad(_chain(x64.to(dt), p), p, dout.to(dt))
    frames, dstate, pc, _ = _gpu(stacks, state, model, dev)
    params = [p for m in pc for p in (m.weight, m.bias)]
    runs = []
    for _ in range(2):
        out = ops.rnd_body(frames, None, dstate, pc)
        runs.append(torch.autograd.grad(out, params, dout.to(dev)))
    names = ("dw1", "db1", "dw2", "db2", "dw3", "db3")
    for n, g, g2, r32, r64 in zip(names, *runs, refs[torch.float32], refs[torch.float64]):
        assert torch.equal(g, g2), n
        _check(f"bwd R={R} {n}", g, r32, r64)


def test_wrong_geometry_is_refused_before_any_launch(dev):
    from oc_cleanrl_amd import _lib, ops

    stacks, state, model = _inputs(2)
    frames, dstate, pc, _ = _gpu(stacks, state, model, dev)
    out = torch.full((2, 3136), 7.0, device=dev)
    ptrs = [p.data_ptr() for m in pc for p in (m.weight, m.bias)]
    for H, W, c1 in ((80, 84, 32), (84, 84, 16)):
        rc = _lib.LIB.ocppo_rnd_body_fwd(None, frames.data_ptr(), 2, 4 * P, None, 2, H, W, c1, 64,
                                         64, dstate.data_ptr(), *ptrs, *([None] * 6),
                                         out.data_ptr(), None, None, None)
        assert rc == _lib.OCPPO_E_INVALID and b"geometry" in _lib.LIB.ocppo_last_error()
    dws = [torch.full_like(p, 7.0) for m in pc for p in (m.weight, m.bias)]
    ws = torch.empty(_lib.LIB.ocppo_rnd_body_workspace_bytes(2) // 4, device=dev)
    a = torch.zeros(2, 12800, device=dev)
    rc = _lib.LIB.ocppo_rnd_body_bwd(None, frames.data_ptr(), 2, 4 * P, None, 2, 84, 80, 32, 64, 64,
                                     dstate.data_ptr(), a.data_ptr(), a.data_ptr(), out.data_ptr(),
                                     ptrs[2], ptrs[4], out.data_ptr(), *[d.data_ptr() for d in dws],
                                     ws.data_ptr(), ws.numel() * 4)
    assert rc == _lib.OCPPO_E_INVALID
    torch.cuda.synchronize()
    assert float(out.min()) == float(out.max()) == 7.0
    assert all(float(d.min()) == float(d.max()) == 7.0 for d in dws)
    assert not ops.rnd_body_ok(frames[:, :100], dstate, pc)
