"""The three PPG entries on the GPU: ops.ppg_aux_loss_fwd_bwd, ops.ppg_aux_gather and
ops.FlatAdamSegments (csrc/ocppo_ppg.hip, ocppo_clip_adam_step_seg)."""
from __future__ import annotations

import ctypes

import pytest
import torch

import ppg_util as U

pytestmark = pytest.mark.gpu


# ---- auxiliary loss ---------------------------------------------------------------------------------
def _aux_inputs(M, A):
    g = torch.Generator().manual_seed(M * 100 + A)
    new, old = (torch.randn((M, A), generator=g) * 2 for _ in range(2))
    v, av, ret = (torch.randn(M, generator=g) for _ in range(3))
    r = torch.arange(M)
    peaked, same = int(r[M // 2]), int(r[-1])
    if A > 1:
        new[peaked, 0] += 40.0  # a peaked row: logit gap 40
        old[0, A - 1] += 40.0
    new[same] = old[same]  # old == new: an exact-zero row
    ret[0], ret[-1] = 30.0, -30.0
    return new, v, av, old, ret, same


# rows per wave = rows per workgroup = 64 (one thread a row, one wave a workgroup), 1024
# workgroups at most: 63 / 64 / 65 straddle the wave and workgroup edge, 130 and 257 take several
# workgroups, 65537 rows are one past what 1024 workgroups hold (the grid-stride path)
@pytest.mark.parametrize("M, A", [(1, 1), (1, 2), (3, 6), (63, 7), (64, 8), (65, 18), (130, 9),
                                  (257, 18), (65537, 2)])
def test_ppg_aux_loss_fwd_bwd(dev, M, A):
    """Kernel boundaries: 64 rows per wave and per workgroup, 65536 rows per grid sweep."""
    from oc_cleanrl_amd import ops

    new, v, av, old, ret, same = _aux_inputs(M, A)
    beta = 0.7
    d = lambda t: t.to(dev)  # noqa: E731
    stats, dl, dv, da = ops.ppg_aux_loss_fwd_bwd(d(new), d(v), d(av), d(old), d(ret), beta)
    r32 = U.aux_ref(new, v, av, old, ret, beta, torch.float32)
    r64 = U.aux_ref(new, v, av, old, ret, beta, torch.float64)
    r64[1][same] = 0  # old == new: the gradient is 0, what f64 autograd leaves there is rounding
    for name, got, own, twin in zip(("stats", "dlogits", "dvalue", "daux"),
                                    (stats, dl, dv, da), r32, r64):
        if name == "stats":
            for k, n in enumerate(ops.PPG_STAT_NAMES):
                U.check(f"aux {n} M={M} A={A}", got[k], own[k], twin[k])
        else:
            U.check(f"aux {name} M={M} A={A}", got, own, twin)
    assert not bool(dl[same].any()), "old == new must give an all-zero dlogits row"
    # ... and kl_r == 0 exactly: that row alone has a zero mean
    s1, dl1, _, _ = ops.ppg_aux_loss_fwd_bwd(d(new[same:same + 1]), d(v[:1]), d(av[:1]),
                                             d(old[same:same + 1]), d(ret[:1]), beta)
    assert float(s1[0]) == 0.0 and not bool(dl1.any())
    # a second launch and a replayed graph are bitwise the first
    outs = [torch.empty_like(t) for t in (stats, dl, dv, da)]
    args = (d(new), d(v), d(av), d(old), d(ret), beta)
    ops.ppg_aux_loss_fwd_bwd(*args, outs[1], outs[2], outs[3], outs[0])
    first = [t.clone() for t in (stats, dl, dv, da)]
    for a, b in zip(first, outs):
        assert torch.equal(a, b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.ppg_aux_loss_fwd_bwd(*args, outs[1], outs[2], outs[3], outs[0])
    for t in outs:
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a, b)


def test_ppg_argument_errors_arrive_before_any_launch(dev):
    from oc_cleanrl_amd import _lib, ops

    L, p = _lib.LIB, ctypes.c_void_p(64)
    assert L.ocppo_ppg_aux_loss_fwd_bwd(None, p, p, p, p, p, 4, 19, 1.0, p, p, p, p, p,
                                        1 << 20) == _lib.OCPPO_E_INVALID
    assert b"A <= 18" in L.ocppo_last_error()
    assert L.ocppo_ppg_aux_loss_fwd_bwd(None, p, p, p, p, p, 4, 6, 1.0, p, p, p, p, p,
                                        8) == _lib.OCPPO_E_WORKSPACE
    assert L.ocppo_ppg_aux_gather(None, p, 7, p, p, p, 2, 2, 1, 4, 4, p, p, p) == \
        _lib.OCPPO_E_INVALID
    assert b"dtype" in L.ocppo_last_error()
    assert L.ocppo_clip_adam_step_seg(None, p, p, p, p, 128, 130, 1, p, 0.9, 0.999, 1e-8, 1.0,
                                      0.5, p, p, 1 << 20) == _lib.OCPPO_E_INVALID
    assert b"split" in L.ocppo_last_error()
    obs = torch.zeros((2, 3, 4), device=dev)
    pi, ret = torch.zeros((2, 3, 2), device=dev), torch.zeros((2, 3), device=dev)
    for bad in ([3], [-1], [0, 5]):
        with pytest.raises(IndexError, match="outside"):
            ops.ppg_aux_gather(obs, pi, ret, bad)


# ---- gather -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_ppg_aux_gather_is_bitwise_torch_indexing(dev, dtype):
    from oc_cleanrl_amd import ops

    g = torch.Generator().manual_seed(7)
    n = 0
    for T in (1, 5):
        for R in (3, 9):
            for D, A in [(D, A) for D in (1, 48, 130) for A in (1, 6, 18)]:
                shape = (T, R, 4, D // 4) if D == 48 else (T, R, D)
                obs = torch.randint(-256, 257, shape, generator=g).to(dtype).to(dev)
                pi = torch.randn((T, R, A), generator=g).to(dev)
                ret = torch.randn((T, R), generator=g).to(dev)
                for k in (1, 2, 4):
                    if k > R:
                        continue
                    # repeated columns and the last column
                    cols = [[R - 1], [R - 1, R - 1], [0, R - 1, 1, R - 1]][(1, 2, 4).index(k)]
                    ct = torch.tensor(cols, dtype=torch.int64, device=dev)
                    oo, op, orr = ops.ppg_aux_gather(obs, pi, ret, ct)
                    assert torch.equal(oo, U.flatten01(obs[:, ct]).float()), (T, R, D, A, k)
                    assert torch.equal(op, U.flatten01(pi[:, ct])), (T, R, D, A, k)
                    assert torch.equal(orr, U.flatten01(ret[:, ct])), (T, R, D, A, k)
                    assert oo.dtype == torch.float32 and tuple(oo.shape[1:]) == tuple(shape[2:])
                    n += 1
    assert n == 2 * 9 * (2 + 3)
    # a host list goes the same way; a device index out of range is clamped, never dereferenced
    a = ops.ppg_aux_gather(obs, pi, ret, [0, R - 1])
    b = ops.ppg_aux_gather(obs, pi, ret, torch.tensor([-5, R + 7], device=dev))
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- FlatAdamSegments -------------------------------------------------------------------------------
def _params(sizes, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in sizes]


def _live(opt):
    """Where the flat buffer holds parameters: the padding between them carries no gradient."""
    live = torch.zeros(opt.numel, dtype=torch.bool)
    for p in opt.param_list:
        off = (p.data_ptr() - opt.params.data_ptr()) // 4
        live[off:off + p.numel()] = True
    return live


def _grads(opt, step, seed=5):
    g = torch.Generator().manual_seed(seed * 100 + step)
    return torch.randn(opt.numel, generator=g)


# the skeleton's threads take 4 elements (one 16-B group) each, 256 threads a workgroup, so a
# workgroup's chunk is 1024 elements: a head of 1024 puts the tail at a chunk's edge, one of
# 1000 + 30 (padded to 1024 + 64) 16 threads into the second chunk, one of 5000 + 17 + 3 (padded
# to 5184) 16 threads into the sixth
@pytest.mark.parametrize("head_sizes", [(1024,), (1000, 30), (5000, 17, 3)])
def test_flat_adam_segments_against_flat_adam(dev, head_sizes):
    from oc_cleanrl_amd import ops

    tail_sizes = (70, 1)
    kw = dict(lr=1e-2, eps=1e-8, max_grad_norm=0.5)
    seg = ops.FlatAdamSegments(_params(head_sizes, dev, 1), _params(tail_sizes, dev, 2), **kw)
    ref = ops.FlatAdam(_params(head_sizes, dev, 1) + _params(tail_sizes, dev, 2), **kw)
    assert seg.numel == ref.numel and torch.equal(seg.params, ref.params)
    assert seg.split == ops.flat_offsets(seg.head_params)[1] and seg.split % 64 == 0
    live = _live(seg)
    # the tail always active: six steps bitwise FlatAdam on the same gradients
    for s in range(6):
        gr = (_grads(seg, s) * live).to(dev)
        seg.grads.copy_(gr)
        ref.grads.copy_(gr)
        seg.step(True)
        ref.step()
        for k in ("params", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(seg, k), getattr(ref, k)), (k, s)
        assert torch.equal(seg.scalars[:5], ref.scalars[:5])
    assert float(seg.scalars[ops.OPT_TAIL_STEP]) == 6 and float(seg.tail_step) == 6
    # the tail inactive (its gradients garbage here, zero there): the head bitwise FlatAdam over
    # the whole buffer, the tail's parameters, moments and count bit-unchanged
    sp = seg.split
    before = {k: getattr(seg, k)[sp:].clone() for k in ("params", "exp_avg", "exp_avg_sq")}
    for s in range(6, 9):
        gr = (_grads(seg, s) * live).to(dev)
        seg.grads.copy_(gr)  # the tail's gradients are left as they come: they must not be read
        gr[sp:] = 0
        ref.grads.copy_(gr)
        seg.step(False)
        ref.step()
        for k in ("params", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(seg, k)[:sp], getattr(ref, k)[:sp]), (k, s)
            assert torch.equal(getattr(seg, k)[sp:], before[k]), (k, s)
        assert torch.equal(seg.scalars[:5], ref.scalars[:5])
        assert float(seg.scalars[ops.OPT_TAIL_STEP]) == 6 and float(seg.tail_step) == 6
    assert float(seg.scalars[ops.OPT_STEP]) == 9
    assert float(seg.scalars[ops.OPT_TAIL_SKIPPED]) == 3
    with pytest.raises(ValueError, match="no weight planes"):
        seg.write_planes([(None, False, None)])


def test_flat_adam_segments_follows_torch_adam_with_grad_none(dev):
    """Three steps with the tail's grad None, then two with it: the parameter deltas against
    torch.optim.Adam on the CPU in f64, torch's f32 Adam being "torch's own"."""
    from oc_cleanrl_amd import ops

    head_sizes, tail_sizes = (1000, 30), (70, 1)
    kw = dict(lr=1e-2, eps=1e-8, max_grad_norm=0.5)
    seg = ops.FlatAdamSegments(_params(head_sizes, dev, 1), _params(tail_sizes, dev, 2), **kw)
    views = [(p, (p.data_ptr() - seg.params.data_ptr()) // 4) for p in seg.param_list]
    nh = len(head_sizes)
    p0 = [p.detach().cpu().clone() for p, _ in views]
    steps = [False, False, False, True, True]
    live = _live(seg)
    grads = [_grads(seg, s) * live for s in range(len(steps))]

    def reference(dtype):
        ps = [torch.nn.Parameter(t.to(dtype).clone()) for t in p0]  # .to(f32) alone is p0 itself
        opt = torch.optim.Adam(ps, lr=kw["lr"], eps=kw["eps"])
        for act, g in zip(steps, grads):
            for i, (p, (v, off)) in enumerate(zip(ps, views)):
                p.grad = (g[off:off + v.numel()].to(dtype).clone()
                          if i < nh or act else None)
            torch.nn.utils.clip_grad_norm_([p for p in ps if p.grad is not None],
                                           kw["max_grad_norm"])
            opt.step()
        assert int(opt.state[ps[0]]["step"]) == 5 and int(opt.state[ps[-1]]["step"]) == 2
        return [p.detach().double() - q.double() for p, q in zip(ps, p0)]

    for act, g in zip(steps, grads):
        seg.grads.copy_(g.to(dev))
        seg.step(act)
    assert float(seg.scalars[ops.OPT_STEP]) == 5 and float(seg.tail_step) == 2
    d32, d64 = reference(torch.float32), reference(torch.float64)
    for i, (p, _) in enumerate(views):
        got = p.detach().cpu().double() - p0[i].double()
        assert float(d64[i].abs().max()) > 0
        U.check(f"segment Adam parameter {i} delta", got, d32[i], d64[i])
