"""The six RND entries (csrc/ocppo_rnd.hip) through ops against the restatements of
tests/rnd_util.py: exact rational running statistics, the f64 twin under the project's error rule,
and bitwise where the script's f32 op order is kept (the reward filter, both GAE scans, the
mask)."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import rnd_util as U

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "u8": torch.uint8}


def _source(R, C, name, strided, seed=0):
    """x [R, C] of dtype `name` (a slice of a wider stack when strided) and its f64 values."""
    g = torch.Generator().manual_seed(seed + 1000 * R + C)
    W = 3 if strided else 1
    if name == "u8":
        full = torch.randint(0, 256, (R, W, C), generator=g, dtype=torch.uint8)
    else:
        full = (torch.randn((R, W, C), generator=g) * 40 + 100).to(DTYPES[name])
    return full, full[:, -1].double().numpy()


def _state_np(state, C):
    s = state.cpu().numpy()
    return s[:C], s[C:2 * C], float(s[2 * C])


@pytest.mark.parametrize("name", ["f32", "bf16", "u8"])
@pytest.mark.parametrize("strided", [False, True])
def test_rms_update_and_normalize(dev, name, strided):
    from oc_cleanrl_amd import ops

    for R in (1, 63, 65, 257):
        for C in (1, 7, 130):
            full, x64 = _source(R, C, name, strided)
            x = full.to(dev)[:, -1]
            state = ops.rms_state(C, dev)
            ops.rms_update(x, state)
            twin, _ = U.rms_update_exact(U.rms_init(C), x64)
            own = U.rms_update_np(U.rms_init(C), x64)
            got = _state_np(state, C)
            for k, nm in enumerate(("mean", "var")):
                U.check64(f"rms {name} {R}x{C} {nm}", got[k], own[k], twin[k])
            assert got[2] == twin[2] == 1e-4 + R
            out = ops.rnd_normalize(x, state)
            ref = U.normalize_ref(x64, got[0], got[1])
            U.check(f"normalize {name} {R}x{C}", out, ref.astype(np.float32), ref)
            assert out.shape == (R, C) and bool(torch.isfinite(out).all())


def test_rms_constant_column_and_two_updates(dev):
    from oc_cleanrl_amd import ops

    R, C = 65, 7
    g = torch.Generator().manual_seed(5)
    a = torch.randn((R, C), generator=g) * 3 + 10
    a[:, 2] = 7.25  # a constant column: batch variance exactly zero
    b = torch.randn((R + 2, C), generator=g) * 5 - 2
    state = ops.rms_state(C, dev)
    ops.rms_update(a.to(dev), state)
    t1, ex1 = U.rms_update_exact(U.rms_init(C), a.double().numpy())
    o1 = U.rms_update_np(U.rms_init(C), a.double().numpy())
    g1 = _state_np(state, C)
    assert np.isfinite(g1[0]).all() and np.isfinite(g1[1]).all() and g1[1][2] > 0
    for k, nm in enumerate(("mean", "var")):
        U.check64(f"constant column {nm}", g1[k], o1[k], t1[k])
    out = ops.rnd_normalize(a.to(dev), state)
    ref = U.normalize_ref(a.double().numpy(), g1[0], g1[1])
    assert bool(torch.isfinite(out).all())
    U.check("normalize constant column", out, ref.astype(np.float32), ref)
    ops.rms_update(b.to(dev), state)
    t2, _ = U.rms_update_exact(ex1, b.double().numpy())  # the exact chain of both updates
    o2 = U.rms_update_np(o1, b.double().numpy())
    g2 = _state_np(state, C)
    for k, nm in enumerate(("mean", "var")):
        U.check64(f"second update {nm}", g2[k], o2[k], t2[k])
    assert g2[2] == 1e-4 + R + R + 2


@pytest.mark.parametrize("R", [1, 65])
@pytest.mark.parametrize("D", [1, 63, 512])
def test_rnd_curiosity(dev, R, D):
    from oc_cleanrl_amd import ops

    g = torch.Generator().manual_seed(R * 1000 + D)
    p, t = torch.randn((R, D), generator=g), torch.randn((R, D), generator=g)
    got = ops.rnd_curiosity(p.to(dev), t.to(dev))
    U.check(f"curiosity {R}x{D}", got, U.curiosity_ref(p, t), U.curiosity_ref(p.double(), t.double()))


SHAPES = [(1, 1), (5, 3), (128, 2), (3, 129)]


@pytest.mark.parametrize("T,N", SHAPES)
def test_rnd_reward_norm_twice(dev, T, N):
    from oc_cleanrl_amd import ops

    g = torch.Generator().manual_seed(T * 1000 + N)
    int_gamma = 0.99
    rewems_d = torch.zeros(T, device=dev)
    state_d = torch.tensor([0.0, 1.0, 1e-4], dtype=torch.float64, device=dev)
    rewems, own_state, twin_state = None, (0.0, 1.0, 1e-4), (0.0, 1.0, 1e-4)
    for call in range(2):
        cur = torch.rand((T, N), generator=g) * 2 + 0.01
        cur_d = cur.to(dev)
        filt_d = torch.empty((N, T), device=dev)
        ops.rnd_reward_norm(cur_d, rewems_d, state_d, int_gamma, filtered=filt_d)
        per_env, rewems = U.reward_filter_np(cur.numpy(), rewems, int_gamma)
        assert per_env.dtype == np.float32
        assert np.array_equal(filt_d.cpu().numpy(), per_env), "filter output"
        assert np.array_equal(rewems_d.cpu().numpy(), rewems), "carried rewems"
        # the statistics: exact from the previous exact-chain state is not needed -- each call's
        # merge starts from the device's own previous state, as NumPy's starts from its own
        prev = tuple(float(v) for v in (twin_state if call == 0 else got_state))
        twin_state = U.reward_stats_exact(prev, per_env)
        own_state = U.reward_stats_np(prev, per_env)
        got_state = tuple(state_d.cpu().tolist())
        for k, nm in enumerate(("mean", "var", "count")):
            U.check64(f"reward_rms {T}x{N} call {call} {nm}", got_state[k], own_state[k],
                      twin_state[k])
        twin = cur.double() / np.sqrt(twin_state[1])
        f32 = cur / float(np.sqrt(own_state[1]))
        U.check(f"normalised curiosity {T}x{N} call {call}", cur_d, f32, twin)


@pytest.mark.parametrize("T,N", SHAPES)
def test_rnd_gae_is_bitwise_the_script_loop(dev, T, N):
    from oc_cleanrl_amd import ops

    g = torch.Generator().manual_seed(T * 1000 + N + 7)
    r = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    rewards, ev, cur, iv = r(T, N), r(T, N), torch.rand((T, N), generator=g), r(T, N)
    next_ext, next_int = r(N), r(N)
    dones = (torch.rand((T, N), generator=g) < 0.2).float()
    dones[0] = 1.0
    dones[T - 1, ::2] = 1.0
    next_done = torch.zeros(N)
    next_done[::2] = 1.0
    k = dict(gamma=0.999, int_gamma=0.99, gae_lambda=0.95, int_coef=1.0, ext_coef=2.0)
    want = U.gae_ref(rewards, ev, dones, next_ext, next_done, cur, iv, next_int, **k)
    d = lambda t: t.to(dev)  # noqa: E731
    got = ops.rnd_gae(d(rewards), d(ev), d(dones), d(next_ext), d(next_done), d(cur), d(iv),
                      d(next_int), **k)
    for name, a, b in zip(("ext_adv", "ext_ret", "int_adv", "int_ret", "adv"), got, want):
        assert torch.equal(a.cpu(), b), name
    adv, ret = ops.gae(d(rewards), d(ev), d(dones), d(next_ext), d(next_done), k["gamma"],
                       k["gae_lambda"])
    assert torch.equal(adv, got[0]) and torch.equal(ret, got[1])


@pytest.mark.parametrize("M", [1, 64, 65, 1000])
@pytest.mark.parametrize("D", [1, 512])
def test_rnd_aux_loss_fwd_bwd(dev, M, D):
    from oc_cleanrl_amd import ops

    g = torch.Generator().manual_seed(M * 1000 + D)
    pred, target = torch.randn((M, D), generator=g), torch.randn((M, D), generator=g)
    v, ret = torch.randn(M, generator=g), torch.randn(M, generator=g)
    seed, vf = 12345, 0.5
    counter = ops.rnd_mask_counter(dev)
    counter.fill_(3)
    for n, prop in enumerate((0.0, 0.25, 1.0)):
        want_mask = U.mask_ref(seed, 3 + n, M, prop)
        mask = ops.rnd_mask(seed, counter, M, prop)
        assert torch.equal(mask.cpu(), want_mask), "mask"
        assert int(counter) == 3 + n  # rnd_mask leaves the counter alone
        stats, dpred, dv = ops.rnd_aux_loss_fwd_bwd(pred.to(dev), target.to(dev), v.to(dev),
                                                    ret.to(dev), seed, counter, prop, vf)
        assert int(counter) == 4 + n  # one per call
        assert float(stats[2]) == float(want_mask.sum())
        if prop == 0.0:
            assert float(stats[2]) == 0 and float(stats[1]) == 0 and not bool(dpred.any())
        if prop == 1.0:
            assert float(stats[2]) == M
        s32, p32, v32 = U.aux_ref(pred, target, v, ret, want_mask, vf, torch.float32)
        s64, p64, v64 = U.aux_ref(pred, target, v, ret, want_mask, vf, torch.float64)
        U.check(f"aux stats M={M} D={D} p={prop}", stats[:2], s32[:2], s64[:2])
        U.check(f"aux dv_int M={M} D={D} p={prop}", dv, v32, v64)
        if prop > 0.0 and float(want_mask.sum()) > 0:
            U.check(f"aux dpred M={M} D={D} p={prop}", dpred, p32, p64)
        else:
            assert not bool(dpred.any())


def test_mask_counter_advances_inside_a_captured_graph(dev):
    from oc_cleanrl_amd import ops

    M, D, seed, prop = 65, 8, 99, 0.25
    g = torch.Generator().manual_seed(1)
    pred, target = (torch.randn((M, D), generator=g).to(dev) for _ in range(2))
    v, ret = (torch.randn(M, generator=g).to(dev) for _ in range(2))
    counter = ops.rnd_mask_counter(dev)
    outs = [(torch.empty(3, device=dev), torch.empty((M, D), device=dev),
             torch.empty(M, device=dev)) for _ in range(2)]

    def body():
        for st, dp, dv in outs:
            ops.rnd_aux_loss_fwd_bwd(pred, target, v, ret, seed, counter, prop, 0.5, dp, dv, st)

    body()  # warm-up (allocates the workspace), counters 0 and 1
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    k = int(counter)
    assert k == 2  # capture launches nothing
    graph.replay()
    torch.cuda.synchronize()
    assert int(counter) == k + 2
    for n, (st, dp, _) in enumerate(outs):
        kept = (dp != 0).any(dim=1).float().cpu()
        assert torch.equal(kept, U.mask_ref(seed, k + n, M, prop)), f"mask of counter {k + n}"
        assert float(st[2]) == float(kept.sum())


def test_argument_errors_arrive_before_any_launch():
    from oc_cleanrl_amd import _lib

    L, d = _lib.LIB, ctypes.c_void_p(64)
    assert L.ocppo_rms_update(None, d, 0, 4, 0, 4, d, d, 1 << 20) == _lib.OCPPO_E_INVALID
    assert b"C=0" in L.ocppo_last_error()
    assert L.ocppo_rms_update(None, d, 0, 4, 3, 4, d, d, 8) == _lib.OCPPO_E_WORKSPACE
    assert L.ocppo_rnd_gae(None, *([None] * 8), 4, 4, 0.99, 0.99, 0.95, 1.0, 2.0,
                           *([None] * 5)) == _lib.OCPPO_E_INVALID
    assert L.ocppo_rnd_aux_loss_fwd_bwd(None, d, d, d, d, 4, 4, 1, d, -0.1, 0.5, d, d, d, d,
                                        1 << 20) == _lib.OCPPO_E_INVALID
    assert b"update_proportion" in L.ocppo_last_error()
