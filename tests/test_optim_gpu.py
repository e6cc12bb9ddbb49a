"""The flat optimizer steps (csrc/ocppo_optim.hip) past their grid caps: every rule's second and
third round of the grid-stride loop (the prefetch branch), the norm pass's unrolled load slots and
its second trip, plane jobs and the segment split in a later round, the scalar tail after the loop.
Sizes and thresholds: optim_util."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import optim_util as K
import pqn_util as U
from oracle import ocppo_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from oc_cleanrl_amd import ops

    return ops


def test_sizes_cross_the_caps_of_the_source():
    """The thresholds this file is built on are the source's, and its sizes cross them."""
    c = K.source_caps()
    assert c == dict(threads=K.THREADS, norm_blocks=K.NORM_BLOCKS, norm_u=K.NORM_U,
                     adam_blocks=K.STEP_BLOCKS["ocppo_clip_adam_step"],
                     exact_blocks=K.STEP_BLOCKS["ocppo_clip_adam_step_exact"],
                     radam_is_norm_blocks=True)
    assert K.STEP_BLOCKS["ocppo_clip_radam_step"] == K.NORM_BLOCKS
    assert K.P3 == 4_194_304 + 1024 + 68 and K.P2 == 2_097_152 + 1024 + 68
    assert K.P2_RADAM == 1_048_576 + 1024 + 68
    assert K.P3 + 3 > K.NORM_TRIP  # the norm pass's second trip
    for entry, rounds3, rounds2 in (("ocppo_clip_adam_step", 3, 2),
                                    ("ocppo_clip_adam_step_exact", 3, 2),
                                    ("ocppo_clip_radam_step", 5, 3)):
        assert K.step_rounds(entry, K.P3 + 3) == rounds3
        assert K.step_rounds(entry, K.P2 + 3) == rounds2
        assert all(K.step_rounds(entry, s.stop - s.start) == 1 for s in K.chunks(K.P3 + 3))
    assert K.step_rounds("ocppo_clip_radam_step", K.P2_RADAM + 3) == 2


# ---- 1. the step is elementwise: chunking must not change it --------------------------------------
@pytest.mark.parametrize("rule", ["adam", "exact", "radam"])
def test_step_past_the_cap_is_bitwise_its_single_round_chunks(dev, rule):
    """max_norm = 0: the clip is 1 and an element's update depends on its own (p, g, m, v) and the
    step count alone. P3 + 3 elements in one call sequence (three rounds of the loop for the
    2048-workgroup rules, five for RAdam, so a thread takes the prefetch branch at least twice; a
    last round of one workgroup and 17 threads; the scalar tail after the loop) against the same
    data as chunks of at most 1,000,000 elements, each its own call sequence in a single round:
    bitwise. A skipped, doubled or mis-prefetched group shows as a mismatch."""
    entry, tail, steps, lr, eps = K.ENTRIES[rule]
    steps = 7 if rule == "radam" else 3  # RAdam: the rectified branch (from step 6) past the cap
    P = K.P3 + 3
    assert K.step_rounds(entry, P) >= 3  # thread 0 of workgroup 0 prefetches twice or more
    g = torch.Generator(device=dev).manual_seed(11)
    p0 = torch.randn(P, device=dev, generator=g)
    grads = [torch.randn(P, device=dev, generator=g) * 0.01 for _ in range(steps)]
    whole = K.run_abi(dev, entry, tail, p0, grads, lr, eps, 0.5, 0.0)
    sc = whole[3].cpu()
    assert float(sc[0]) == steps and float(sc[2]) == 1.0 and bool(torch.isfinite(sc).all())
    if rule == "radam":
        assert float(sc[5]) > 0  # the last steps were rectified
    parts = K.chunks(P)
    assert parts[-1].stop == P and (parts[-1].stop - parts[-1].start) % 4 == 3
    for s in parts:
        n = s.stop - s.start
        assert n <= K.CHUNK and s.start % 4 == 0 and K.step_rounds(entry, n) == 1
        part = K.run_abi(dev, entry, tail, p0[s], [gr[s] for gr in grads], lr, eps, 0.5, 0.0)
        for name, a, b in zip(("params", "exp_avg", "exp_avg_sq"), whole, part):
            assert torch.equal(a[s], b), (rule, name, s)
        assert float(part[3][0]) == steps
        # the chunk did move: every second moment is positive (each element was visited) and the
        # parameters are not the initial ones
        assert bool((part[2] > 0).all()) and not torch.equal(part[0], p0[s])
        assert int((part[0] != p0[s]).sum()) > n // 2


# ---- 2. the norm pass counts every element once ---------------------------------------------------
def _norm_of(dev, grad, scale=1.0, max_norm=0.0):
    P = grad.numel()
    entry, tail, _, lr, eps = K.ENTRIES["adam"]
    sc = K.run_abi(dev, entry, tail, torch.zeros(P), [grad], lr, eps, scale, max_norm)[3].cpu()
    return sc


def _marker_sets(P):
    """Two disjoint sets of 16 element positions at the ends of the norm pass's regions: group g
    (elements 4 g .. 4 g + 3) is loaded in slot g // S of trip 0 for g < 4 S, S = 1024 * 256
    groups, and in slot 0 of trip 1 from 4 S on."""
    S = K.NORM_BLOCKS * K.THREADS
    last = P // 4 - 1  # the last full group
    assert 4 * S < last < 5 * S and P % 4 == 3
    el = lambda group, lane: 4 * group + lane  # noqa: E731
    a = [0,                                    # element 0
         el(0, 3), el(S - 1, 0),               # slot 0: first and last group
         el(S, 1), el(2 * S - 1, 2),           # slot 1
         el(3 * S, 3), el(4 * S - 1, 0),       # slot 3
         el(4 * S, 1),                         # the second trip's first group
         el(last, 2),                          # the last full group
         P - 3, P - 2, P - 1,                  # the scalar tail
         el(2 * S, 0), el(3 * S - 1, 3), el(S + 12345, 2), el(4 * S + 100, 0)]
    b = [el(0, 1), el(0, 2), el(S - 1, 3),     # the other lanes / the other side of each edge
         el(S, 0), el(2 * S - 1, 3),
         el(2 * S, 3), el(3 * S - 1, 0),
         el(3 * S, 0), el(4 * S - 1, 3),
         el(4 * S, 0), el(4 * S, 3),
         el(last, 0), el(last, 3), el(last - 1, 0),
         el(K.THREADS - 1, 3), el(K.THREADS, 0)]  # a workgroup's edge
    return a, b


def test_norm_pass_markers_past_the_caps(dev):
    """A zero gradient of P3 + 3 elements with 16 ones: the sum of squares is 16 in any order,
    so total_norm is 4 exactly if each marked element is counted once."""
    P = K.P3 + 3
    a, b = _marker_sets(P)
    assert len(set(a)) == 16 and len(set(b)) == 16 and not set(a) & set(b)
    assert max(a + b) < P and min(a + b) >= 0
    for marks in (a, b):
        grad = torch.zeros(P)
        grad[marks] = 1.0
        sc = _norm_of(dev, grad)
        assert float(sc[1]) == 4.0 and float(sc[2]) == 1.0 and float(sc[0]) == 1.0


def test_norm_pass_census_past_the_caps(dev):
    """Every element counted exactly once: 16 gradients of ones on the elements i % 16 == k. The
    f32 sums are integers below 2^24, so exact; total_norm is sqrtf of the count (about 512, where
    an ulp of error is 6e-5) and its square is within 0.1 of the count, while one element missed
    or doubled moves it by 1."""
    P = K.P3 + 3
    idx = torch.arange(P)
    for k in range(16):
        mask = idx % 16 == k
        total = float(_norm_of(dev, mask.float())[1])
        assert round(total * total) == int(mask.sum()), k


def test_norm_pass_random_gradient_past_the_caps(dev):
    P, scale, max_norm = K.P3 + 3, 0.5, 0.5
    grad = torch.randn(P, generator=torch.Generator().manual_seed(3))
    sc = _norm_of(dev, grad, scale, max_norm)
    coef, total = U.clip_coef([grad.double() * scale], max_norm)
    np.testing.assert_allclose(float(sc[1]), float(total), rtol=1e-5)
    # the coefficient: max_norm / (total_norm + 1e-6) in f32 on the device's own total_norm
    # (within rtol 1e-5 of the twin's, as asserted above) plus the rounding of one f32 add and
    # one f32 divide
    assert float(coef) < 1e-3
    np.testing.assert_allclose(float(sc[2]), float(coef), rtol=1e-5 + 2 * 2.0 ** -23)
    own = np.float32(max_norm) / (np.float32(float(sc[1])) + np.float32(1e-6))
    np.testing.assert_allclose(float(sc[2]), float(own), rtol=2 * 2.0 ** -23)


# ---- 3. each rule against its twin, past the cap, with clipping active -----------------------------
def test_adam_past_the_cap_against_the_oracle(dev):
    """ocppo_clip_adam_step over P2 + 3 elements (two rounds and the scalar tail) against the
    oracle's f32 restatement, step by step, as test_clip_adam_abi_scalar_tail does."""
    entry, tail, steps, lr, eps = K.ENTRIES["adam"]
    P, scale, max_norm = K.P2 + 3, 0.5, 0.5
    assert K.step_rounds(entry, P) == 2
    p0 = torch.randn(P, generator=torch.Generator().manual_seed(P))
    grads = K.normed_grads(P, steps, seed=P + 1)
    ref = dict(p=p0.numpy(), m=np.zeros(P, np.float32), v=np.zeros(P, np.float32), step=0)
    seen = []

    def against_oracle(p, sc):
        gr = grads[ref["step"]].numpy()
        ref["p"], ref["m"], ref["v"], ref["step"], total = O.clip_adam_step(
            ref["p"], gr, ref["m"], ref["v"], ref["step"], lr, eps=eps, max_norm=max_norm,
            grad_scale=scale)
        seen.append(float(sc[2]) < 1.0)
        np.testing.assert_allclose(float(sc[1]), total, rtol=1e-5)
        np.testing.assert_allclose(p.cpu().numpy(), ref["p"], rtol=1e-6, atol=1e-9)

    K.run_abi(dev, entry, tail, p0, grads, lr, eps, scale, max_norm, against_oracle)
    assert seen == K.CLIPS[:steps]  # the clip was active where it was meant to be


@pytest.mark.parametrize("rule", ["exact", "radam"])
def test_exact_adam_and_radam_past_the_cap_against_torch(dev, rule):
    """ocppo_clip_adam_step_exact against torch.optim.Adam and ocppo_clip_radam_step against
    pqn_util.RAdamRef, two rounds and the scalar tail, by the rule of lstm_util.check against
    the f32 run and the f64 twin."""
    entry, tail, steps, lr, eps = K.ENTRIES[rule]
    P = (K.P2_RADAM if rule == "radam" else K.P2) + 3
    scale, max_norm = 0.5, 0.5
    assert K.step_rounds(entry, P) == 2
    make = K.radam_twin(lr) if rule == "radam" else K.adam_twin(lr, eps)
    p0 = torch.randn(P, generator=torch.Generator().manual_seed(P))
    grads = K.normed_grads(P, steps, seed=P + 1)
    seen = []
    got = K.run_abi(dev, entry, tail, p0, grads, lr, eps, scale, max_norm,
                    lambda p, sc: seen.append(float(sc[2]) < 1.0))
    assert seen == K.CLIPS[:steps]
    f32 = K.torch_twin(make, grads, p0, torch.float32, scale, max_norm)
    f64 = K.torch_twin(make, grads, p0, torch.float64, scale, max_norm)
    for name, a, b, c in zip(("param", "exp_avg", "exp_avg_sq"), got, f32, f64):
        U.check(f"{entry} P={P} {name}", a, b, c)
    sc = got[3].cpu()
    assert float(sc[0]) == steps and bool(torch.isfinite(sc).all())
    if rule == "radam":
        assert float(sc[5]) > 0  # the last steps were rectified


# ---- 4. plane jobs in a later round ------------------------------------------------------------------
@pytest.mark.parametrize("w1_offset", [K.ROUND + 4096, K.ROUND - 65536])
def test_adam_step_writes_the_weight_planes_in_a_later_round(ops, dev, w1_offset):
    """test_adam_step_writes_the_weight_planes behind a filler parameter: both weights wholly in
    round 2 of the step's loop, or the first one straddling the round's edge."""
    g = torch.Generator(device=dev).manual_seed(5)

    def build():
        torch.manual_seed(7)
        filler = torch.nn.Parameter(torch.randn(w1_offset).to(dev))
        lin1, lin2 = torch.nn.Linear(512, 256).to(dev), torch.nn.Linear(136, 1024).to(dev)
        ws = [filler, lin1.weight, lin2.weight]
        return ws, ops.FlatAdam(ws, lr=1e-3, eps=1e-5, max_grad_norm=0.5)

    (_, w1, w2), opt = build()
    (_, v1, v2), plain = build()  # the same step without plane jobs
    off1 = (w1.data_ptr() - opt.params.data_ptr()) // 4
    off2 = (w2.data_ptr() - opt.params.data_ptr()) // 4
    assert off1 == w1_offset and off2 == off1 + w1.numel()
    assert K.step_rounds("ocppo_clip_adam_step", opt.numel) == 2
    if w1_offset >= K.ROUND:
        assert off2 + w2.numel() <= 2 * K.ROUND  # both wholly in round 2
    else:
        assert off1 < K.ROUND < off1 + w1.numel()  # the first straddles
    p1 = torch.zeros(3, 256, 512, dtype=torch.bfloat16, device=dev)
    p2 = torch.zeros(3, 136, 1024, dtype=torch.bfloat16, device=dev)  # of W2^T
    opt.write_planes([(w1, 0, p1), (w2, 1, p2)])
    before = w1.detach().clone()
    for _ in range(2):
        gr = torch.randn(opt.numel, device=dev, generator=g)
        opt.grads.copy_(gr)
        plain.grads.copy_(gr)
        opt.step()
        plain.step()
    torch.cuda.synchronize()
    assert not torch.equal(before, w1.detach())
    assert torch.equal(p1.view(torch.int16), ops.split_planes_ref(w1.detach()).view(torch.int16))
    assert torch.equal(p2.view(torch.int16),
                       ops.split_planes_ref(w2.detach().t().contiguous()).view(torch.int16))
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(opt, k), getattr(plain, k)), k


# ---- 5. segments past the cap ------------------------------------------------------------------------
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


# the split inside round 1 with the tail running into round 2; exactly at the round's edge; inside
# round 2, one full workgroup plus 16 threads in (1000 and 30 pad to 1024 + 64)
@pytest.mark.parametrize("head_sizes,split", [((2_000_000, 67_003), 2_067_008),
                                              ((K.ROUND,), K.ROUND),
                                              ((K.ROUND, 1000, 30), K.ROUND + 1024 + 64)])
def test_flat_adam_segments_against_flat_adam_past_the_cap(ops, dev, head_sizes, split):
    """test_flat_adam_segments_against_flat_adam with the split around the edge of the step's
    first round: three steps with the tail, two without, one more with it."""
    tail_sizes = (70_000, 1)
    kw = dict(lr=1e-2, eps=1e-8, max_grad_norm=0.5)
    seg = ops.FlatAdamSegments(_params(head_sizes, dev, 1), _params(tail_sizes, dev, 2), **kw)
    ref = ops.FlatAdam(_params(head_sizes, dev, 1) + _params(tail_sizes, dev, 2), **kw)
    assert seg.numel == ref.numel and torch.equal(seg.params, ref.params)
    sp = seg.split
    assert sp == split and sp % 64 == 0
    assert K.step_rounds("ocppo_clip_adam_step_seg", seg.numel) == 2
    assert seg.numel - sp > 64 * K.THREADS * 4  # the tail spans workgroups (68 of them)
    if sp < K.ROUND:
        assert seg.numel > K.ROUND  # the tail runs into round 2
    live = _live(seg)
    keys = ("params", "exp_avg", "exp_avg_sq")

    def grads(s):
        g = torch.Generator().manual_seed(500 + s)
        return (torch.randn(seg.numel, generator=g) * live).to(dev)

    for s in range(3):  # the tail active: bitwise FlatAdam on the same gradients
        gr = grads(s)
        seg.grads.copy_(gr)
        ref.grads.copy_(gr)
        seg.step(True)
        ref.step()
        for k in keys:
            assert torch.equal(getattr(seg, k), getattr(ref, k)), (k, s)
        assert torch.equal(seg.scalars[:5], ref.scalars[:5])
    assert float(seg.scalars[ops.OPT_TAIL_STEP]) == 3 and float(seg.tail_step) == 3
    # the tail inactive (its gradients garbage here, zero there): the head bitwise FlatAdam over
    # the whole buffer, the tail's parameters, moments and count bit-unchanged
    before = {k: getattr(seg, k)[sp:].clone() for k in keys}
    assert all(bool(before[k].any()) for k in keys)
    for s in range(3, 5):
        gr = grads(s)
        seg.grads.copy_(gr)  # the tail's gradients are left as they come: they must not be read
        gr[sp:] = 0
        ref.grads.copy_(gr)
        seg.step(False)
        ref.step()
        for k in keys:
            assert torch.equal(getattr(seg, k)[:sp], getattr(ref, k)[:sp]), (k, s)
            assert torch.equal(getattr(seg, k)[sp:], before[k]), (k, s)
        assert torch.equal(seg.scalars[:5], ref.scalars[:5])
        assert float(seg.scalars[ops.OPT_TAIL_STEP]) == 3 and float(seg.tail_step) == 3
    assert float(seg.scalars[ops.OPT_STEP]) == 5
    assert float(seg.scalars[ops.OPT_TAIL_SKIPPED]) == 2
    # one more step with the tail: the head is FlatAdam's step 6; the tail is FlatAdam's step 4
    # from the tail's own state (ref's tail moved on zero gradients meanwhile), under the same
    # clip, since the norm is the same sum over the same gradients
    ref4 = ops.FlatAdam(_params(head_sizes, dev, 1) + _params(tail_sizes, dev, 2), **kw)
    for k in keys:
        getattr(ref4, k).copy_(getattr(seg, k))
    ref4.scalars[ops.OPT_STEP] = 3.0
    gr = grads(5)
    for o in (seg, ref, ref4):
        o.grads.copy_(gr)
    seg.step(True)
    ref.step()
    ref4.step()
    for k in keys:
        assert torch.equal(getattr(seg, k)[:sp], getattr(ref, k)[:sp]), k
        assert torch.equal(getattr(seg, k)[sp:], getattr(ref4, k)[sp:]), k
        assert not torch.equal(getattr(seg, k)[sp:], before[k]), k
    assert torch.equal(seg.scalars[:5], ref.scalars[:5])
    assert float(ref4.scalars[ops.OPT_STEP]) == 4
    assert torch.equal(seg.scalars[1:3], ref4.scalars[1:3])  # the same norm and clip
    assert float(seg.scalars[ops.OPT_STEP]) == 6
    assert float(seg.scalars[ops.OPT_TAIL_SKIPPED]) == 2
    assert float(seg.scalars[ops.OPT_TAIL_STEP]) == 4 and float(seg.tail_step) == 4
