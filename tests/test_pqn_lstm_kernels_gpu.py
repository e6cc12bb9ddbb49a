"""ocppo_pqn_lstm_act and ocppo_pqn_head_loss_fwd_bwd (csrc/ocppo_pqn_lstm.hip) on the GPU: the
act kernel bitwise against the two entries it fuses, the head-loss kernel's exact structure, and
its values against an f64 twin under a bound measured from the composed f32 path."""
from __future__ import annotations

import ctypes
import re

import pytest
import torch
import torch.nn.functional as F

import pqn_lstm_util as U
from conftest import ROOT

pytestmark = pytest.mark.gpu

CSRC = ROOT / "oc_cleanrl_amd" / "csrc"
# the kernels' own geometry, read from their sources
STEP_ENVS = int(re.search(r"constexpr int kStepEnvs = (\d+);",
                          (CSRC / "ocppo_lstm_step.h").read_text()).group(1))
HL_ROWS = int(re.search(r"constexpr int kHlRows = (\d+);",
                        (CSRC / "ocppo_pqn_lstm.hip").read_text()).group(1))
SEED, DUR = 1234, 1000.0
EXPLORE, GREEDY = (1.0, 1.0), (0.0, 0.0)  # (start_e, end_e): epsilon above / below every coin


def _bits(t):
    return t.contiguous().view(torch.int32)


def _act_case(dev, H, A, I, N, ties=False):
    g = torch.Generator().manual_seed(1000 * H + 10 * A + I)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    c = dict(x=r(N, I), w_ih=0.3 * r(4 * H, I), b_ih=0.1 * r(4 * H), w_hh=0.3 * r(4 * H, H),
             b_hh=0.1 * r(4 * H), h=r(N, H), c=r(N, H), wq=r(A, H), bq=r(A))
    c["done"] = (torch.arange(N) % 2).float()  # mixed 0 / 1 (a lone env: 0)
    if ties and A >= 3:  # rows 0 and 2 of the head equal: q ties there for every env
        c["wq"][2], c["bq"][2] = c["wq"][0], c["bq"][0]
    c = {k: v.to(dev).contiguous() for k, v in c.items()}
    c["step"] = torch.tensor([40], dtype=torch.int64, device=dev)
    return c


def _composed(ops, c, eps):
    """ops.lstm_step, then ops.pqn_act on the new h."""
    h, cc = c["h"].clone(), c["c"].clone()
    ops.lstm_step(c["x"], c["w_ih"], c["b_ih"], c["w_hh"], c["b_hh"], c["done"], h, cc)
    N, A = h.shape[0], c["wq"].shape[0]
    q = torch.full((N, A), -7.0, device=h.device)
    e = torch.full((1,), -1.0, device=h.device)
    a, v = ops.pqn_act(h, c["wq"], c["bq"], SEED, c["step"], *eps, DUR, epsilon_out=e,
                       step_offset=8, q_out=q)
    return dict(h=h, c=cc, actions=a, values=v, q=q, eps=e)


def _fused(ops, c, eps, commit=True):
    h, cc = c["h"].clone(), c["c"].clone()
    N, A = h.shape[0], c["wq"].shape[0]
    q = torch.full((N, A), -7.0, device=h.device)
    e = torch.full((1,), -1.0, device=h.device)
    a, v = ops.pqn_lstm_act(c["x"], c["w_ih"], c["b_ih"], c["w_hh"], c["b_hh"], c["done"], h, cc,
                            c["wq"], c["bq"], SEED, c["step"], *eps, DUR, epsilon_out=e,
                            step_offset=8, q_out=q, commit=commit)
    return dict(h=h, c=cc, actions=a, values=v, q=q, eps=e)


@pytest.mark.parametrize("I", [1, 5, 512])
@pytest.mark.parametrize("A", [1, 6, 18])
@pytest.mark.parametrize("H", [32, 64, 128])
def test_act_is_bitwise_lstm_step_then_pqn_act(dev, H, A, I):
    """commit = 1 at N in {1, 3, a workgroup's environments + 1}, mixed dones, a nonzero incoming
    state, epsilon above and below the coin: every output bitwise the composed pair's; two runs
    agree; row n does not change when N grows; commit = 0 leaves h / c untouched and writes the
    same q / values."""
    from oc_cleanrl_amd import ops

    NS = (1, 3, STEP_ENVS + 1)
    big = _act_case(dev, H, A, I, NS[-1])
    prev = None
    for N in reversed(NS):
        c = {k: (v if k in ("w_ih", "b_ih", "w_hh", "b_hh", "wq", "bq", "step") else
                 v[:N].contiguous()) for k, v in big.items()}
        assert ops.pqn_lstm_act_ok(c["x"], c["h"], c["wq"])
        for eps in (EXPLORE, GREEDY):
            want, got = _composed(ops, c, eps), _fused(ops, c, eps)
            for k in ("h", "c", "values", "q", "eps"):
                assert torch.equal(_bits(got[k]), _bits(want[k])), (k, N, eps)
            assert torch.equal(got["actions"], want["actions"]), (N, eps)
            assert float(got["eps"]) == eps[0]
            again = _fused(ops, c, eps)
            for k in got:
                assert torch.equal(got[k], again[k]), (k, N)
        assert not torch.equal(got["h"], c["h"])  # the state moved
        if prev is not None:  # row n of the larger batch
            for k in ("h", "c", "values", "q", "actions"):
                assert torch.equal(got[k], prev[k][:N]), (k, N)
        prev = got
        dry = _fused(ops, c, GREEDY, commit=False)
        assert dry["actions"] is None
        assert torch.equal(_bits(dry["h"]), _bits(c["h"]))
        assert torch.equal(_bits(dry["c"]), _bits(c["c"]))
        assert torch.equal(_bits(dry["q"]), _bits(got["q"]))
        assert torch.equal(_bits(dry["values"]), _bits(got["values"]))


@pytest.mark.parametrize("H", [32, 128])
def test_act_ties_resolve_to_the_lowest_index(dev, H):
    from oc_cleanrl_amd import ops

    c = _act_case(dev, H, 6, 5, STEP_ENVS + 1, ties=True)
    got = _fused(ops, c, GREEDY)
    q = got["q"].cpu()
    assert torch.equal(q[:, 0], q[:, 2])
    first = (q == q.max(1, keepdim=True).values).float().argmax(1)  # first index of the maximum
    assert torch.equal(got["actions"].cpu(), first)
    assert torch.equal(got["values"].cpu(), q.max(1).values)
    assert not bool((got["actions"] == 2).any())
    # all rows equal: every q ties, action 0
    c["wq"][:] = c["wq"][0]
    c["bq"][:] = c["bq"][0]
    assert not bool(_fused(ops, c, GREEDY)["actions"].any())


def test_act_contract(dev):
    from oc_cleanrl_amd import _lib, ops

    f = lambda *s: torch.zeros(*s, device=dev)  # noqa: E731
    assert ops.pqn_lstm_act_ok(f(3, 5), f(3, 64), f(6, 64))
    assert not ops.pqn_lstm_act_ok(f(3, 5), f(3, 48), f(6, 48))
    assert not ops.pqn_lstm_act_ok(f(3, 5), f(3, 64), f(0, 64))
    assert not ops.pqn_lstm_act_ok(f(3, 5), f(3, 64), f(19, 64))
    assert not ops.pqn_lstm_act_ok(f(3, 5), f(2, 64), f(6, 64))
    L = _lib.LIB
    x, w_ih, b, w_hh, done = f(3, 5), f(256, 5), f(256), f(256, 64), f(3)
    h, c, wq, bq, v = f(3, 64), f(3, 64), f(18, 64), f(18), f(3)
    acts = torch.zeros(3, dtype=torch.int64, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def raw(N=3, H=64, A=6, hp=p(h)):
        return L.ocppo_pqn_lstm_act(None, p(x), p(w_ih), p(b), p(w_hh), p(b), p(done), N, 5, H,
                                    hp, p(c), 1, p(wq), p(bq), A, 0, p(step), 0, 1.0, 0.1, 10.0,
                                    p(acts), p(v), None, None)

    for kw in (dict(H=48), dict(A=0), dict(A=19), dict(hp=None)):
        assert raw(**kw) == _lib.OCPPO_E_INVALID, kw
    assert raw(N=0) == _lib.OCPPO_OK
    torch.cuda.synchronize()
    assert not bool(h.any()) and not bool(acts.any())  # nothing ran


# ---- the update's head + loss ---------------------------------------------------------------
def _hl_case(dev, M, H, A, seed=0):
    g = torch.Generator().manual_seed(seed + 7 * M + 13 * H + A)
    h = torch.randn(M, H, generator=g)
    wq = torch.randn(A, H, generator=g) / H ** 0.5
    bq = 0.1 * torch.randn(A, generator=g)
    # the highest action is never taken (A > 1)
    actions = torch.randint(0, max(A - 1, 1), (M,), generator=g)
    returns = torch.randn(M, generator=g)
    return tuple(t.to(dev).contiguous() for t in (h, wq, bq, actions, returns))


HL_GRID = [(M, H, A) for H in (4, 128, 1024) for A in (1, 2, 18)
           for M in sorted({1, 67, 2 * HL_ROWS + 3})]


@pytest.mark.parametrize("M,H,A", HL_GRID)
def test_head_loss_structure_is_exact(dev, M, H, A):
    """Rows of dwq / dbq of an action nobody took are bitwise zero; dh[m] == g_m * wq[a_m] in f32
    with g_m recomputed from the kernel's own q_a (the workspace's first M floats); two runs are
    bitwise equal; an out-of-range action behaves as the clamped one."""
    from oc_cleanrl_amd import ops

    h, wq, bq, actions, returns = _hl_case(dev, M, H, A)
    assert ops.pqn_head_loss_ok(h, wq)
    ws = ops.HeadLossWorkspace(M, H, A, dev)
    junk = lambda *s: torch.full(s, 3.5, device=dev)  # noqa: E731  (outputs are overwritten)
    stats, dh, dwq, dbq = ops.pqn_head_loss_fwd_bwd(h, wq, bq, actions, returns, junk(M, H),
                                                    junk(A, H), junk(A), junk(2), ws)
    q_a = ws.q_taken.clone()
    taken = set(actions.tolist())
    for a in range(A):
        if a not in taken:
            assert not bool(_bits(dwq[a]).any()) and not bool(_bits(dbq[a:a + 1]).any()), a
    assert A == 1 or (A - 1) not in taken
    g = (q_a - returns) * torch.tensor(2.0 / M, dtype=torch.float32, device=dev)
    assert torch.equal(dh, g.unsqueeze(1) * wq[actions])
    assert torch.isfinite(stats).all() and torch.isfinite(dwq).all()
    stats2, dh2, dwq2, dbq2 = ops.pqn_head_loss_fwd_bwd(h, wq, bq, actions, returns,
                                                        workspace=ws)
    for a_, b_ in ((stats, stats2), (dh, dh2), (dwq, dwq2), (dbq, dbq2)):
        assert torch.equal(_bits(a_), _bits(b_))
    wild = actions.clone()
    wild[0] = -3
    wild[-1] = A + 5
    clamped = wild.clamp(0, A - 1)
    got = ops.pqn_head_loss_fwd_bwd(h, wq, bq, wild, returns, workspace=ws)
    want = ops.pqn_head_loss_fwd_bwd(h, wq, bq, clamped, returns)
    for a_, b_ in zip(got, want):
        assert torch.equal(_bits(a_), _bits(b_))


def _abs_err(a, twin):
    return float((a.detach().double().cpu() - twin).abs().max())


@pytest.mark.parametrize("M,H,A", HL_GRID)
def test_head_loss_values_within_twice_the_composed_paths_error(dev, M, H, A):
    """Against the f64 twin (pqn_lstm_util.head_loss_ref: Linear -> one-hot masked sum ->
    mse_loss -> autograd): per output, the kernel's largest absolute error is at most 2 x the
    largest absolute error of the composed f32 path on the same inputs (F.linear +
    ops.pqn_loss_fwd_bwd + autograd, the parent's code). The factor 2 is for the different
    summation order over M and H; nothing else is allowed for.

    Bound used: 2 x the composed path's error of the same case and output, nothing added.
    Measured on the MI355X, largest absolute error over the grid's cases, kernel / composed, and
    the worst per-case ratio: loss 9.7e-8 / 8.0e-6 (1.00), mean q_a 5.9e-8 /
    1.8e-6 (1.00), dh 1.8e-7 / 3.6e-7 (1.85), dwq 6.7e-7 / 1.1e-5 (1.00), dbq 1.2e-7 / 3.3e-6
    (1.00). The kernel accumulates its sums in f64 and rounds once, so every output but dh is the
    nearest f32 to the exact result; dh's factor is f32 arithmetic on the rounded q_a (the
    structure test above needs that), and its 1.85 is a one-ulp difference.
    """
    from oc_cleanrl_amd import ops

    h, wq, bq, actions, returns = _hl_case(dev, M, H, A, seed=1)
    twin = U.head_loss_ref(h, wq, bq, actions, returns, torch.float64)
    stats, dh, dwq, dbq = ops.pqn_head_loss_fwd_bwd(h, wq, bq, actions, returns)
    got = dict(loss=stats[0], q_mean=stats[1], dh=dh, dwq=dwq, dbq=dbq)
    hh, ww, bb = (t.clone().requires_grad_() for t in (h, wq, bq))
    q = F.linear(hh, ww, bb)
    cstats, dq = ops.pqn_loss_fwd_bwd(q.detach(), actions, returns)
    torch.autograd.backward(q, dq)
    comp = dict(loss=cstats[0], q_mean=cstats[1], dh=hh.grad, dwq=ww.grad, dbq=bb.grad)
    fails = []
    for k in got:
        e, own = _abs_err(got[k], twin[k]), _abs_err(comp[k], twin[k])
        print(f"head_loss M={M} H={H} A={A} {k}: kernel {e:.3g} composed {own:.3g} "
              f"bound {2 * own:.3g}")
        if not e <= 2 * own:
            fails.append((k, e, own))
    assert not fails, fails
