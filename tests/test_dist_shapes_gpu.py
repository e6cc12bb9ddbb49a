"""The C51 and Rainbow kernels (ocppo_distributional.h) at their atom, action and batch boundaries:
N = 2, 63, 64, 65, 127, 128 (a lane holds atoms `lane` and `lane + 64`), A with a partial batch of
the greedy scan's 6 actions after a full one, B with a partial last round of the loss workgroup's 16
waves, stored actions outside [0, A), and ties / NaN in the third action batch.

Inputs are c51_util / rainbow_util's seeded cases; both references run on the CPU: the f32
restatement and its f64 twin on the SAME f32 projected index b (projected_index says why), so the
rule is the suite's own: a tensor's error against the twin, relative to the twin's largest element,
is at most max(3 x the f32 reference's own error, 4 * 2^-23) (dist_util.bound). Every case is
checked by dist_util.assert_case before it is launched (test_dist_shapes_cpu.py does the same
without a GPU)."""
import numpy as np
import pytest
import torch

import c51_util
import rainbow_util
from dist_util import (ACT_SHAPES, CLAMP_SHAPE, F32_FLOOR, LOSS_SHAPES, assert_act_case,
                       assert_case, bound, rel_err, row_rel_err)

pytestmark = pytest.mark.gpu
GRAPH_SHAPE = (17, 13, 65)  # a partial last round: idle waves still reach both barriers
NAN = float("nan")


# ---- launchers: every output NaN-filled (actions -1), so every element must be written -----------
def on_device(z, dev, actions=None):
    """The arrays of case `z` as device tensors, `actions` in place of the case's own."""
    t = {k: torch.from_numpy(v).to(dev) for k, v in z.items() if isinstance(v, np.ndarray)}
    if actions is not None:
        t["actions"] = torch.from_numpy(actions).to(dev)
    return t


def c51_loss(t, z, outs=None):
    from oc_cleanrl_amd import ops

    if outs is None:
        B, N = t["logits"].shape[0], t["atoms"].numel()
        full = lambda *s: torch.full(s, NAN, device=t["logits"].device)  # noqa: E731
        outs = dict(dlogits=full(*t["logits"].shape), stats=full(2), target_pmfs=full(B, N),
                    next_action=torch.full_like(t["actions"], -1))
    ops.c51_loss_fwd_bwd(*[t[k] for k in ("logits", "logits_next", "atoms", "actions", "rewards",
                                          "dones")],
                         float(z["gamma"]), float(z["v_min"]), float(z["v_max"]), **outs)
    return outs


def rainbow_loss(t, z, outs=None):
    from oc_cleanrl_amd import ops

    if outs is None:
        (B, N), AN = t["value"].shape, t["advantage"].shape[1]
        full = lambda *s: torch.full(s, NAN, device=t["value"].device)  # noqa: E731
        outs = dict(dvalue=full(B, N), dadvantage=full(B, AN), loss_per_sample=full(B),
                    stats=full(2), target_pmfs=full(B, N),
                    best_actions=torch.full_like(t["actions"], -1))
    ops.rainbow_loss_fwd_bwd(*[t[k] for k in rainbow_util.HEADS + ("support", "actions", "rewards",
                                                                   "dones", "weights")],
                             float(z["gamma"]) ** int(z["n_step"]), float(z["v_min"]),
                             float(z["v_max"]), **outs)
    return outs


LEARNERS = {"c51": (c51_util, c51_loss, "next_action"),
            "rainbow": (rainbow_util, rainbow_loss, "best_actions")}


def as_numpy(outs):
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in outs.items()}
    return dict(o, loss=o["stats"][0], q_values=o["stats"][1])


def check_against_twin(tag, got, c, checked):
    """The rule for every checked tensor, and for target_pmfs also per row (relative to that
    row's largest twin element: a wrong upper-half atom in one row cannot hide behind another
    row's peak). A tensor whose twin is identically zero must be exactly zero."""
    r32, r64 = c["r32"], c["r64"]
    report, failed = [], []
    for k in checked:
        if not np.isfinite(got[k]).all():
            failed.append((k, "not finite"))
        elif not np.any(r64[k]):
            report.append(f"{k} exact 0")
            if np.any(got[k]):
                failed.append((k, "twin is identically zero", float(np.abs(got[k]).max())))
        else:
            (lim, own), err = bound(r32[k], r64[k]), rel_err(got[k], r64[k])
            report.append(f"{k} {err:.2g} / {own:.2g}")
            if not err <= lim:
                failed.append((k, err, own, lim))
    if np.isfinite(got["target_pmfs"]).all():
        err = row_rel_err(got["target_pmfs"], r64["target_pmfs"])
        own = row_rel_err(r32["target_pmfs"], r64["target_pmfs"])
        lim = np.maximum(3 * own, F32_FLOOR)
        i = int(np.argmax(err - lim))
        report.append(f"target_pmfs rows {err.max():.2g} / {own.max():.2g}")
        if not (err <= lim).all():
            failed.append(("target_pmfs row", i, float(err[i]), float(own[i]), float(lim[i])))
    print(f"{tag}: error vs f64 / the f32 reference's own: " + ", ".join(report))
    assert not failed, failed


# ---- 2. the loss kernels at the boundary shapes --------------------------------------------------
@pytest.mark.parametrize("learner", LEARNERS)
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=str)
def test_loss_kernel_at_boundary_shape(dev, learner, shape):
    util, launch, action_key = LEARNERS[learner]
    c = util.loss_case(*shape)
    assert_case(c, util.CHECKED, action_key)
    z, (B, A, N) = c["z"], shape
    t = on_device(z, dev)
    outs = launch(t, z)
    got = as_numpy(outs)
    assert np.array_equal(got[action_key], c["r64"][action_key])
    check_against_twin(f"{learner} {shape}", got, c, util.CHECKED)
    if learner == "c51":  # rows of the actions not taken: exactly zero
        taken = np.zeros((B, A), bool)
        taken[np.arange(B), z["actions"]] = True
        assert (got["dlogits"].reshape(B, A, N)[~taken] == 0).all()
    elif A == 1:  # advantage - its own mean: no gradient reaches it
        assert (got["dadvantage"] == 0).all()
    again = launch(t, z)  # a second launch is bitwise the first
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], again[k]), k
    if shape == GRAPH_SHAPE:  # and so is a replayed graph
        replayed = {k: torch.zeros_like(v) for k, v in outs.items()}
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            launch(t, z, outs=replayed)
        for _ in range(2):  # stats are rewritten, not accumulated
            g.replay()
        torch.cuda.synchronize()
        for k in outs:
            assert torch.equal(outs[k], replayed[k]), k


# ---- 3. stored actions outside [0, A) ------------------------------------------------------------
@pytest.mark.parametrize("learner", LEARNERS)
def test_out_of_range_actions_read_the_nearest_row(dev, learner):
    """clamp_action: a stored action of -1 / A gives bitwise the launch with 0 / A - 1. The two
    rows are inner ones (1 and 3 of 5), where the rows next to the taken action's are still the
    tensor's own."""
    util, launch, action_key = LEARNERS[learner]
    B, A, N = CLAMP_SHAPE
    c = util.loss_case(B, A, N)
    assert_case(c, util.CHECKED, action_key)
    outside, nearest = c["z"]["actions"].copy(), c["z"]["actions"].copy()
    outside[1], outside[3] = -1, A
    nearest[1], nearest[3] = 0, A - 1
    z = c["z"]
    a, b = launch(on_device(z, dev, outside), z), launch(on_device(z, dev, nearest), z)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
        assert torch.isfinite(a[k]).all() if a[k].is_floating_point() else (a[k] >= 0).all(), k


# ---- 4. the acting kernels -----------------------------------------------------------------------
def c51_act(logits, atoms, dev):
    """ops.c51_epsilon_greedy at epsilon 0: (actions, q) on the CPU, q NaN-filled before."""
    from oc_cleanrl_amd import ops

    E, A = logits.shape[0], logits.shape[1] // atoms.numel()
    q = torch.full((E, A), NAN, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    act = ops.c51_epsilon_greedy(logits.to(dev), atoms.to(dev), 11, step, 0.0, 0.0, 100.0, q_out=q)
    return act.cpu(), q.cpu()


def rainbow_act(value, advantage, support, dev):
    from oc_cleanrl_amd import ops

    E, A = value.shape[0], advantage.shape[1] // support.numel()
    q = torch.full((E, A), NAN, device=dev)
    act = ops.rainbow_greedy(value.to(dev), advantage.to(dev), support.to(dev), q_out=q)
    return act.cpu(), q.cpu()


def check_acting(tag, act, q, c):
    lim, own = bound(c["q32"], c["q64"])
    err = rel_err(q.numpy(), c["q64"])
    print(f"{tag}: q error vs f64 {err:.2g}, torch f32's own {own:.2g}")
    assert torch.isfinite(q).all() and err <= lim, (err, own, lim)
    assert torch.equal(act, torch.argmax(q, 1))
    assert np.array_equal(act.numpy(), c["q64"].argmax(1))  # assert_act_case: no near-tie


@pytest.mark.parametrize("shape", ACT_SHAPES, ids=str)
def test_c51_acting_at_boundary_shape(dev, shape):
    c = c51_util.act_case(*shape)
    assert_act_case(c)
    act, q = c51_act(c["logits"], c["atoms"], dev)
    check_acting(f"c51 q {shape}", act, q, c)


@pytest.mark.parametrize("shape", ACT_SHAPES, ids=str)
def test_rainbow_acting_at_boundary_shape(dev, shape):
    c = rainbow_util.act_case(*shape)
    assert_act_case(c)
    act, q = rainbow_act(c["value"], c["advantage"], c["support"], dev)
    check_acting(f"rainbow q {shape}", act, q, c)
    torch.testing.assert_close(q, torch.from_numpy(c["q32"]), rtol=1e-5, atol=1e-5)


# pinned cases at A = 13: actions 12 and 8 sit in the greedy scan's third and second batch
PIN = (4, 13, 65)


def _tied(rows):
    """[E, A, N] rows with action 3 copied into action 12, both with their mass on the top atom:
    the shared maximum of the expected value."""
    rows = rows.clone()
    rows[:, 3, -1] += 20.0
    rows[:, 12] = rows[:, 3]
    return rows


def test_c51_acting_tie_in_the_third_batch_takes_the_lower_index(dev):
    E, A, N = PIN
    c = c51_util.act_case(E, A, N)
    act, q = c51_act(_tied(c["logits"].view(E, A, N)).view(E, A * N), c["atoms"], dev)
    assert torch.equal(q[:, 3], q[:, 12])  # bitwise: the same chain in either batch
    assert (q[:, 3:4] > torch.cat((q[:, :3], q[:, 4:12]), 1)).all()
    assert act.tolist() == [3] * E


def test_rainbow_acting_tie_in_the_third_batch_takes_the_lower_index(dev):
    E, A, N = PIN
    c = rainbow_util.act_case(E, A, N)
    adv = _tied(c["advantage"].view(E, A, N)).view(E, A * N)
    act, q = rainbow_act(c["value"], adv, c["support"], dev)
    assert torch.equal(q[:, 3], q[:, 12])
    assert (q[:, 3:4] > torch.cat((q[:, :3], q[:, 4:12]), 1)).all()
    assert act.tolist() == [3] * E


def test_c51_acting_nan_beats_every_number(dev):
    """c51_better's rule is torch.argmax's: a NaN expected value beats every number, and the
    first one is kept."""
    E, A, N = PIN
    c = c51_util.act_case(E, A, N)
    logits = c["logits"].clone().view(E, A, N)
    logits[:, 8, 5] = NAN
    act, q = c51_act(logits.view(E, A * N), c["atoms"], dev)
    assert torch.isnan(q[:, 8]).all() and int(torch.isnan(q).sum()) == E
    assert act.tolist() == [8] * E and torch.equal(act, torch.argmax(q, 1))


def test_rainbow_acting_nan_takes_the_first(dev):
    """One NaN advantage reaches every action of its row through the dueling mean: every
    expected value is NaN and the first is kept, as torch.argmax does on the same q."""
    E, A, N = PIN
    c = rainbow_util.act_case(E, A, N)
    adv = c["advantage"].clone().view(E, A, N)
    adv[:, 8, 5] = NAN
    act, q = rainbow_act(c["value"], adv.view(E, A * N), c["support"], dev)
    assert torch.isnan(q).all()
    assert act.tolist() == [0] * E and torch.equal(act, torch.argmax(q, 1))
