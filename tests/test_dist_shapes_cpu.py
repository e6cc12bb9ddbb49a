"""The generated C51 / Rainbow cases of test_dist_shapes_gpu.py without a GPU: every shape of the
sweep satisfies dist_util.assert_case (same action in the f32 restatement and the twin, no near-tie
of expected values, the f32 reference's own error at most 64 * 2^-23, the edge rows present), the
shared f32 projected index is the one the f32 restatement forms itself, and the plain float64 run
is NOT a usable twin for Rainbow."""
import numpy as np
import pytest
import torch

import c51_util
import rainbow_util
from dist_util import (ACT_SHAPES, CLAMP_SHAPE, LOSS_SHAPES, OWN_MAX, assert_act_case, assert_case,
                       own_error)

LEARNERS = {"c51": (c51_util, "next_action"), "rainbow": (rainbow_util, "best_actions")}


@pytest.mark.parametrize("learner", LEARNERS)
@pytest.mark.parametrize("shape", LOSS_SHAPES + (CLAMP_SHAPE,), ids=str)
def test_generated_case_conditions(learner, shape):
    util, action_key = LEARNERS[learner]
    c = util.loss_case(*shape)
    assert_case(c, util.CHECKED, action_key)
    z, (B, A, N) = c["z"], shape
    assert z["rewards"].shape == (B,) and z["support"].shape == (N,)
    assert z["actions"].min() >= 0 and z["actions"].max() < A
    worst = {k: own_error(c["r32"][k], c["r64"][k]) for k in util.CHECKED}
    print(f"{learner} {shape}: the f32 reference's own error: "
          + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))
    # b= changes nothing in f32: the shared index is the one the restatement forms itself
    plain = util.restated(z, torch.float32)
    for k, v in c["r32"].items():
        assert np.array_equal(v, plain[k]), k
    if learner == "rainbow":
        assert z["weights"].max() == 1.0 and z["weights"].min() >= 0.05


@pytest.mark.parametrize("learner", LEARNERS)
@pytest.mark.parametrize("shape", ACT_SHAPES, ids=str)
def test_generated_acting_case_conditions(learner, shape):
    c = LEARNERS[learner][0].act_case(*shape)
    assert_act_case(c)
    assert c["q64"].shape == shape[:2] and c["q32"].dtype == np.float32


def test_plain_float64_run_is_no_twin_for_rainbow():
    """Why the twin takes the f32 index: at a clamped row f32 gives b == N - 1 exactly, f64 on the
    f32-rounded delta_z gives N - 1 + eps, and (l == b) then drops that row's whole mass."""
    c = rainbow_util.loss_case(49, 11, 128)
    plain64 = rainbow_util.restated(c["z"], torch.float64)
    assert own_error(c["r32"]["target_pmfs"], plain64["target_pmfs"]) > 0.5
    assert own_error(c["r32"]["target_pmfs"], c["r64"]["target_pmfs"]) <= OWN_MAX
