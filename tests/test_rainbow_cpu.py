"""Rainbow surface without a GPU: the Args dataclass and both networks against fixtures made from
the reference (tests/golden/gen_golden_rainbow.py), and rainbow_util's restatement of the replay
and of the loss block against every fixture (this validates the oracle the GPU tests use)."""
import dataclasses
import json

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from rainbow_util import (ADDSEQ_FIXTURES, CHECKED, F32_FLOOR, LOSS_FIXTURES, SAMPLE_FIXTURES,
                          PerOracle, bounds, check_elementwise, fixture, per_weights, rel_err,
                          restated, retrieve, strata, tree_is_consistent)


def test_args_fields_and_defaults_match_reference():
    from oc_cleanrl_amd.rainbow import RainbowArgs

    ref = json.loads((GOLDEN / "rainbow_args_fields.json").read_text())
    mine = {f.name: f.default for f in dataclasses.fields(RainbowArgs)}
    assert [n for n, _ in ref] == list(mine)[:len(ref)]  # same names, same order, ours after
    for name, default in ref:
        if name == "backend":  # ALE / OCAtari are not available: declared difference
            assert mine[name] == "Synthetic" and default == "HackAtari"
            continue
        got = list(mine[name]) if isinstance(mine[name], tuple) else mine[name]
        assert got == default, name
    assert mine["vecnorm_reward"] is False and mine["cuda_graphs"] is True
    a = RainbowArgs()
    assert (a.n_step, a.n_atoms, a.learning_rate, a.seed) == (3, 51, 0.0000625, 1)


def _seeded_net(kind):
    from oc_cleanrl_amd.rainbow import (NoisyDuelingDistributionalNetwork,
                                        NoisyDuelingDistributionalPPObj)

    z = fixture(f"rainbow_init_{kind}")
    torch.manual_seed(int(z["seed"]))
    A, N = int(z["n_actions"]), int(z["n_atoms"])
    if kind == "pixels":
        net = NoisyDuelingDistributionalNetwork((4, 84, 84), A, N, -10, 10)
    else:
        net = NoisyDuelingDistributionalPPObj(
            (4, 12), A, N, -10, 10, encoder_dims=tuple(int(v) for v in z["encoder_dims"]),
            decoder_dims=tuple(int(v) for v in z["decoder_dims"]))
    return net, z


@pytest.mark.parametrize("kind", ["obj", "pixels"])
def test_network_layout_seeded_init_and_forward(kind):
    net, z = _seeded_net(kind)
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in z["keys"]]  # same keys, same order, noise buffers included
    assert torch.equal(sd["support"], torch.from_numpy(z["support"]))  # bitwise
    assert net.delta_z == float(z["delta_z"])
    for (k, v), shape, (s, sa) in zip(sd.items(), z["shapes"], z["sums"]):
        assert list(v.shape) == json.loads(str(shape)), k
        np.testing.assert_allclose(float(v.double().sum()), s, rtol=1e-5, atol=1e-5, err_msg=k)
        np.testing.assert_allclose(float(v.double().abs().sum()), sa, rtol=1e-6, err_msg=k)
    with torch.no_grad():
        q_dist = net(torch.from_numpy(z["x"]))
    assert q_dist.shape == z["q_dist"].shape
    np.testing.assert_allclose(q_dist.numpy(), z["q_dist"], rtol=1e-5, atol=1e-7)
    net.reset_noise()  # new noise moves the output; eval() switches it off
    with torch.no_grad():
        assert not torch.equal(net(torch.from_numpy(z["x"])), q_dist)


# ---- the replay oracle against the fixtures -------------------------------------------------------
def replay_fixture_oracle(z):
    return PerOracle(int(z["capacity"]), z["obs"].shape[2:], int(z["n_step"]), float(z["gamma"]),
                     float(z["alpha"]), float(z["eps"]))


def updates_after(z):
    """{add index: update number} of an add-sequence fixture."""
    return {int(z[f"upd{j}_after_add"]): j for j in range(int(z["n_updates"]))}


@pytest.mark.parametrize("name", ADDSEQ_FIXTURES)
def test_oracle_reproduces_add_sequences(name):
    z = fixture(f"per_addseq_{name}")
    rb = replay_fixture_oracle(z)
    assert np.array_equal(z["gamma_pows"], [rb.gamma ** i for i in range(rb.n_step)])
    upd = updates_after(z)
    for t in range(len(z["pos"])):
        rb.add(z["in_obs"][t], z["in_action"][t], z["in_reward"][t], z["in_next_obs"][t],
               z["in_done"][t])
        for mine, key in ((rb.obs, "obs"), (rb.next_obs, "next_obs"), (rb.actions, "actions"),
                          (rb.rewards, "rewards"), (rb.dones, "dones"), (rb.tree, "tree")):
            assert np.array_equal(mine, z[key][t]), (key, t)  # bitwise
        assert (rb.pos, rb.size) == (int(z["pos"][t]), int(z["size"][t]))
        assert f32_bits(rb.max_priority) == f32_bits(z["max_priority"][t])
        if t in upd:
            j = upd[t]
            rb.update_priorities(z[f"upd{j}_indices"], z[f"upd{j}_priorities"])
            assert np.array_equal(rb.tree, z[f"upd{j}_tree"]), j  # bitwise, duplicates included
            assert f32_bits(rb.max_priority) == f32_bits(z[f"upd{j}_max_priority"])
            assert tree_is_consistent(rb.tree, rb.capacity)
            idx = z[f"upd{j}_indices"]
            last = {int(i): k for k, i in enumerate(idx)}  # the last occurrence wins
            keep = sorted(last.values())
            check_elementwise(rb.leaves()[idx[keep]], rb.leaves()[idx[keep]],
                              z[f"upd{j}_leaf64"][keep], "leaf")


def f32_bits(x) -> int:
    return int(np.asarray(x, np.float32).view(np.uint32))


@pytest.mark.parametrize("name", SAMPLE_FIXTURES)
def test_oracle_reproduces_samples(name):
    z = fixture(f"per_sample_{name}")
    C, B, tree, size = int(z["capacity"]), int(z["B"]), z["buf_tree"], int(z["buf_size"])
    assert tree_is_consistent(tree, C)
    lo, hi = strata(tree[0], B)
    assert np.array_equal(lo, z["seg_lo"]) and np.array_equal(hi, z["seg_hi"])  # bitwise f32
    ub = z["upperbounds"]
    assert ((ub >= lo) & (ub < hi)).all()
    idx = np.array([retrieve(tree, C, u) for u in ub])
    for j in (0, 1):
        assert np.array_equal(idx, z[f"b{j}_indices"])
        probs, w = per_weights(tree, C, size, idx, float(z[f"b{j}_beta"]))
        assert np.array_equal(probs, z[f"b{j}_probs"])
        check_elementwise(w, z[f"b{j}_weights"], z[f"b{j}_weights64"], "weights")
        assert np.array_equal(z["buf_obs"][idx], z[f"b{j}_obs"])
        assert np.array_equal(z["buf_next_obs"][idx], z[f"b{j}_next_obs"])
        assert np.array_equal(z["buf_rewards"][idx], z[f"b{j}_rewards"])


# ---- the loss oracle against the fixtures ---------------------------------------------------------
@pytest.mark.parametrize("name", LOSS_FIXTURES)
def test_restated_loss_reproduces_fixture(name):
    z = fixture(f"rainbow_loss_{name}")
    r32, r64 = restated(z, torch.float32), restated(z, torch.float64)
    assert np.array_equal(r32["best_actions"], z["best_actions"])
    assert np.array_equal(r64["best_actions"], z["best_actions"])
    lim = bounds(z)
    for k in CHECKED:
        assert rel_err(r64[k], z[k + "64"]) <= 1e-12, k  # the twin itself
        assert rel_err(r32[k], z[k + "64"]) <= lim[k][0], (k, lim[k])
    assert np.isfinite(z["dadvantage"]).all() and (z["weights"] > 0).all()
    assert z["weights"].max() == 1.0


def test_edges_fixture_covers_the_projection_branches():
    z = fixture("rainbow_loss_edges")
    assert z["dones"].any() and not z["dones"].all()
    N, v_min, v_max = z["support"].shape[0], float(z["v_min"]), float(z["v_max"])
    gamma_n = np.float32(float(z["gamma"]) ** int(z["n_step"]))
    tz = np.clip(z["rewards"][:, None] + gamma_n * z["support"] * (1 - z["dones"][:, None]),
                 np.float32(v_min), np.float32(v_max))
    b = (tz - np.float32(v_min)) / np.float32((v_max - v_min) / (N - 1))
    assert (tz == v_min).any() and (tz == v_max).any()
    assert ((np.floor(b) == b) & (tz > v_min) & (tz < v_max)).any()  # the (l == b) branch
    assert F32_FLOOR == 4 * 2.0 ** -23
