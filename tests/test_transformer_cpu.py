"""The object-set transformer learner without a GPU: the flag surface, the agent's module layout
and seeded init against fixtures made from the reference (tests/golden/gen_golden_transformer.py),
the plain-torch restatement of a block (tests/transformer_util.py) against the same fixtures, and
the fused path's gate."""
import dataclasses
import json

import numpy as np
import pytest
import torch

import transformer_util as tu
from conftest import GOLDEN, golden

FIXTURES = ("e32_max", "e128_mean", "e32_first_nomask")


def test_args_fields_and_defaults_match_reference():
    from oc_cleanrl_amd.transformer import TransformerArgs

    ref = json.loads((GOLDEN / "transformer_args_fields.json").read_text())
    mine = {f.name: f.default for f in dataclasses.fields(TransformerArgs)}
    assert [n for n, _ in ref] == list(mine)[:len(ref)]  # same names, same order, ours after
    declared = {"backend": ("Synthetic", 0),  # ALE / OCAtari are not available
                "obs_mode": ("obj", "ori"),   # this package's name of object-vector observations
                "seed": (42, None)}           # the script draws a random seed per run
    for name, default in ref:
        if name in declared:
            assert (mine[name], default) == declared[name], name
            continue
        assert mine[name] == default, name
    a = TransformerArgs()
    assert (a.emb_dim, a.num_heads, a.num_blocks, a.dropout) == (128, 8, 3, 0.1)
    assert (a.pooling_type, a.num_post_layers, a.masking) == ("max", 1, True)
    assert "num_obj" in mine and "cuda_graphs" in mine and "encoder_dims" not in mine


def _agent(z, dropout=0.0):
    from oc_cleanrl_amd.agents import EnvSpec
    from oc_cleanrl_amd.transformer import OCTransformerAgent

    torch.manual_seed(int(z["seed"]))
    return OCTransformerAgent(EnvSpec((int(z["S"]), int(z["F"])), int(z["n_actions"])),
                              int(z["emb_dim"]), int(z["num_heads"]), int(z["num_blocks"]),
                              bool(z["masking"]), int(z["num_obj"]), None,
                              pooling_type=str(z["pooling_type"]),
                              num_post_layers=int(z["num_post_layers"]), dropout=dropout)


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_keys_and_seeded_init_match_reference(name):
    z = golden(f"transformer_{name}.npz")
    sd = _agent(z).state_dict()
    assert list(sd) == [str(k) for k in z["keys"]]
    for k, v in sd.items():
        assert np.array_equal(v.numpy(), z["p:" + k]), k
    assert any(k == "transformer.layers.0.self_attn.in_proj_weight" for k in sd)


@pytest.mark.parametrize("name", FIXTURES)
def test_agent_on_torch_modules_matches_reference(name):
    """On the CPU the agent runs torch's own layer modules: the reference's numbers."""
    z = golden(f"transformer_{name}.npz")
    ag = _agent(z).train()
    x = torch.from_numpy(z["x"])
    hidden = ag.trunk(x)
    logits, value = ag.heads(hidden)
    loss = (logits * torch.from_numpy(z["wl"])).sum() + (value * torch.from_numpy(z["wv"])).sum()
    loss.backward()
    np.testing.assert_allclose(hidden.detach().numpy(), z["hidden"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(logits.detach().numpy(), z["logits"], rtol=0, atol=1e-6)
    for k, p in ag.named_parameters():
        if "g:" + k in z:
            np.testing.assert_allclose(p.grad.numpy(), z["g:" + k], rtol=0,
                                       atol=2e-6 * np.abs(z["g:" + k]).max(), err_msg=k)
        else:
            assert p.grad is None and not bool(z["masking"]), k


@pytest.mark.parametrize("name", FIXTURES)
def test_restated_block_and_pooling_match_fixtures(name):
    """tests/transformer_util.py in f64 on the f32 weights is the fixtures' f64 twin (to f64
    rounding), in f32 it obeys the error rule against that twin."""
    z, z64 = golden(f"transformer_{name}.npz"), golden(f"transformer_{name}_f64.npz")
    cfg = tu.fixture_cfg(z)
    for dtype in (torch.float64, torch.float32):
        p = tu.fixture_params(z, dtype, grad=True)
        x = torch.from_numpy(z["x"]).to(dtype)
        hidden, logits, value, steps = tu.agent_ref(x, p, **cfg)
        loss = (logits * torch.from_numpy(z["wl"]).to(dtype)).sum() + \
            (value * torch.from_numpy(z["wv"]).to(dtype)).sum()
        loss.backward()
        got = {"enc": steps[0], "hidden": hidden, "logits": logits, "value": value,
               **{f"block{i}": s for i, s in enumerate(steps[1:])},
               **{"g:" + k: v.grad for k, v in p.items() if v.grad is not None}}
        assert {k for k in z64 if k.startswith("g:")} == {k for k in got if k.startswith("g:")}
        for k, v in got.items():
            if dtype == torch.float64:
                assert tu.rel_err(v.detach(), z64[k]) < 1e-12, k
            else:
                tu.check(f"{name} {k}", v.detach(), z[k], z64[k])


def test_pooling_variants_restate_the_reference_quirks():
    from oc_cleanrl_amd.transformer import pool

    h = torch.tensor([[[1.0, -2.0], [3.0, -1.0], [5.0, -0.5]]])
    mask = torch.tensor([[True, True, False]])
    # max: multiplied by the mask first, so a padded row competes as 0
    assert pool(h, mask, "max").tolist() == [[3.0, 0.0]]
    # mean: ALL rows summed, divided by the number of valid ones
    assert pool(h, mask, "mean").tolist() == [[4.5, -1.75]]
    assert pool(h, mask, "first").tolist() == [[1.0, -2.0]]
    assert pool(h, None, "max").tolist() == [[5.0, -0.5]]
    assert torch.allclose(pool(h, None, "mean"), h.mean(1))
    for kind in ("max", "mean", "first"):
        assert torch.equal(pool(h, mask, kind), tu.pool_ref(h, mask, kind))


def test_attn_ok_gates_the_fused_path():
    from oc_cleanrl_amd import transformer as T

    assert T.attn_shape_ok(6, 128, 8, 0.0) and T.attn_shape_ok(64, 512, 8, 0.0)
    assert not T.attn_shape_ok(6, 128, 8, 0.1)   # dropout > 0: torch's modules
    assert not T.attn_shape_ok(65, 128, 8, 0.0)  # S = 65
    assert not T.attn_shape_ok(6, 32, 8, 0.0)    # head dim 4
    assert not T.attn_shape_ok(6, 1024, 16, 0.0)  # E > 512
    assert not T.attn_ok(torch.zeros(2, 6, 8), 128, 8, 0.0)  # a CPU tensor
    assert T.TransformerArgs().dropout == 0.1  # the reference's default selects the torch path
