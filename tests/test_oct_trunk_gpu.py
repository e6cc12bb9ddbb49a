"""ops.oct_trunk (csrc/ocppo_oct_trunk.hip): the object-set transformer agent's whole trunk, inference
forward, as one launch -- against the float64 twin (transformer_util.agent_ref) under the project's
error rule with torch's own f32 modules on the GPU as the yardstick, its routing in
OCTransformerAgent.trunk, and the trainer's rollout on it. Run with -s for the (measured / torch's
own) pairs."""
import pytest
import torch

import transformer_util as tu
from test_transformer_gpu import _state, _trainer

pytestmark = pytest.mark.gpu

NUM_OBJ = 3


def _agent(dev, S, F, E, heads, blocks, post, masking, pooling, dropout=0.0):
    """A real agent with seeded parameters; LayerNorm weights / biases and every Linear bias moved
    away from their 1 / 0 initial values so that they matter."""
    from oc_cleanrl_amd.agents import EnvSpec
    from oc_cleanrl_amd.transformer import OCTransformerAgent

    torch.manual_seed(E + S)
    ag = OCTransformerAgent(EnvSpec((S, F), 4), E, heads, blocks, masking, NUM_OBJ, None,
                            pooling_type=pooling, num_post_layers=post, dropout=dropout)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for k, p in ag.named_parameters():
            if "norm" in k or k.endswith("bias"):
                p.add_(0.3 * torch.randn(p.shape, generator=gen))
    return ag.to(dev).train()


def _inputs(B, S, F, mask, seed=0):
    """Unit-scale object sets whose type columns say which objects exist (make_masks)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, F, generator=gen)
    valid = tu.make_masks(mask, B, S, gen)
    typ = torch.nn.functional.one_hot(torch.randint(0, NUM_OBJ, (B, S), generator=gen), NUM_OBJ)
    x[..., :NUM_OBJ] = typ if valid is None else typ * valid[..., None]
    return x, valid


def _three(ag, x, dev, monkeypatch, tile=0):
    """(kernel, torch's own f32 modules on the GPU, the f64 twin on the CPU) hidden of x."""
    from oc_cleanrl_amd import ops
    from oc_cleanrl_amd import transformer as T

    layers = ag.transformer.layers
    with torch.no_grad():
        got = ops.oct_trunk(x.to(dev), ag.encoder, layers, list(ag.network)[::2], ag.num_heads,
                            ag.masking, NUM_OBJ, ag.pooling_type, tile)
        monkeypatch.setattr(T, "FUSED_ATTN", False)
        own = ag.trunk(x.to(dev))
        monkeypatch.setattr(T, "FUSED_ATTN", True)
    p = {k: v.detach().double().cpu() for k, v in ag.state_dict().items()}
    twin = tu.agent_ref(x.double(), p, heads=ag.num_heads, blocks=len(layers),
                        post=len(ag.network) // 2, num_obj=NUM_OBJ, masking=ag.masking,
                        pooling_type=ag.pooling_type)[0]
    return got, own, twin


# E, heads, S, B, F, blocks, post, mask ("none": masking off), pooling, tile rows (0: the rule)
CASES = [
    (32, 4, 1, 1, 8, 1, 0, "tail", "max", 0),
    (32, 4, 5, 3, 11, 1, 2, "hole", "mean", 64),   # fewer samples than the workgroup holds
    (32, 4, 16, 67, 8, 3, 2, "tail", "first", 32),  # two samples per tile, ragged last workgroup
    (32, 4, 17, 3, 11, 1, 0, "one", "max", 0),
    (32, 4, 64, 3, 8, 1, 2, "tail", "mean", 0),
    (64, 1, 5, 67, 8, 1, 2, "none", "max", 0),
    (64, 1, 16, 1, 11, 3, 0, "none", "mean", 0),
    (64, 1, 17, 67, 8, 1, 0, "hole", "first", 0),
    (64, 1, 64, 1, 11, 1, 2, "one", "mean", 0),
    (64, 1, 1, 67, 8, 1, 2, "none", "first", 0),
    (128, 8, 1, 3, 11, 1, 0, "tail", "mean", 0),
    (128, 8, 5, 67, 11, 3, 2, "tail", "max", 64),  # 12 samples per tile, 7 in the last
    (128, 8, 16, 3, 8, 1, 2, "hole", "max", 0),
    (128, 8, 17, 1, 8, 1, 2, "tail", "mean", 0),
    (128, 8, 64, 3, 11, 3, 0, "none", "max", 0),
    (128, 8, 8, 67, 8, 3, 1, "one", "first", 64),
]


@pytest.mark.parametrize("E,heads,S,B,F,blocks,post,mask,pooling,tile", CASES)
def test_trunk_matches_f64_twin(dev, monkeypatch, E, heads, S, B, F, blocks, post, mask, pooling,
                                tile):
    ag = _agent(dev, S, F, E, heads, blocks, post, mask != "none", pooling)
    x, _ = _inputs(B, S, F, mask)
    got, own, twin = _three(ag, x, dev, monkeypatch, tile)
    assert got.shape == (B, E)
    tu.check(f"E{E} h{heads} S{S} B{B} F{F} L{blocks} P{post} {mask} {pooling} hidden", got, own,
             twin)


def test_invalid_tokens_do_not_leak(dev, monkeypatch):
    """One sample twice, the second time with large finite values in the excluded objects' other
    features: under masked attention and `first` pooling (row 0 is valid) they change nothing."""
    S, F = 5, 11
    ag = _agent(dev, S, F, 32, 4, 2, 1, True, "first")
    x, valid = _inputs(1, S, F, "tail", seed=3)
    if valid.all():
        valid[0, -2:] = False
        x[0, -2:, :NUM_OBJ] = 0
    loud = x.clone()
    loud[0, ~valid[0], NUM_OBJ:] = 1e4
    both = torch.cat([x, loud])
    got, own, twin = _three(ag, both, dev, monkeypatch)
    for i in range(2):
        tu.check(f"sample {i} hidden", got[i], own[i], twin[i])
    e = tu.rel_err(got[1], got[0])
    print(f"loud against quiet: {e:.3g}")
    assert e <= tu.FLOOR


def test_agent_routes_under_no_grad_only(dev, monkeypatch):
    from oc_cleanrl_amd import ops
    from oc_cleanrl_amd import transformer as T

    # the default routing: the measured sizes only (S <= 16, 80 .. 65,536 token rows)
    assert all(ops.oct_trunk_routed(B, S) for B, S in ((10, 8), (128, 16), (4096, 16)))
    assert not any(ops.oct_trunk_routed(B, S) for B, S in ((4, 6), (10, 64), (3, 32), (8192, 16)))
    calls = {"trunk": 0, "mha": 0}
    trunk, mha = ops.oct_trunk, ops.mha
    monkeypatch.setattr(ops, "oct_trunk_routed", lambda B, S: True)
    monkeypatch.setattr(ops, "oct_trunk", lambda *a, **k: (
        calls.__setitem__("trunk", calls["trunk"] + 1), trunk(*a, **k))[1])
    monkeypatch.setattr(ops, "mha", lambda *a: (calls.__setitem__("mha", calls["mha"] + 1),
                                                mha(*a))[1])
    ag = _agent(dev, 6, 8, 32, 4, 2, 1, True, "max")
    x = _inputs(4, 6, 8, "tail")[0].to(dev)
    with torch.no_grad():
        h = ag.trunk(x)
    assert calls == {"trunk": 1, "mha": 0}
    h2 = ag.trunk(x)  # an autograd graph is wanted: the chain, as before
    assert calls == {"trunk": 1, "mha": 2} and h2.requires_grad
    assert tu.rel_err(h, h2.detach()) < 1e-4
    with torch.no_grad():
        monkeypatch.setattr(T, "FUSED_ATTN", False)
        ag.trunk(x)
        monkeypatch.setattr(T, "FUSED_ATTN", True)
        _agent(dev, 6, 8, 32, 4, 2, 1, True, "max", dropout=0.1).trunk(x)
        monkeypatch.setattr(T, "FUSED_TRUNK", False)
        ag.trunk(x)
    assert calls == {"trunk": 1, "mha": 4}


def test_trainer_rollout_on_the_kernel(dev, monkeypatch):
    """The trainer's policy step runs the kernel (routing forced on) and agrees with the f64 twin
    on its own net_obs; two captured iterations are bitwise two eager ones."""
    from oc_cleanrl_amd import ops

    calls = []
    trunk = ops.oct_trunk
    monkeypatch.setattr(ops, "oct_trunk_routed", lambda B, S: True)
    monkeypatch.setattr(ops, "oct_trunk", lambda *a, **k: (calls.append(1), trunk(*a, **k))[1])
    runs = []
    for graphs in (True, False):
        tr = _trainer(dev, cuda_graphs=graphs)
        for _ in range(3):
            tr.train_iteration(collect_metrics=False)
        torch.cuda.synchronize()
        assert tr.graphs_ready == graphs and calls
        runs.append(_state(tr))
        if not graphs:
            ag, a = tr.agent, tr.args
            with torch.no_grad():
                n = len(calls)
                got = tr._policy_hidden(0)
                assert len(calls) == n + 1
            x = tr.net_obs.detach().cpu()
            monkeypatch.setattr(ops, "oct_trunk_routed", lambda B, S: False)
            with torch.no_grad():
                own = ag.trunk(tr.net_obs)
            p = {k: v.detach().double().cpu() for k, v in ag.state_dict().items()}
            twin = tu.agent_ref(x.double(), p, heads=a.num_heads, blocks=a.num_blocks,
                                post=a.num_post_layers, num_obj=a.num_obj, masking=a.masking,
                                pooling_type=a.pooling_type)[0]
            tu.check("policy hidden", got, own, twin)
        tr.close()
    assert all(torch.equal(x, y) for x, y in zip(*runs))
