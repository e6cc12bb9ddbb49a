"""Counter-based dropout on the GPU (csrc/ocppo_attn.hip): ops.dropout bitwise
against the numpy mask of tests/dropout_util.py, ops.mha with dropout on the probabilities against
a float64 twin that multiplies the numpy mask in (the project's error rule: at most
max(3 x torch's own f32 error on the same ops with the same explicit mask, 4 * 2^-23) of the twin's
largest element), repeatability, the agent's fused path with dropout in train() and eval(),
hipGraph replay, and the trainer. Run with -s for the (measured / torch's own) pairs; the worst
ones are in DESIGN.md 13."""
import math

import numpy as np
import pytest
import torch

import dropout_util as du
import transformer_util as tu
from conftest import golden

pytestmark = pytest.mark.gpu

SEED = 1234
PS = (0.1, 0.5)


def _rng(dev, offset=0, seed=SEED):
    from oc_cleanrl_amd import ops

    return ops.philox_state(seed, dev, offset)


def _scaled_mask(keep, p, dtype):
    """keep * 1 / (1 - p): the f32-rounded scale the kernels use for f32, the double for f64."""
    s = float(du.scale_f32(p)) if dtype == torch.float32 else 1.0 / (1.0 - p)
    return torch.from_numpy(keep).to(dtype) * s


# ---- ops.dropout --------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 257, 320 * 8 * 128])
def test_dropout_forward_is_the_numpy_mask_bitwise(dev, n, p):
    from oc_cleanrl_amd import ops

    offset, site = 3, 5
    rng = _rng(dev, offset)
    want = du.keep_elementwise(SEED, offset, site, n, p).astype(np.float32) * du.scale_f32(p)
    y = ops.dropout(torch.ones(n, device=dev), rng, site, p)
    assert np.array_equal(y.cpu().numpy(), want)
    # a pointer that is not 16-B aligned, on either side: the same words, element by element
    x1 = torch.ones(n + 1, device=dev)[1:]
    assert x1.data_ptr() % 16 == 4
    assert np.array_equal(ops.dropout(x1, rng, site, p).cpu().numpy(), want)
    buf = torch.full((n + 2,), -7.0, device=dev)
    ops.dropout_fwd(torch.ones(n, device=dev), rng, site, p, out=buf[1:n + 1])
    assert np.array_equal(buf[1:n + 1].cpu().numpy(), want)
    assert float(buf[0]) == -7.0 and float(buf[n + 1]) == -7.0
    assert torch.equal(rng.cpu(), torch.tensor([SEED, offset]))  # a launch reads the state only


def test_dropout_sites_and_offsets_are_different_masks(dev):
    from oc_cleanrl_amd import ops

    n, p = 4096, 0.5
    x = torch.ones(n, device=dev)
    got = {}
    for offset, site in ((0, 0), (0, 1), (1, 0), (2, 255)):
        got[offset, site] = ops.dropout(x, _rng(dev, offset), site, p).cpu().numpy()
        want = du.keep_elementwise(SEED, offset, site, n, p).astype(np.float32) * np.float32(2)
        assert np.array_equal(got[offset, site], want)
    keys = list(got)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert not np.array_equal(got[a], got[b]), (a, b)


def test_dropout_p0_returns_its_input_and_bad_arguments_raise(dev):
    from oc_cleanrl_amd import _lib, ops

    x = torch.ones(8, device=dev)
    assert ops.dropout(x, None, 0, 0.0) is x
    rng = _rng(dev)
    for p in (-0.1, 1.0):
        with pytest.raises(ValueError, match="not in"):
            ops.dropout(x, rng, 0, p)
    for site in (-1, 256):
        with pytest.raises(ValueError, match="site"):
            ops.dropout(x, rng, site, 0.1)
    with pytest.raises(ValueError, match="rng"):
        ops.dropout(x, None, 0, 0.1)
    with pytest.raises(ValueError, match="dtype"):
        ops.dropout(x, rng.float(), 0, 0.1)
    L = _lib.LIB
    assert L.ocppo_dropout(None, x.data_ptr(), rng.data_ptr(), 256, 1, 1.5, 8, x.data_ptr() + 64) \
        == _lib.OCPPO_E_INVALID
    assert L.ocppo_dropout(None, x.data_ptr(), rng.data_ptr(), 0, 1, 1.5, 8, x.data_ptr()) \
        == _lib.OCPPO_E_INVALID  # in place
    assert L.ocppo_dropout(None, x.data_ptr(), None, 0, 1, 1.5, 8, None) == _lib.OCPPO_E_INVALID
    assert L.ocppo_philox_advance(None, None) == _lib.OCPPO_E_INVALID


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n", [5, 257])
def test_dropout_backward_reads_the_forwards_state(dev, n, p):
    """dx = dy * scale * mask bitwise, with the live generator state advanced between the forward
    and the backward: the backward reads the tensor the forward was given."""
    from oc_cleanrl_amd import ops

    offset, site = 6, 9
    live = _rng(dev, offset)
    snap = live.clone()
    x = torch.randn(n, device=dev, requires_grad=True)
    y = ops.dropout(x, snap, site, p)
    ops.philox_advance(live)
    assert torch.equal(live.cpu(), torch.tensor([SEED, offset + 1]))
    dy = torch.arange(n, dtype=torch.float32, device=dev)
    y.backward(dy)
    keep = du.keep_elementwise(SEED, offset, site, n, p)
    want = np.where(keep, np.arange(n, dtype=np.float32) * du.scale_f32(p), np.float32(0))
    assert np.array_equal(x.grad.cpu().numpy(), want)
    assert np.array_equal(y.detach().cpu().numpy(),
                          np.where(keep, x.detach().cpu().numpy() * du.scale_f32(p), np.float32(0)))
    assert not np.array_equal(keep, du.keep_elementwise(SEED, offset + 1, site, n, p))


# ---- ops.mha with dropout -----------------------------------------------------------------------
def _mha_case(dev, B, S, heads, dh, kind, seed):
    gen = torch.Generator().manual_seed(seed)
    E = heads * dh
    qkv = torch.randn(B, S, 3 * E, generator=gen)
    dout = torch.randn(B, S, E, generator=gen)
    mask = tu.make_masks(kind, B, S, gen)
    return qkv.to(dev), dout.to(dev), None if mask is None else mask.to(dev)


def mha_drop_ref(qkv, key_valid, heads: int, m):
    """tu.mha_ref with the explicit mask m [B, heads, S, S] = keep * scale multiplied into the
    probabilities."""
    B, S, E3 = qkv.shape
    E = E3 // 3
    dh = E // heads
    q, k, v = (t.reshape(B, S, heads, dh).transpose(1, 2) for t in qkv.split(E, dim=2))
    s = q @ k.transpose(-1, -2) / math.sqrt(dh)
    if key_valid is not None:
        s = s.masked_fill(~key_valid.bool()[:, None, None, :], float("-inf"))
    return ((torch.softmax(s, dim=-1) * m) @ v).transpose(1, 2).reshape(B, S, E)


def _drop_ref(qkv, dout, mask, heads, keep, p, dtype):
    q = qkv.detach().to(dtype).clone().requires_grad_(True)
    out = mha_drop_ref(q, mask, heads, _scaled_mask(keep, p, dtype).to(qkv.device))
    out.backward(dout.to(dtype))
    return out.detach(), q.grad


def test_mha_p0_with_rng_is_mha_without_it(dev):
    from oc_cleanrl_amd import ops

    qkv, dout, mask = _mha_case(dev, 3, 17, 8, 16, "tail", seed=2)
    kv = mask.to(torch.uint8)
    outs = []
    for extra in ((), (_rng(dev, 4), 7, 0.0)):
        q = qkv.clone().requires_grad_(True)
        out = ops.mha(q, kv, 8, *extra)
        out.backward(dout)
        outs.append((out.detach(), q.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    with pytest.raises(ValueError, match="not in"):
        ops.mha(qkv, kv, 8, _rng(dev), 0, 1.0)
    with pytest.raises(ValueError, match="rng"):
        ops.mha(qkv, kv, 8, None, 0, 0.1)


HEADS = [(8, 16), (4, 8), (16, 32), (1, 64)]


@pytest.mark.parametrize("S", [1, 4, 5, 16, 17, 64])
@pytest.mark.parametrize("heads,dh", HEADS)
def test_mha_dropout_matches_f64_twin(dev, S, heads, dh):
    from oc_cleanrl_amd import ops

    assert ops.mha_dropout_shape_ok(S, heads * dh, heads)  # dh = 64 is in the dropout contract
    worst = {"out": (0.0, 0.0), "dqkv": (0.0, 0.0)}
    for B in (1, 3):
        for kind in ("none", "tail", "one"):
            for p in PS:
                offset, site = B + 1, 4 * (S % 3)
                qkv, dout, mask = _mha_case(dev, B, S, heads, dh, kind, seed=S * 131 + B)
                kv = None if mask is None else mask.to(torch.uint8)
                keep = du.keep_attention(SEED, offset, site, B, heads, S, p)
                q = qkv.clone().requires_grad_(True)
                out = ops.mha(q, kv, heads, _rng(dev, offset), site, p)
                out.backward(dout)
                o32, g32 = _drop_ref(qkv, dout, mask, heads, keep, p, torch.float32)
                o64, g64 = _drop_ref(qkv, dout, mask, heads, keep, p, torch.float64)
                tag = f"mha B{B} S{S} h{heads} dh{dh} {kind} p{p}"
                for name, got, f32, twin in (("out", out.detach(), o32, o64),
                                             ("dqkv", q.grad, g32, g64)):
                    e, own = tu.rel_err(got, twin), tu.rel_err(f32, twin)
                    worst[name] = max(worst[name], (e, own))
                    assert e <= tu.bound(own), (tag, name, e, own)
                if mask is not None:  # excluded keys: dK and dV exactly 0
                    E = heads * dh
                    dk, dv = q.grad[..., E:2 * E], q.grad[..., 2 * E:]
                    assert not dk[~mask].any() and not dv[~mask].any(), tag
    print(f"mha dropout S{S} h{heads} dh{dh}: out {worst['out'][0]:.3g} / {worst['out'][1]:.3g}, "
          f"dqkv {worst['dqkv'][0]:.3g} / {worst['dqkv'][1]:.3g}")


def test_mha_dropout_repeatable_and_lse_unchanged(dev):
    from oc_cleanrl_amd import ops

    B, S, heads, dh, p = 67, 17, 8, 16, 0.1
    qkv, dout, mask = _mha_case(dev, B, S, heads, dh, "tail", seed=9)
    kv = mask.to(torch.uint8)
    rng = _rng(dev, 5)

    def run(r, site):
        out, lse = ops.mha_dropout_fwd(qkv, kv, heads, r, site, p)
        return out, lse, ops.mha_dropout_bwd(qkv, kv, out, lse, dout, heads, r, site, p)

    a, b = run(rng, 8), run(rng.clone(), 8)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = run(rng, 4)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[2], c[2])
    assert torch.equal(a[1], c[1]) and torch.equal(a[1], ops.mha_fwd(qkv, kv, heads)[1])
    E = heads * dh
    assert not a[2][..., E:2 * E][~mask].any() and not a[2][..., 2 * E:][~mask].any()


def test_mha_query_row_with_every_key_dropped_is_zero(dev):
    """p = 0.5, S = 4: a (sample, head, query) whose four keys are all dropped (found with the
    numpy restatement) yields an exactly-zero output row and finite gradients."""
    from oc_cleanrl_amd import ops

    B, S, heads, dh, p, site = 3, 4, 8, 16, 0.5, 0
    for offset in range(64):
        keep = du.keep_attention(SEED, offset, site, B, heads, S, p)
        dead = np.argwhere(~keep.any(-1))
        if len(dead):
            break
    assert len(dead), "no fully dropped row in 64 offsets"
    qkv, dout, _ = _mha_case(dev, B, S, heads, dh, "none", seed=11)
    q = qkv.clone().requires_grad_(True)
    out = ops.mha(q, None, heads, _rng(dev, offset), site, p)
    out.backward(dout)
    assert torch.isfinite(out).all() and torch.isfinite(q.grad).all()
    for b, h, i in dead:
        assert not out[b, i, h * dh:(h + 1) * dh].any(), (b, h, i)
    o64, g64 = _drop_ref(qkv, dout, None, heads, keep, p, torch.float64)
    o32, g32 = _drop_ref(qkv, dout, None, heads, keep, p, torch.float32)
    tu.check("dead row out", out.detach(), o32, o64)
    tu.check("dead row dqkv", q.grad, g32, g64)


# ---- the agent ----------------------------------------------------------------------------------
FIXTURE = "transformer_e32_max.npz"
P_AGENT = 0.1


def _agent(z, dev, dropout, fused_dropout=False, seed=SEED):
    from oc_cleanrl_amd.agents import EnvSpec
    from oc_cleanrl_amd.transformer import OCTransformerAgent

    ag = OCTransformerAgent(EnvSpec((int(z["S"]), int(z["F"])), int(z["n_actions"])),
                            int(z["emb_dim"]), int(z["num_heads"]), int(z["num_blocks"]),
                            bool(z["masking"]), int(z["num_obj"]), None,
                            pooling_type=str(z["pooling_type"]),
                            num_post_layers=int(z["num_post_layers"]), dropout=dropout,
                            fused_dropout=fused_dropout, seed=seed)
    ag.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("p:")})
    return ag.to(dev).train()


def _loss_backward(ag, z, dev):
    x = torch.from_numpy(z["x"]).to(dev)
    hidden = ag.trunk(x)
    logits, value = ag.heads(hidden)
    loss = (logits * torch.from_numpy(z["wl"]).to(dev)).sum() + \
        (value * torch.from_numpy(z["wv"]).to(dev)).sum()
    ag.zero_grad()
    loss.backward()
    return hidden.detach(), logits.detach(), value.detach()


def _block_drop_ref(x, prm, prefix, heads, key_valid, masks, eps=1e-5):
    """tu.block_ref with the four explicit dropout masks (keep * scale) of one layer."""
    g = lambda k: prm[prefix + k]  # noqa: E731
    B, S, E = x.shape
    qkv = x @ g("self_attn.in_proj_weight").T + g("self_attn.in_proj_bias")
    a = mha_drop_ref(qkv, key_valid, heads, masks[0]) @ g("self_attn.out_proj.weight").T + \
        g("self_attn.out_proj.bias")
    x = tu.add_layernorm_ref(x, a * masks[1].view(B, S, E), g("norm1.weight"), g("norm1.bias"), eps)
    f = torch.relu(x @ g("linear1.weight").T + g("linear1.bias")) * masks[2].view(B, S, -1)
    f = f @ g("linear2.weight").T + g("linear2.bias")
    return tu.add_layernorm_ref(x, f * masks[3].view(B, S, E), g("norm2.weight"), g("norm2.bias"),
                                eps)


def _agent_drop_ref(z, dtype, offset, p=P_AGENT, seed=SEED):
    """(hidden, logits, value, grads) of the agent on the fixture's input with the numpy masks of
    every site at generator offset `offset`: tu.agent_ref's steps around _block_drop_ref."""
    cfg = tu.fixture_cfg(z)
    prm = tu.fixture_params(z, dtype, grad=True)
    x = torch.from_numpy(z["x"]).to(dtype)
    B, S, _ = x.shape
    E, H = int(z["emb_dim"]), cfg["heads"]
    dff = prm["transformer.layers.0.linear1.weight"].shape[0]
    mask = (x[..., :cfg["num_obj"]] != 0).any(-1) if cfg["masking"] else None
    h = x @ prm["encoder.weight"].T + prm["encoder.bias"]
    for i in range(cfg["blocks"]):
        masks = [_scaled_mask(du.keep_attention(seed, offset, 4 * i, B, H, S, p), p, dtype)]
        for k, n in ((1, B * S * E), (2, B * S * dff), (3, B * S * E)):
            masks.append(_scaled_mask(du.keep_elementwise(seed, offset, 4 * i + k, n, p), p, dtype))
        h = _block_drop_ref(h, prm, f"transformer.layers.{i}.", H, mask, masks)
    if cfg["masking"]:
        for i in range(cfg["post"]):
            h = torch.relu(h @ prm[f"network.{2 * i}.weight"].T + prm[f"network.{2 * i}.bias"])
    hidden = tu.pool_ref(h, mask, cfg["pooling_type"])
    logits = hidden @ prm["actor.weight"].T + prm["actor.bias"]
    value = hidden @ prm["critic.weight"].T + prm["critic.bias"]
    loss = (logits * torch.from_numpy(z["wl"]).to(dtype)).sum() + \
        (value * torch.from_numpy(z["wv"]).to(dtype)).sum()
    loss.backward()
    grads = {k: v.grad for k, v in prm.items() if v.grad is not None}
    return hidden.detach(), logits.detach(), value.detach(), grads


def test_agent_train_takes_the_fused_path_and_eval_is_the_dropout0_agent(dev):
    z = golden(FIXTURE)
    ag = _agent(z, dev, P_AGENT, fused_dropout=True)
    x = torch.from_numpy(z["x"]).to(dev)
    with torch.no_grad():
        h, fused = ag.tokens(x, ag.valid_mask(x))
    assert fused and ag.training
    assert torch.equal(ag.rng.cpu(), torch.tensor([SEED, 1]))
    assert "rng" not in ag.state_dict() and not list(ag.buffers())
    off = _agent(z, dev, P_AGENT)  # the default route for dropout > 0: torch's modules
    with torch.no_grad():
        assert off.tokens(x, off.valid_mask(x))[1] is False
    ag.eval()
    ag0 = _agent(z, dev, 0.0).eval()
    with torch.no_grad():
        a, b = ag.trunk(x), ag0.trunk(x)
        assert ag.tokens(x, ag.valid_mask(x))[1]
    assert torch.equal(a, b)
    assert not torch.equal(ag0.tokens(x, ag0.valid_mask(x))[0].detach(), h)
    assert torch.equal(ag.rng.cpu(), torch.tensor([SEED, 1]))  # eval() draws nothing


def test_agent_train_matches_f64_restatement_and_offsets_advance(dev):
    z = golden(FIXTURE)
    ag = _agent(z, dev, P_AGENT, fused_dropout=True)
    for offset in (0, 1):  # two successive forwards use offsets k and k + 1
        hidden, logits, value = _loss_backward(ag, z, dev)
        assert torch.equal(ag.rng.cpu(), torch.tensor([SEED, offset + 1]))
        r32 = _agent_drop_ref(z, torch.float32, offset)
        r64 = _agent_drop_ref(z, torch.float64, offset)
        for k, got, f32, twin in (("hidden", hidden, r32[0], r64[0]),
                                  ("logits", logits, r32[1], r64[1]),
                                  ("value", value, r32[2], r64[2])):
            tu.check(f"offset {offset} {k}", got, f32, twin)
        n = 0
        for k, prm in ag.named_parameters():
            if prm.grad is None:
                assert k not in r64[3], k
                continue
            n += 1
            tu.check(f"offset {offset} g:{k}", prm.grad, r32[3][k], r64[3][k])
        assert n == len(r64[3]) and n > 10
    assert tu.rel_err(_agent_drop_ref(z, torch.float64, 0)[0], r64[0]) > 1e-3  # masks differ


def _graph_body(ag, x, wl):
    hidden = ag.trunk(x)
    logits, value = ag.heads(hidden)
    loss = (logits * wl).sum() + value.sum()
    return [hidden] + list(torch.autograd.grad(loss, list(ag.parameters()), allow_unused=True))


def test_agent_forward_backward_replays_as_a_hipgraph(dev):
    """One forward + backward with its generator advance captured after an eager warm-up: every
    replay draws the masks of the next offset, bitwise the eager result at that offset."""
    z = golden(FIXTURE)
    x = torch.from_numpy(z["x"]).to(dev)
    wl = torch.from_numpy(z["wl"]).to(dev)
    eager = _agent(z, dev, P_AGENT, fused_dropout=True)
    want = [[t.clone() for t in _graph_body(eager, x, wl) if t is not None] for _ in range(3)]
    ag = _agent(z, dev, P_AGENT, fused_dropout=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        warm = [t.clone() for t in _graph_body(ag, x, wl) if t is not None]  # offset 0
    torch.cuda.current_stream().wait_stream(s)
    assert all(torch.equal(a, b) for a, b in zip(warm, want[0]))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = [t for t in _graph_body(ag, x, wl) if t is not None]
    torch.cuda.synchronize()
    assert torch.equal(ag.rng.cpu(), torch.tensor([SEED, 1]))  # capturing ran nothing
    got = []
    for k in (1, 2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(ag.rng.cpu(), torch.tensor([SEED, k + 1]))
        got.append([t.clone() for t in out])
        assert len(got[-1]) == len(want[k])
        assert all(torch.equal(a, b) for a, b in zip(got[-1], want[k])), k
    assert not torch.equal(got[0][0], got[1][0])  # the two replays' masks differ


# ---- the trainer --------------------------------------------------------------------------------
def _trainer(dev, **kw):
    from oc_cleanrl_amd.transformer import TransformerArgs, TransformerTrainer, finalize

    cfg = dict(num_envs=8, num_steps=8, buffer_window_size=6, num_features=8, emb_dim=32,
               num_heads=4, num_blocks=2, num_minibatches=2, update_epochs=2, dropout=0.1,
               fused_dropout=True, total_timesteps=8 * 8 * 100, seed=7, save_model=False,
               gemm_table=False)
    cfg.update(kw)
    return TransformerTrainer(finalize(TransformerArgs(**cfg)), dev, log=False)


def test_trainer_with_fused_dropout(dev, monkeypatch):
    """dropout = 0.1 on the fused path: two iterations (eager, then captured) with finite losses
    and moving parameters; the same seed gives the same bits; dropout = 0 gives other bits."""
    from oc_cleanrl_amd import ops

    calls = {"p": 0}
    mha = ops.mha
    monkeypatch.setattr(ops, "mha", lambda *a: (calls.__setitem__("p", calls["p"] + (len(a) == 6)),
                                                mha(*a))[1])
    runs = []
    for kw in ({}, {}, {"dropout": 0.0}):
        calls["p"] = 0
        tr = _trainer(dev, **kw)
        before = [p.detach().clone() for p in tr.params]
        for _ in range(2):
            m = tr.train_iteration()
        torch.cuda.synchronize()
        assert np.isfinite(tr.stats.cpu().numpy()).all() and np.isfinite(m["losses/value_loss"])
        assert all(not torch.equal(p, b) for p, b in zip(tr.params, before))
        if kw:
            assert calls["p"] == 0 and tr.agent.rng is None
        else:
            assert calls["p"] > 0 and tr.agent.fused_dropout
            assert int(tr.agent.rng[0]) == 7 and int(tr.agent.rng[1]) > 8  # > one rollout's forwards
        runs.append([p.detach().clone() for p in tr.params])
        tr.close()
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert not all(torch.equal(a, b) for a, b in zip(runs[0], runs[2]))
