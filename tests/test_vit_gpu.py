"""The pixel ViT on the GPU: ops.vit_patch_ln (csrc/ocppo_vit_patch.hip) against its float64 twin
(rearrange by reshape / permute, F.layer_norm on the 0-255 values), ViTAgent's fused path against
FUSED_VIT = False on the same weights, and two ViTTrainer iterations. The error rule is
tests/transformer_util.py's: at most max(3 x torch's own f32 error, 4 * 2^-23) of the twin's
largest element. Run with -s for the (measured / torch's own) pairs."""
import copy

import pytest
import torch
import torch.nn.functional as F

import transformer_util as tu

pytestmark = pytest.mark.gpu

H = 84


def _frames(C, gen):
    """Six u8 stacks: 0 all zero, 1 with a constant-200 patch at token (0, 0), 2 with every pixel
    encoding its (channel, row, column), the rest random."""
    src = torch.randint(0, 256, (6, C, H, H), generator=gen, dtype=torch.uint8)
    src[0] = 0
    src[1, :, :21, :21] = 200
    c, r, w = torch.meshgrid(torch.arange(C), torch.arange(H), torch.arange(H), indexing="ij")
    src[2] = ((c * 61 + r * H + w) % 251).to(torch.uint8)
    return src


def _twin(src, idx, p, gamma, beta, dy, dtype):
    x = (src if idx is None else src[idx]).to(dtype)
    R, C = x.shape[:2]
    x = x.reshape(R, C, H // p, p, H // p, p).permute(0, 2, 4, 3, 5, 1).reshape(R, -1, p * p * C)
    g, b = (t.detach().to(dtype).clone().requires_grad_(True) for t in (gamma, beta))
    y = F.layer_norm(x, (x.shape[-1],), g, b, 1e-5)
    y.backward(dy.to(dtype))
    return x, y.detach(), g.grad, b.grad


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("p", [12, 14, 21])
def test_vit_patch_ln_matches_f64_twin(dev, p, C, R, permuted):
    from oc_cleanrl_amd import ops

    gen = torch.Generator().manual_seed(p * 100 + C * 10 + R)
    src = _frames(C, gen).to(dev)
    E, T = C * p * p, (H // p) ** 2
    idx = torch.tensor([3, 1, 0, 1, 2][:R] if permuted else list(range(R)), device=dev)
    ln = torch.nn.LayerNorm(E).to(dev)
    with torch.no_grad():
        ln.weight.copy_(torch.randn(E, generator=gen))
        ln.bias.copy_(torch.randn(E, generator=gen))
    dy = torch.randn(R, T, E, generator=gen).to(dev)
    y = ops.vit_patch_ln(src[:R] if not permuted else src, idx if permuted else None, ln, p)
    y.backward(dy)
    x, y64, dg64, db64 = _twin(src, idx, p, ln.weight, ln.bias, dy, torch.float64)
    _, y32, dg32, db32 = _twin(src, idx, p, ln.weight, ln.bias, dy, torch.float32)
    tu.check("y", y.detach(), y32, y64)
    tu.check("dgamma", ln.weight.grad, dg32, dg64)
    tu.check("dbeta", ln.bias.grad, db32, db64)
    const = x.amax(-1) == x.amin(-1)  # the zero frame's tokens, the constant-200 patch
    assert bool(const.any()) == (R == 5 or not permuted)
    assert torch.equal(y.detach()[const], ln.bias.detach().expand(int(const.sum()), E))
    dg, db = ln.weight.grad.clone(), ln.bias.grad.clone()
    ln.zero_grad()
    ops.vit_patch_ln(src[:R] if not permuted else src, idx if permuted else None, ln, p).backward(dy)
    assert torch.equal(ln.weight.grad, dg) and torch.equal(ln.bias.grad, db)


def _agent_grads(agent, src, fused, dl, dv, dtype=torch.float32):
    from oc_cleanrl_amd import vit

    ag = copy.deepcopy(agent).to(dtype)
    hidden = ag.trunk_stacks(src, None) if fused else ag.trunk(src)
    if fused:
        assert vit.FUSED_VIT and ag.fused_ok(src)
    logits, value = ag.actor(hidden), ag.critic(hidden)
    torch.autograd.backward([logits, value], [dl.to(dtype), dv.to(dtype)])
    return {"logits": logits.detach(), "value": value.detach(),
            **{n: q.grad for n, q in ag.named_parameters()}}


def test_vit_agent_fused_matches_plain(dev):
    from oc_cleanrl_amd.agents import EnvSpec
    from oc_cleanrl_amd.vit import ViTAgent

    torch.manual_seed(11)
    gen = torch.Generator().manual_seed(12)
    agent = ViTAgent(EnvSpec((4, H, H), 6), emb_dim=32, num_heads=2, num_blocks=2).to(dev)
    src = _frames(4, gen)[1:4].to(dev)
    dl, dv = torch.randn(3, 6, generator=gen).to(dev), torch.randn(3, 1, generator=gen).to(dev)
    got = _agent_grads(agent, src, True, dl, dv)
    f32 = _agent_grads(agent, src, False, dl, dv)
    twin = _agent_grads(agent, src, False, dl, dv, torch.float64)
    assert set(got) == set(twin) and all(v is not None for v in got.values())
    for name in got:
        tu.check(name, got[name], f32[name], twin[name])


def test_vit_trainer_two_iterations_and_reload(dev, tmp_path):
    from oc_cleanrl_amd.agents import EnvSpec
    from oc_cleanrl_amd.vit import ViTAgent, ViTArgs, ViTTrainer, finalize

    args = finalize(ViTArgs(num_envs=4, num_steps=8, num_blocks=1, total_timesteps=4 * 8 * 100,
                            seed=3, save_model=False, gemm_table=False, track=False,
                            capture_video=False))
    tr = ViTTrainer(args, dev, log=False)
    assert tr.agent.fused_ok(tr.b_obs)
    before = [q.detach().clone() for q in tr.agent.parameters()]
    for _ in range(2):
        m = tr.train_iteration()
    assert all(torch.isfinite(torch.as_tensor(float(v))) for v in m.values()
               if isinstance(v, (int, float)))
    assert all(not torch.equal(b, q.detach()) for b, q in zip(before, tr.agent.parameters()))
    path = tmp_path / "vit.cleanrl_model"
    tr.save(path)
    fresh = ViTAgent(EnvSpec(tr.obs_shape, tr.A), args.emb_dim, args.num_heads, args.num_blocks,
                     args.patch_size)
    fresh.load_state_dict(torch.load(path, map_location="cpu", weights_only=False)["model_weights"],
                          strict=True)
    tr.close()
