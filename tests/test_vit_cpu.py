"""ViTAgent without a GPU: the state-dict keys and shapes are vit_pytorch SimpleViT's behind
nn.Sequential(SimpleViT, nn.Flatten) plus the two heads, pos_embedding stays outside the state
dict, and the learner's flags carry the script's defaults."""
import torch


def _expected(C, p, dim, heads, blocks, A):
    E, inner = C * p * p, heads * 64
    keys = {"network.0.to_patch_embedding.1": (E,), "network.0.to_patch_embedding.3": (dim,),
            "network.0.transformer.norm": (dim,)}
    lin = {"network.0.to_patch_embedding.2": (dim, E), "network.0.linear_head": (dim, dim),
           "actor": (A, dim), "critic": (1, dim)}
    out = {}
    for i in range(blocks):
        pre = f"network.0.transformer.layers.{i}."
        keys[pre + "0.norm"] = keys[pre + "1.net.0"] = (dim,)
        out[pre + "0.to_qkv.weight"] = (3 * inner, dim)  # bias-free
        out[pre + "0.to_out.weight"] = (dim, inner)
        lin[pre + "1.net.1"] = lin[pre + "1.net.3"] = (dim, dim)
    for k, s in keys.items():
        out[k + ".weight"] = out[k + ".bias"] = s
    for k, s in lin.items():
        out[k + ".weight"], out[k + ".bias"] = s, s[:1]
    return out


def test_vit_agent_state_dict_and_forward():
    from oc_cleanrl_amd.agents import EnvSpec
    from oc_cleanrl_amd.vit import ViTAgent, ViTArgs, posemb_sincos_2d

    torch.manual_seed(0)
    agent = ViTAgent(EnvSpec((4, 84, 84), 6), emb_dim=32, num_heads=2, num_blocks=2, patch_size=12)
    got = {k: tuple(v.shape) for k, v in agent.state_dict().items()}
    assert got == _expected(4, 12, 32, 2, 2, 6)
    pos = agent.network[0].pos_embedding
    assert not isinstance(pos, torch.nn.Parameter) and tuple(pos.shape) == (49, 32)
    assert torch.equal(pos, posemb_sincos_2d(7, 7, 32)) and float(pos[0, 8]) == 1.0  # cos(0)
    x = torch.randint(0, 256, (3, 4, 84, 84), dtype=torch.uint8)
    logits, value = agent.logits_and_value(x)
    assert tuple(logits.shape) == (3, 6) and tuple(value.shape) == (3, 1)
    assert not agent.fused_ok(x)  # CPU stacks: the plain path
    a = ViTArgs()
    assert (a.emb_dim, a.num_heads, a.num_blocks, a.patch_size, a.num_envs, a.seed, a.clip_coef,
            a.obs_mode, a.backend) == (128, 8, 4, 12, 10, 42, 0.1, "dqn", "Synthetic")
