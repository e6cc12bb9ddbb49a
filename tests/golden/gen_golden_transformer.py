"""Generate the transformer-agent fixtures under tests/golden/ FROM THE REFERENCE ITSELF.

Like gen_golden_rainbow.py this runs only where the reference checkout is mounted read-only; only
the .npz / .json outputs are committed, no reference program text is stored.

What is executed: cleanrl/ppo_atari_oc_transformer.py is read as text by line range, dedented,
compiled and exec'd:
    :209-212  layer_init
    :215-277  PPOAgent, with a stub `args` namespace (dropout, pooling_type, num_post_layers) as
              the module global it reads
The agent is put in train() mode with dropout = 0, so torch takes its standard path and not the
inference fast path.

Fixtures (each records the numpy and torch versions that made it):
  transformer_args_fields.json  [name, default] of the script's Args dataclass, declaration order
  transformer_{name}.npz      the configuration, inputs x [B, S, F] with padded (all-zero type
                        columns) objects, the seeded state dict ("p:" + key), the encoder output,
                        every block's output, hidden / logits / value, the scalar loss
                        sum(logits * wl) + sum(value * wv) and every parameter gradient ("g:" + key)
  transformer_{name}_f64.npz  the same computation as a float64 twin on the same f32 inputs and
                        weights, under the same names

    python tests/golden/gen_golden_transformer.py
"""
from __future__ import annotations

import ast
import json
import sys
import textwrap
import types
import warnings
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn
from torch.distributions import Categorical
from torch.nn import TransformerEncoder, TransformerEncoderLayer

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
SCRIPT = REF / "cleanrl" / "ppo_atari_oc_transformer.py"
INIT_LINES = (209, 212)
AGENT_LINES = (215, 277)

sys.dont_write_bytecode = True
warnings.filterwarnings("ignore", category=UserWarning)
VERSIONS = dict(numpy_version=np.array(np.__version__), torch_version=np.array(torch.__version__))


def block(lines):
    src = SCRIPT.read_text().splitlines()[lines[0] - 1:lines[1]]
    return compile(textwrap.dedent("\n".join(src)), f"{SCRIPT}:{lines[0]}-{lines[1]}", "exec")


ARGS = types.SimpleNamespace(dropout=0.0, pooling_type="max", num_post_layers=1)
NS = dict(torch=torch, nn=nn, np=np, Categorical=Categorical,
          TransformerEncoder=TransformerEncoder, TransformerEncoderLayer=TransformerEncoderLayer,
          args=ARGS)
exec(block(INIT_LINES), NS)
exec(block(AGENT_LINES), NS)


class Space:
    def __init__(self, shape=None, n=None):
        self.shape = shape
        self.n = n


class Envs:
    def __init__(self, obs_shape, n_actions):
        self.observation_space = Space(shape=tuple(obs_shape))
        self.action_space = Space(shape=(), n=n_actions)


def gen_args_fields():
    cls = next(n for n in ast.parse(SCRIPT.read_text()).body
               if isinstance(n, ast.ClassDef) and n.name == "Args")
    fields = []
    for s in cls.body:
        if not isinstance(s, ast.AnnAssign):
            continue
        try:
            default = ast.literal_eval(s.value)
        except ValueError:
            if s.target.id == "exp_name":  # the script's file name without ".py"
                default = SCRIPT.stem
            else:  # seed: a random draw per run
                assert s.target.id == "seed"
                default = None
        fields.append([s.target.id, default])
    (OUT / "transformer_args_fields.json").write_text(json.dumps(fields, indent=1) + "\n")


def inputs(rng, B, S, F, num_obj, masked):
    """Object sets: a one-hot type in the first num_obj columns, features after; padded objects
    are all-zero rows (ragged tails, one hole in the middle, one sample with a single object)."""
    x = rng.standard_normal((B, S, F)).astype(np.float32)
    x[..., :num_obj] = 0
    kind = rng.integers(0, num_obj, (B, S))
    for b in range(B):
        x[b, np.arange(S), kind[b]] = 1.0
    if masked:
        for b in range(B):
            n = S if b == 0 else max(1, int(rng.integers(1, S + 1)))
            x[b, n:] = 0
        if B > 1 and S > 2:
            x[1, :] = 0
            x[1, 0, 0] = 1.0          # exactly one valid object
            x[1, 0, num_obj:] = rng.standard_normal(F - num_obj)
        if B > 2 and S > 3:
            x[2] = rng.standard_normal((S, F))
            x[2, :, :num_obj] = 0
            x[2, :, 1 % num_obj] = 1.0
            x[2, 1] = 0               # a hole in the middle
    return x


def run(agent, x, wl, wv, dtype):
    agent = agent.to(dtype)
    agent.train()
    outs = {}
    hooks = [agent.encoder.register_forward_hook(
        lambda m, i, o: outs.__setitem__("enc", o.detach().numpy()))]
    for k, layer in enumerate(agent.transformer.layers):
        hooks.append(layer.register_forward_hook(
            lambda m, i, o, k=k: outs.__setitem__(f"block{k}", o.detach().numpy())))
    xt = torch.from_numpy(x).to(dtype)
    hidden = agent.forward(xt)
    logits, value = agent.actor(hidden), agent.critic(hidden)
    loss = (logits * torch.from_numpy(wl).to(dtype)).sum() + \
        (value * torch.from_numpy(wv).to(dtype)).sum()
    agent.zero_grad()
    loss.backward()
    for h in hooks:
        h.remove()
    outs.update(hidden=hidden.detach().numpy(), logits=logits.detach().numpy(),
                value=value.detach().numpy(), loss=np.array(loss.item()))
    for k, p in agent.named_parameters():
        if p.grad is not None:  # masking off: the reference's forward skips the post layers
            outs["g:" + k] = p.grad.detach().numpy().copy()
    return outs


def gen(name, emb, heads, blocks, post, S, F, B, pooling, masked, seed, A=6, num_obj=3):
    ARGS.pooling_type, ARGS.num_post_layers, ARGS.dropout = pooling, post, 0.0
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    agent = NS["PPOAgent"](Envs((S, F), A), emb, heads, blocks, masked, num_obj, "cpu")
    sd = {k: v.detach().clone() for k, v in agent.state_dict().items()}
    x = inputs(rng, B, S, F, num_obj, masked)
    valid = x[..., :num_obj].sum(-1) != 0
    assert valid.any(1).all(), "a fully padded sample is outside the contract"
    if masked:
        assert (~valid).any() and (valid.sum(1) == 1).any()
    wl = rng.standard_normal((B, A)).astype(np.float32)
    wv = rng.standard_normal((B, 1)).astype(np.float32)
    r32 = run(agent, x, wl, wv, torch.float32)
    agent.load_state_dict(sd)
    r64 = run(agent, x, wl, wv, torch.float64)
    if pooling == "max":
        # which row wins the max must not hang on a rounding: margin between best and second
        h = r64[f"block{blocks - 1}"]
        if masked:
            w = {k: v.double().numpy() for k, v in sd.items()}
            for i in range(post):
                h = np.maximum(h @ w[f"network.{2 * i}.weight"].T + w[f"network.{2 * i}.bias"], 0)
            h = h * valid[..., None]
        if S > 1:
            top2 = np.sort(h, axis=1)[:, -2:]
            gap = top2[:, 1] - top2[:, 0]
            # (a maximum of exactly 0 is a tie of ReLU-cut / masked rows: no gradient either way)
            ok = (gap > 1e-4 * np.abs(h).max()) | (top2[:, 1] == 0)
            assert ok.all(), (name, float(ok.mean()))
            print(f"{name}: max-pool margin > 1e-4 of the largest element, or an exact 0, in "
                  f"every column; smallest non-zero margin {gap[top2[:, 1] != 0].min():.3g}")
    cfg = dict(emb_dim=emb, num_heads=heads, num_blocks=blocks, num_post_layers=post, S=S, F=F,
               B=B, pooling_type=np.array(pooling), masking=masked, seed=seed, n_actions=A,
               num_obj=num_obj)
    main = dict(cfg, x=x, wl=wl, wv=wv, keys=np.array(list(sd)), **VERSIONS,
                **{"p:" + k: v.numpy() for k, v in sd.items()}, **r32)
    np.savez_compressed(OUT / f"transformer_{name}.npz", **main)
    np.savez_compressed(OUT / f"transformer_{name}_f64.npz", **cfg, **VERSIONS, **r64)
    err = max(float(np.abs(r32[k] - r64[k]).max() / np.abs(r64[k]).max())
              for k in r64 if k.startswith("g:"))
    print(f"transformer_{name}: loss {float(r32['loss'])!r}, worst f32 gradient error {err:.3g}")


def main():
    torch.set_num_threads(8)
    gen_args_fields()
    gen("e32_max", 32, 4, 2, 1, S=6, F=8, B=5, pooling="max", masked=True, seed=61)
    gen("e128_mean", 128, 8, 1, 1, S=17, F=8, B=3, pooling="mean", masked=True, seed=62)
    gen("e32_first_nomask", 32, 4, 1, 1, S=5, F=8, B=4, pooling="first", masked=False, seed=63)
    print("fixtures written to", OUT)


if __name__ == "__main__":
    main()
