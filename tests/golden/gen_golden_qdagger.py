"""Generate the QDagger fixtures from the reference script (data only, no reference text):

    python tests/golden/gen_golden_qdagger.py /path/to/reference

  qdagger_args_fields.json  names and defaults of the script's Args, found by AST
  qdagger_state_keys.json   keys and shapes of the script's student for a (4, 84, 84) input and
                            6 actions (its classes are executed from the file)
  qdagger_loss_B*_A*.npz    inputs and outputs of the script's own loss lines :303-315 (offline,
                            coefficient 1.0) and :412-424 (online, coefficient 0.37), executed
                            from the file with stand-ins for the networks and the batch, with
                            loss.backward() for dq, in f32 and in f64
"""
import ast
import json
import sys
import textwrap
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
SCRIPT = "cleanrl/qdagger_dqn_atari_impalacnn.py"
OFFLINE_LINES, ONLINE_LINES = (303, 315), (412, 424)
CASES = [(7, 18), (32, 6)]
TEMPERATURES = (1.0, 0.5)
ONLINE_COEFF = 0.37
GAMMA = 0.99


def args_fields(tree, path: Path) -> dict:
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Args")
    out = {}
    for n in cls.body:
        if isinstance(n, ast.AnnAssign):
            try:
                out[n.target.id] = ast.literal_eval(n.value)
            except ValueError:
                assert n.target.id == "exp_name"  # derived from the file's name
                out[n.target.id] = path.stem
    return out


def definitions(tree, src: str, names) -> dict:
    """Execute the named top-level classes / functions of the script in a fresh namespace."""
    import torch.nn as nn
    import torch.nn.functional as F

    ns = {"torch": torch, "nn": nn, "F": F}
    for n in tree.body:
        if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names:
            exec(compile(ast.Module([n], []), SCRIPT, "exec"), ns)
    return ns


def state_keys(tree, src: str) -> dict:
    ns = definitions(tree, src, ("ResidualBlock", "ConvSequence", "QNetwork"))
    space = types.SimpleNamespace
    envs = space(single_observation_space=space(shape=(4, 84, 84)), single_action_space=space(n=6))
    ns["envs"] = envs
    net = ns["QNetwork"](envs)
    return {k: list(v.shape) for k, v in net.state_dict().items()}


def run_lines(lines, span, ns_defs, t: dict, dtype, temperature: float, coeff: float) -> dict:
    """The script's lines `span` on the tensors `t` cast to `dtype`."""
    import torch.nn.functional as F

    code = textwrap.dedent("".join(lines[span[0] - 1:span[1]]))
    c = {k: v.to(dtype) if v.is_floating_point() else v for k, v in t.items()}
    q = c["q"].clone().requires_grad_(True)
    space = types.SimpleNamespace
    data = space(observations="obs", next_observations="next", actions=c["actions"].reshape(-1, 1),
                 rewards=c["rewards"].reshape(-1, 1), dones=c["dones"].reshape(-1, 1))
    ns = {"torch": torch, "F": F, "data": data, "distill_coeff": coeff,
          "args": space(gamma=GAMMA, temperature=temperature),
          "kl_divergence_with_logits": ns_defs["kl_divergence_with_logits"],
          "target_network": lambda x: c["q_next"], "teacher_model": lambda x: c["q_teacher"],
          "q_network": lambda x: q}
    exec(code, ns)
    ns["loss"].backward()
    return {"loss": ns["loss"].detach().numpy(), "q_loss": ns["q_loss"].detach().numpy(),
            "distill_loss": ns["distill_loss"].detach().numpy(),
            "q_values": ns["old_val"].mean().detach().numpy(), "dq": q.grad.numpy()}


def main(reference: str):
    path = Path(reference) / SCRIPT
    src = path.read_text()
    tree = ast.parse(src)
    lines = src.splitlines(keepends=True)
    (HERE / "qdagger_args_fields.json").write_text(json.dumps(args_fields(tree, path), indent=1))
    torch.manual_seed(0)
    (HERE / "qdagger_state_keys.json").write_text(json.dumps(state_keys(tree, src), indent=1))
    defs = definitions(tree, src, ("kl_divergence_with_logits",))
    for B, A in CASES:
        g = torch.Generator().manual_seed(1000 * B + A)
        t = {"q": torch.randn(B, A, generator=g), "q_next": torch.randn(B, A, generator=g),
             "q_teacher": 2 * torch.randn(B, A, generator=g),
             "actions": torch.randint(0, A, (B,), generator=g),
             "rewards": torch.randn(B, generator=g),
             "dones": (torch.arange(B) % 2).float()}
        out = {k: v.numpy() for k, v in t.items()}
        for T in TEMPERATURES:
            for coeff, span in ((1.0, OFFLINE_LINES), (ONLINE_COEFF, ONLINE_LINES)):
                for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
                    r = run_lines(lines, span, defs, t, dtype, T, coeff)
                    for k, v in r.items():
                        out[f"T{T}_c{coeff}_{tag}_{k}"] = v
        np.savez(HERE / f"qdagger_loss_B{B}_A{A}.npz", **out)


if __name__ == "__main__":
    main(sys.argv[1])
