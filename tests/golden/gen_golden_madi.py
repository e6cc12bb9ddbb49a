"""Writes the MaDi fixtures of tests/golden from the reference checkout (only this generator and
its outputs are committed):

    madi_args_fields.json : names and defaults of the `Args` dataclass of cleanrl/ppo_atari_madi.py,
                            read from the script's syntax tree (nothing of it is imported or run)
    madi_state_keys.json  : state-dict keys of the agent (architectures/ppo.py PPODefault,
                            normalize=False) and of the masker (architectures/madi.py MaskerNet)
    madi_init_f32.npz     : MaskerNet((4, 84, 84), 3, 32)'s initial weights after
                            torch.manual_seed(INIT_SEED)
    madi_ref_*.npz        : for the small shapes REF_SHAPES, the inputs and random weights of
                            tests/madi_util.make_case, the reference module's f32 output, and the
                            f64 output and f64 parameter gradients for the case's g

    python tests/golden/gen_golden_madi.py /path/to/reference            # the fixtures
    python tests/golden/gen_golden_madi.py /path/to/reference --search   # madi_util.CASE_SEEDS
"""
from __future__ import annotations

import ast
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import madi_util as U  # noqa: E402

INIT_SEED = 1
REF_SHAPES = ((1, 1, 3, 16), (2, 1, 17, 32), (1, 4, 17, 32))
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")


def fields(script: Path) -> list:
    tree = ast.parse(script.read_text())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Args")
    out = []
    for node in cls.body:
        if isinstance(node, ast.AnnAssign):
            value = eval(compile(ast.Expression(node.value), "<default>", "eval"),
                         {"__builtins__": {}, "int": int, "float": float})
            out.append({"name": node.target.id, "type": ast.unparse(node.annotation),
                        "default": value})
    return out


class _Space:
    def __init__(self, shape=(), n=None):
        self.shape, self.n = shape, n


class _Envs:
    observation_space = _Space((4, 84, 84))
    action_space = _Space((), 6)


def main(ref: Path, search: bool):
    if search:
        print({shape: U.find_seed(shape) for shape in U.CASES})
        return
    (HERE / "madi_args_fields.json").write_text(
        json.dumps(fields(ref / "cleanrl" / "ppo_atari_madi.py"), indent=1) + "\n")
    sys.path.insert(0, str(ref / "cleanrl"))
    from architectures.madi import MaskerNet
    from architectures.ppo import PPODefault

    torch.manual_seed(INIT_SEED)
    masker = MaskerNet((4, 84, 84), 3, 32)
    agent = PPODefault(_Envs(), "cpu", normalize=False)
    (HERE / "madi_state_keys.json").write_text(json.dumps(
        {"agent": list(agent.state_dict()), "masker": list(masker.state_dict())}, indent=1) + "\n")
    np.savez_compressed(HERE / "madi_init_f32.npz", seed=INIT_SEED,
                        **{k: v.numpy() for k, v in masker.state_dict().items()})
    for shape in REF_SHAPES:
        B, W, H, F = shape
        case = U.make_case(*shape, U.CASE_SEEDS[shape])
        m = MaskerNet((W, H, H), 3, F)
        convs = [l for l in m.layers if isinstance(l, torch.nn.Conv2d)]
        with torch.no_grad():
            for i, c in enumerate(convs):
                c.weight.copy_(case["weights"][2 * i])
                c.bias.copy_(case["weights"][2 * i + 1])
            y32 = m(case["x"].float())
        y64, g64, zmin = U.reference(case, torch.float64)
        assert zmin >= U.Z_MIN, (shape, zmin)
        np.savez_compressed(
            HERE / f"madi_ref_b{B}w{W}h{H}f{F}.npz", x=case["x"].numpy(), g=case["g"].numpy(),
            seed=case["seed"], y_f32=y32.numpy(), y_f64=y64.numpy(),
            **{n: w.numpy() for n, w in zip(NAMES, case["weights"])},
            **{"d" + n: d.numpy() for n, d in zip(NAMES, g64)})


if __name__ == "__main__":
    main(Path(sys.argv[1]), "--search" in sys.argv[2:])
