"""Writes tests/golden/ppg_args_fields.json: the names and defaults of the `Args` dataclass of
cleanrl/ppg_procgen.py, read from the script's syntax tree (nothing of it is imported or run).

    python tests/golden/gen_golden_ppg.py /path/to/reference/cleanrl/ppg_procgen.py
"""
from __future__ import annotations

import ast
import json
import sys
from pathlib import Path


def fields(script: Path) -> list:
    tree = ast.parse(script.read_text())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Args")
    out = []
    for node in cls.body:
        if not isinstance(node, ast.AnnAssign):
            continue
        name = node.target.id
        if name == "exp_name":  # os.path.basename(__file__) without ".py"
            value = script.stem
        else:  # literals and int(25e6)
            value = eval(compile(ast.Expression(node.value), "<default>", "eval"),
                         {"__builtins__": {}, "int": int, "float": float})
        out.append({"name": name, "type": ast.unparse(node.annotation), "default": value})
    return out


if __name__ == "__main__":
    dst = Path(__file__).resolve().parent / "ppg_args_fields.json"
    dst.write_text(json.dumps(fields(Path(sys.argv[1])), indent=1) + "\n")
    print(dst)
