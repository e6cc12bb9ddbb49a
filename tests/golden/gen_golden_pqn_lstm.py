"""Generate the recurrent-PQN fixtures under tests/golden/ FROM THE REFERENCE ITSELF.

Like gen_golden_lstm.py this runs only where the reference checkout is mounted read-only; only
the .json outputs are committed, no reference program text is stored.

What is executed: cleanrl/pqn_atari_envpool_lstm.py is read as text by line range, dedented,
compiled and exec'd:
    :111-114  layer_init
    :117-165  QNetwork
and its Args dataclass (:20-74) is read through `ast` (nothing of it is executed).

Fixtures (recorded data: names, defaults and shapes only):
  pqn_lstm_args.json        [name, default] of the script's Args dataclass, declaration order
  pqn_lstm_state_keys.json  [key, shape] of QNetwork(envs).state_dict() for the script's
                            84 x 84 x 1 observation and 6 actions, in state-dict order

    python tests/golden/gen_golden_pqn_lstm.py
"""
from __future__ import annotations

import ast
import json
import sys
import textwrap
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
SCRIPT = REF / "cleanrl" / "pqn_atari_envpool_lstm.py"
INIT_LINES = (111, 114)
NET_LINES = (117, 165)
N_ACTIONS = 6

sys.dont_write_bytecode = True


def block(lines):
    text = textwrap.dedent("\n".join(SCRIPT.read_text().splitlines()[lines[0] - 1:lines[1]]))
    return compile(text, f"{SCRIPT}:{lines[0]}-{lines[1]}", "exec")


class Space:
    def __init__(self, n):
        self.n = n


class Envs:
    def __init__(self, n_actions):
        self.single_action_space = Space(n_actions)


def gen_args():
    cls = next(n for n in ast.parse(SCRIPT.read_text()).body
               if isinstance(n, ast.ClassDef) and n.name == "Args")
    fields = []
    for s in cls.body:
        if not isinstance(s, ast.AnnAssign):
            continue
        try:
            default = ast.literal_eval(s.value)
        except ValueError:
            assert s.target.id == "exp_name"  # the script's file name without ".py"
            default = SCRIPT.stem
        fields.append([s.target.id, default])
    (OUT / "pqn_lstm_args.json").write_text(json.dumps(fields, indent=1) + "\n")


def gen_state_keys():
    ns = dict(torch=torch, nn=nn, np=np)
    exec(block(INIT_LINES), ns)
    exec(block(NET_LINES), ns)
    torch.manual_seed(1)
    net = ns["QNetwork"](Envs(N_ACTIONS))
    q, _ = net(torch.zeros(2, 1, 84, 84), (torch.zeros(1, 2, 128), torch.zeros(1, 2, 128)),
               torch.zeros(2))
    assert tuple(q.shape) == (2, N_ACTIONS)
    keys = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    (OUT / "pqn_lstm_state_keys.json").write_text(json.dumps(keys, indent=1) + "\n")


def main():
    gen_args()
    gen_state_keys()
    print("fixtures written to", OUT)


if __name__ == "__main__":
    main()
