"""Generate the recurrent-agent fixtures under tests/golden/ FROM THE REFERENCE ITSELF.

Like gen_golden_transformer.py this runs only where the reference checkout is mounted read-only;
only the .npz / .json outputs are committed, no reference program text is stored.

What is executed: cleanrl/ppo_atari_lstm.py is read as text by line range, dedented, compiled and
exec'd:
    :111-114  layer_init
    :117-170  Agent
    :296-306  the minibatch index code (envsperbatch, envinds, flatinds, the epoch / start loops),
              with `args` a stub namespace and the loop body cut after `mb_inds = ...`

Fixtures (each records the numpy and torch versions that made it):
  lstm_args_fields.json  [name, default] of the script's Args dataclass, declaration order
  lstm_ref_{name}.npz    inputs x [T * B, 1, 84, 84] (time-major), done [T * B], the initial state
                         h0 / c0 [1, B, 128], the seeded state dict ("p:" + key), get_states'
                         output and final state, logits / value, the scalar loss
                         sum(logits * wl) + sum(value * wv) and every parameter gradient
                         ("g:" + key); tensors of more than lstm_util.FULL_MAX elements are held
                         as shape, float64 sum and a fixed sample (the committed-file size limit;
                         the seeded init is re-created from `seed` by the test); and mb_inds
                         [epochs, minibatches, T * envs / minibatches], what the script's index
                         code yields after np.random.seed(mb_seed) at num_envs = 8, num_steps = 4,
                         num_minibatches = 4
  lstm_ref_{name}_f64.npz  the same computation as a float64 twin on the same f32 inputs and
                         weights, under the same names

    python tests/golden/gen_golden_lstm.py
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
from torch.distributions.categorical import Categorical

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))
from lstm_util import FULL_MAX, pick_indices  # noqa: E402
SCRIPT = REF / "cleanrl" / "ppo_atari_lstm.py"
INIT_LINES = (111, 114)
AGENT_LINES = (117, 170)
INDEX_HEAD = (296, 300)   # assert ... clipfracs = []
INDEX_LOOP = (301, 306)   # for epoch ... mb_inds = flatinds[:, mbenvinds].ravel()

sys.dont_write_bytecode = True
warnings.filterwarnings("ignore", category=UserWarning)
VERSIONS = dict(numpy_version=np.array(np.__version__), torch_version=np.array(torch.__version__))


def text(lines):
    return textwrap.dedent("\n".join(SCRIPT.read_text().splitlines()[lines[0] - 1:lines[1]]))


def block(lines):
    return compile(text(lines), f"{SCRIPT}:{lines[0]}-{lines[1]}", "exec")


NS = dict(torch=torch, nn=nn, np=np, Categorical=Categorical)
exec(block(INIT_LINES), NS)
exec(block(AGENT_LINES), NS)


class Space:
    def __init__(self, shape=None, n=None):
        self.shape = shape
        self.n = n


class Envs:
    def __init__(self, n_actions):
        self.single_action_space = Space(shape=(), n=n_actions)


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
            assert s.target.id == "exp_name"  # the script's file name without ".py"
            default = SCRIPT.stem
        fields.append([s.target.id, default])
    (OUT / "lstm_args_fields.json").write_text(json.dumps(fields, indent=1) + "\n")


def mb_inds(seed, num_envs=8, num_steps=4, num_minibatches=4, update_epochs=3):
    """The script's own index code, with a line appended to the loop body that records mb_inds."""
    rec = []
    ns = dict(np=np, rec=rec, args=types.SimpleNamespace(
        num_envs=num_envs, num_steps=num_steps, num_minibatches=num_minibatches,
        update_epochs=update_epochs, batch_size=num_envs * num_steps))
    np.random.seed(seed)
    exec(block(INDEX_HEAD), ns)
    loop = text(INDEX_LOOP)
    indent = loop.splitlines()[-1][:len(loop.splitlines()[-1]) - len(loop.splitlines()[-1].lstrip())]
    exec(compile(loop + "\n" + indent + "rec.append(mb_inds.copy())\n", "index loop", "exec"), ns)
    return np.stack(rec).reshape(update_epochs, num_minibatches, -1)


def pack(out, key, arr):
    """Tensors of more than FULL_MAX elements (the 3136 x 512 Linear, the LSTM matrices) as their
    shape, float64 sum and the elements at lstm_util.pick_indices; smaller ones whole."""
    arr = np.asarray(arr)
    if arr.size <= FULL_MAX:
        out[key] = arr
    else:
        out[key + "::shape"] = np.array(arr.shape)
        out[key + "::sum"] = np.array(arr.astype(np.float64).sum())
        out[key + "::pick"] = arr.reshape(-1)[pick_indices(arr.size)]


def run(agent, x, done, h0, c0, wl, wv, dtype):
    agent = agent.to(dtype)
    t = lambda a: torch.from_numpy(a).to(dtype)  # noqa: E731
    hidden, (hT, cT) = agent.get_states(t(x), (t(h0), t(c0)), t(done))
    logits, value = agent.actor(hidden), agent.critic(hidden)
    loss = (logits * t(wl)).sum() + (value * t(wv)).sum()
    agent.zero_grad()
    loss.backward()
    outs = dict(hidden=hidden.detach().numpy(), hT=hT.detach().numpy(), cT=cT.detach().numpy(),
                logits=logits.detach().numpy(), value=value.detach().numpy(),
                loss=np.array(loss.item()))
    for k, p in agent.named_parameters():
        pack(outs, "g:" + k, p.grad.detach().numpy().copy())
    return outs


def gen(name, T, B, seed, done_kind, zero_state, A=4, mb_seed=7):
    assert T * B <= 12
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    agent = NS["Agent"](Envs(A))
    sd = {k: v.detach().clone() for k, v in agent.state_dict().items()}
    x = rng.integers(0, 256, (T * B, 1, 84, 84)).astype(np.float32)
    done = np.zeros((T, B), np.float32)
    if done_kind == "mixed":
        done[rng.random((T, B)) < 0.3] = 1.0
        done[0, 0] = 1.0
    H = agent.lstm.hidden_size
    h0 = np.zeros((1, B, H), np.float32) if zero_state else \
        rng.standard_normal((1, B, H)).astype(np.float32)
    c0 = np.zeros((1, B, H), np.float32) if zero_state else \
        rng.standard_normal((1, B, H)).astype(np.float32)
    done = done.reshape(-1)
    wl = rng.standard_normal((T * B, A)).astype(np.float32)
    wv = rng.standard_normal((T * B, 1)).astype(np.float32)
    r32 = run(agent, x, done, h0, c0, wl, wv, torch.float32)
    agent.load_state_dict(sd)
    r64 = run(agent, x, done, h0, c0, wl, wv, torch.float64)
    cfg = dict(T=T, B=B, seed=seed, n_actions=A, mb_seed=mb_seed, mb_inds=mb_inds(mb_seed))
    main = dict(cfg, x=x.astype(np.uint8), done=done, h0=h0, c0=c0, wl=wl, wv=wv,
                keys=np.array(list(sd)), **VERSIONS, **r32)
    for k, v in sd.items():  # the seeded init: the test re-creates it from `seed`
        pack(main, "p:" + k, v.numpy())
    np.savez_compressed(OUT / f"lstm_ref_{name}.npz", **main)
    np.savez_compressed(OUT / f"lstm_ref_{name}_f64.npz", **cfg, **VERSIONS, **r64)
    err = max(float(np.abs(r32[k] - r64[k]).max() / max(np.abs(r64[k]).max(), 1e-300))
              for k in r64 if k.startswith("g:") and not k.endswith("::shape"))
    print(f"lstm_ref_{name}: loss {float(r32['loss'])!r}, worst f32 gradient error {err:.3g}")


def main():
    torch.set_num_threads(8)
    gen_args_fields()
    gen("t4b3_mixed", 4, 3, seed=71, done_kind="mixed", zero_state=False)
    print("fixtures written to", OUT)


if __name__ == "__main__":
    main()
