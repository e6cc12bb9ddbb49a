"""Generate the C51 fixtures under tests/golden/ FROM THE REFERENCE ITSELF.

Like gen_golden.py this runs only where the reference checkout is mounted read-only; only the
.npz / .json outputs are committed, no reference program text is stored.

What is executed:
  * cleanrl/architectures/dqn.py is imported as a module (QNetwork_C51: pure torch);
  * the train step's loss block cleanrl/c51_atari_oc.py:339-359 (target pmf projection, taken
    action's pmf, clamped cross entropy) is read as text by line range, dedented, compiled and
    exec'd with `q_network` / `target_network` = the reference's own QNetwork_C51 whose `network`
    is replaced by a stub module returning seeded logits (the online stub's with requires_grad),
    then `loss.backward()` gives d loss / d logits.

Fixtures:
  c51_{name}.npz        inputs (logits, logits_next, atoms, actions, rewards, dones, gamma, v_min,
                        v_max), target_pmfs, old_pmfs, loss, q_values (c51_atari_oc.py:363-364),
                        dlogits and the target net's greedy next action; and under the same names
                        + "64" the float64 twin: the same block on the same f32 inputs (f32-valued
                        atoms, f32-valued gamma) run in float64
  c51_args_fields.json  [name, default] of c51_atari_oc.py's Args dataclass, declaration order
  c51_init_a6.npz       a seeded reference QNetwork_C51 (A = 6, N = 51, 4x84x84): state-dict keys,
                        shapes and checksums, the atoms buffer, and get_action's outputs on two
                        seeded u8-valued inputs

    python tests/golden/gen_golden_c51.py
"""
from __future__ import annotations

import ast
import json
import sys
import textwrap
import types
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
C51_SCRIPT = REF / "cleanrl" / "c51_atari_oc.py"
C51_LOSS_LINES = (339, 359)

sys.dont_write_bytecode = True
sys.path.insert(0, str(REF / "cleanrl"))
from architectures.dqn import QNetwork_C51  # noqa: E402  (the reference's own module)


def block(lines, script):
    src = script.read_text().splitlines()[lines[0] - 1:lines[1]]
    return compile(textwrap.dedent("\n".join(src)), f"{script}:{lines[0]}-{lines[1]}", "exec")


C51_LOSS_CODE = block(C51_LOSS_LINES, C51_SCRIPT)


class Space:
    def __init__(self, shape=None, n=None):
        self.shape = shape
        self.n = n


class Envs:
    def __init__(self, obs_shape, n_actions):
        self.observation_space = Space(shape=obs_shape)
        self.action_space = Space(shape=(), n=n_actions)


class StubLogits(nn.Module):
    """Stands in for QNetwork_C51.network: returns the seeded logits whatever the input."""

    def __init__(self, logits):
        super().__init__()
        self.logits = logits

    def forward(self, x):
        return self.logits


def stub_net(logits, A, N, v_min, v_max, dtype):
    net = QNetwork_C51(Envs((4, 84, 84), A), n_atoms=N, v_min=v_min, v_max=v_max)
    net = net.to(dtype)  # the f32 linspace atoms, as they are or widened exactly to f64
    net.network = StubLogits(logits)
    return net


def run_block(logits, logits_next, actions, rewards, dones, A, N, v_min, v_max, gamma, dtype):
    B = logits.shape[0]
    lg = torch.from_numpy(logits).to(dtype).requires_grad_(True)
    q_network = stub_net(lg, A, N, v_min, v_max, dtype)
    target_network = stub_net(torch.from_numpy(logits_next).to(dtype), A, N, v_min, v_max, dtype)
    data = types.SimpleNamespace(
        observations=torch.zeros(B, 1, dtype=dtype), next_observations=torch.zeros(B, 1, dtype=dtype),
        actions=torch.from_numpy(actions).reshape(B, 1),
        rewards=torch.from_numpy(rewards).to(dtype).reshape(B, 1),
        dones=torch.from_numpy(dones).to(dtype).reshape(B, 1))
    args = types.SimpleNamespace(gamma=gamma, v_min=v_min, v_max=v_max, n_atoms=N)
    ns = dict(torch=torch, data=data, args=args, q_network=q_network,
              target_network=target_network)
    exec(C51_LOSS_CODE, ns)
    ns["loss"].backward()
    with torch.no_grad():
        next_action, _ = target_network.get_action(data.next_observations)
        pm = torch.softmax(target_network.network(None).view(B, A, N), dim=2)
        next_q = (pm * target_network.atoms).sum(2)
        old_val = (ns["old_pmfs"] * q_network.atoms).sum(1)  # c51_atari_oc.py:363
    return dict(target_pmfs=ns["target_pmfs"].numpy(), old_pmfs=ns["old_pmfs"].detach().numpy(),
                loss=np.array(ns["loss"].item()), q_values=np.array(old_val.mean().item()),
                dlogits=lg.grad.numpy(), next_action=next_action.numpy().astype(np.int64),
                b=ns["b"].numpy(), l=ns["l"].numpy(), u=ns["u"].numpy(), next_q=next_q.numpy(),
                atoms=q_network.atoms.numpy())


LO, HI = 1e-5, 1 - 1e-5


def clamp_margins(p):
    """Nearest relative distance of any taken-action pmf to 1e-5 and absolute to 1 - 1e-5."""
    p = p.astype(np.float64)
    return float(np.abs(p / LO - 1).min()), float(np.abs(p - HI).min())


def inputs(B, A, N, seed, scale, reward_kind):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, A * N)) * scale).astype(np.float32)
    logits_next = (rng.standard_normal((B, A * N)) * scale).astype(np.float32)
    actions = rng.integers(0, A, B).astype(np.int64)
    if reward_kind == "pong":
        rewards = rng.choice([-1.0, 0.0, 0.0, 0.0, 1.0], B).astype(np.float32)
        dones = (rng.random(B) < 0.2).astype(np.float32)
    elif reward_kind == "ties":
        rewards = rng.integers(-3, 4, B).astype(np.float32)
        dones = (rng.random(B) < 0.5).astype(np.float32)
    else:  # wide returns for the +-100 support
        rewards = (rng.standard_normal(B) * 30).astype(np.float32)
        dones = (rng.random(B) < 0.2).astype(np.float32)
    return logits, logits_next, actions, rewards, dones


def gen_c51(name, B, A, N, v, gamma, seed, scale=1.0, reward_kind="pong", peaked=False):
    """One fixture; `peaked` searches seeds upward from `seed` until the reference's own taken
    action pmfs stay clear of both clamp bounds (the clamped loss is discontinuous there) with
    elements on each side of each bound."""
    v_min, v_max = -v, v
    while True:
        ins = inputs(B, A, N, seed, scale, reward_kind)
        r32 = run_block(*ins, A, N, v_min, v_max, gamma, torch.float32)
        rel, ab = clamp_margins(r32["old_pmfs"])
        p = r32["old_pmfs"]
        sides = (p < LO).any() and (p > LO).any() and (p > HI).any() and (p < HI).any()
        if rel > 1e-3 and ab > 1e-6 and (sides or not peaked):
            break
        if not peaked:
            raise AssertionError(f"{name}: a pmf sits at a clamp bound ({rel:.3g}, {ab:.3g})")
        seed += 1
    # the same block in float64 on the same f32 inputs (gamma as the f32 run rounds it)
    r64 = run_block(*ins, A, N, v_min, v_max, float(np.float32(gamma)), torch.float64)
    assert np.array_equal(r32["atoms"].astype(np.float64), r64["atoms"])
    assert np.array_equal(r32["next_action"], r64["next_action"]), name
    assert np.array_equal(r32["l"], r64["l"]) and np.array_equal(r32["u"], r64["u"]), name
    # the greedy next action must not hang on the summation order of the expected value
    top2 = np.sort(r64["next_q"], axis=1)[:, -2:]
    gap = float((top2[:, 1] - top2[:, 0]).min() / np.abs(r64["next_q"]).max()) if A > 1 else 1.0
    assert gap > 1e-4, (name, gap)
    rel64, ab64 = clamp_margins(r64["old_pmfs"])
    assert rel64 > 1e-3 and ab64 > 1e-6, (name, rel64, ab64)
    frac_int = float((r32["l"] == r32["u"]).mean())
    if reward_kind == "ties":
        b = r32["b"]
        assert (b == 0).any() and (b == N - 1).any(), "both clamp ends must be hit"
        assert frac_int > 0.5
    logits, logits_next, actions, rewards, dones = ins
    out = dict(logits=logits, logits_next=logits_next, atoms=r32["atoms"], actions=actions,
               rewards=rewards, dones=dones, gamma=np.array(gamma), v_min=np.array(float(v_min)),
               v_max=np.array(float(v_max)), n_actions=np.array(A), seed=np.array(seed))
    for k in ("target_pmfs", "old_pmfs", "loss", "q_values", "dlogits", "next_action"):
        out[k] = r32[k]
        if k != "next_action":
            out[k + "64"] = r64[k]
    np.savez_compressed(OUT / f"c51_{name}.npz", **out)
    below, above = float((p < LO).mean()), float((p > HI).mean())
    print(f"c51_{name}: seed {seed}, integer b {frac_int:.2f}, pmf < 1e-5 {below:.2f}, "
          f"> 1-1e-5 {above:.4f}, nearest to the bounds rel {rel:.2g} abs {ab:.2g}, "
          f"next-q gap {gap:.2g}, delta_z {float(r32['atoms'][1] - r32['atoms'][0])!r}")


def gen_args_fields():
    cls = next(n for n in ast.parse(C51_SCRIPT.read_text()).body
               if isinstance(n, ast.ClassDef) and n.name == "Args")
    fields = []
    for s in cls.body:
        if not isinstance(s, ast.AnnAssign):
            continue
        try:
            default = ast.literal_eval(s.value)
        except ValueError:  # exp_name: the script's file name without ".py"
            assert s.target.id == "exp_name"
            default = C51_SCRIPT.stem
        fields.append([s.target.id, default])
    (OUT / "c51_args_fields.json").write_text(json.dumps(fields, indent=1) + "\n")


def gen_init(seed=1, A=6, N=51):
    torch.manual_seed(seed)
    net = QNetwork_C51(Envs((4, 84, 84), A), n_atoms=N, v_min=-10, v_max=10)
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (2, 4, 84, 84)).astype(np.uint8)
    with torch.no_grad():
        action, pmfs = net.get_action(torch.from_numpy(x).float())
        given, pmfs_given = net.get_action(torch.from_numpy(x).float(), torch.tensor([A - 1, 0]))
    sd = net.state_dict()
    np.savez_compressed(
        OUT / "c51_init_a6.npz", seed=seed, n_actions=A, n_atoms=N, x=x, keys=np.array(list(sd)),
        shapes=np.array([json.dumps(list(v.shape)) for v in sd.values()]),
        sums=np.array([[float(v.double().sum()), float(v.double().abs().sum())]
                       for v in sd.values()]),
        atoms=sd["atoms"].numpy(), action=action.numpy().astype(np.int64), pmfs=pmfs.numpy(),
        given=given.numpy().astype(np.int64), pmfs_given=pmfs_given.numpy())


def main():
    torch.set_num_threads(8)
    gen_c51("b32_a6_n51", 32, 6, 51, 10, 0.99, seed=41)
    gen_c51("ties", 16, 3, 5, 2, 0.5, seed=42, reward_kind="ties")
    gen_c51("peaked", 32, 6, 51, 10, 0.99, seed=3, scale=6.0, peaked=True)
    gen_c51("b7_a18_n101", 7, 18, 101, 100, 0.99, seed=44, reward_kind="wide")
    gen_args_fields()
    gen_init()
    print("fixtures written to", OUT)


if __name__ == "__main__":
    main()
