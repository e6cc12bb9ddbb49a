"""Generate the Rainbow fixtures under tests/golden/ FROM THE REFERENCE ITSELF.

Like gen_golden_c51.py this runs only where the reference checkout is mounted read-only; only the
.npz / .json outputs are committed, no reference program text is stored.

What is executed:
  * cleanrl/architectures/rainbow.py is imported as a module (NoisyLinear,
    NoisyDuelingDistributionalPPObj: pure torch);
  * cleanrl/rainbow_atari_oc.py is read as text by line range, dedented, compiled and exec'd:
      :239-327  NoisyLinear + NoisyDuelingDistributionalNetwork (the pixel network)
      :338-499  SumSegmentTree, MinSegmentTree, PrioritizedReplayBuffer
      :655-701  the train step's loss block, with `q_network` / `target_network` = the reference's
                own NoisyDuelingDistributionalPPObj whose `network` is the identity and whose
                `value_head` / `advantage_head` return seeded tensors (the online net's on
                `observations` with requires_grad); then `loss.backward()`.

Fixtures (each records the numpy and torch versions that made it):
  rainbow_args_fields.json   [name, default] of the script's Args dataclass, declaration order
  rainbow_init_{obj,pixels}.npz  a seeded network (A = 6, N = 51): state-dict keys, shapes and
                        checksums (the noise buffers included), the support, and the forward (with
                        the noise the constructor drew) on two seeded inputs
  per_addseq_c{C}_n{n}.npz   a scripted add sequence with interleaved update_priorities calls:
                        after every add all buffers, pos, size, max_priority and the tree; after
                        every update the tree, max_priority and a float64 twin of each new leaf
  per_sample_c{C}.npz   one buffer state, the float64 upperbounds one sample() call drew, and its
                        indices, rows, probs and weights at two betas with a float64 twin
  rainbow_loss_{name}.npz    inputs, best_actions, target_pmfs, loss_per_sample, loss, q_values
                        (:710-713), dvalue, dadvantage; and under the same names + "64" the float64
                        twin: the same block on the same f32 inputs run in float64

    python tests/golden/gen_golden_rainbow.py
"""
from __future__ import annotations

import ast
import collections
import json
import math
import sys
import textwrap
import types
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent
SCRIPT = REF / "cleanrl" / "rainbow_atari_oc.py"
NET_LINES = (239, 327)
REPLAY_LINES = (338, 499)
LOSS_LINES = (655, 701)

sys.dont_write_bytecode = True
sys.path.insert(0, str(REF / "cleanrl"))
from architectures.rainbow import NoisyDuelingDistributionalPPObj  # noqa: E402  (the reference's)

VERSIONS = dict(numpy_version=np.array(np.__version__), torch_version=np.array(torch.__version__))


def block(lines):
    src = SCRIPT.read_text().splitlines()[lines[0] - 1:lines[1]]
    return compile(textwrap.dedent("\n".join(src)), f"{SCRIPT}:{lines[0]}-{lines[1]}", "exec")


NET_NS = dict(torch=torch, nn=nn, F=F, math=math, np=np)
exec(block(NET_LINES), NET_NS)
REPLAY_NS = dict(np=np, torch=torch, deque=collections.deque, collections=collections,
                 PrioritizedBatch=lambda **kw: types.SimpleNamespace(**kw))
exec(block(REPLAY_LINES), REPLAY_NS)
LOSS_CODE = block(LOSS_LINES)


class Space:
    def __init__(self, shape=None, n=None):
        self.shape = shape
        self.n = n


class Envs:
    """The vector env's spaces as the networks read them (num_envs = 1)."""

    def __init__(self, obs_shape, n_actions):
        self.observation_space = Space(shape=(1,) + tuple(obs_shape))
        self.single_action_space = Space(shape=(), n=n_actions)


# ---- Args ---------------------------------------------------------------------------------------
def gen_args_fields():
    cls = next(n for n in ast.parse(SCRIPT.read_text()).body
               if isinstance(n, ast.ClassDef) and n.name == "Args")
    fields = []
    for s in cls.body:
        if not isinstance(s, ast.AnnAssign):
            continue
        try:
            default = ast.literal_eval(s.value)
        except ValueError:  # exp_name: the script's file name without ".py"
            assert s.target.id == "exp_name"
            default = SCRIPT.stem
        fields.append([s.target.id, default])
    (OUT / "rainbow_args_fields.json").write_text(json.dumps(fields, indent=1) + "\n")


# ---- networks -----------------------------------------------------------------------------------
def gen_init(kind, seed=1, A=6, N=51):
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    if kind == "pixels":
        net = NET_NS["NoisyDuelingDistributionalNetwork"](Envs((4, 84, 84), A), N, -10, 10)
        x = rng.integers(0, 256, (2, 4, 84, 84)).astype(np.float32)
        extra = {}
    else:
        enc, dec = (32, 64), (64,)
        net = NoisyDuelingDistributionalPPObj(Envs((4, 12), A), N, -10, 10, encoder_dims=enc,
                                              decoder_dims=dec)
        x = rng.integers(0, 256, (2, 4, 12)).astype(np.float32)
        extra = dict(encoder_dims=np.array(enc), decoder_dims=np.array(dec))
    with torch.no_grad():
        q_dist = net(torch.from_numpy(x))
    sd = net.state_dict()
    np.savez_compressed(
        OUT / f"rainbow_init_{kind}.npz", seed=seed, n_actions=A, n_atoms=N, x=x,
        keys=np.array(list(sd)), shapes=np.array([json.dumps(list(v.shape)) for v in sd.values()]),
        sums=np.array([[float(v.double().sum()), float(v.double().abs().sum())]
                       for v in sd.values()]),
        support=sd["support"].numpy(), delta_z=np.array(net.delta_z), q_dist=q_dist.numpy(),
        **extra, **VERSIONS)


# ---- prioritized replay -------------------------------------------------------------------------
OBS_SHAPE = (2, 3)


def snapshot(rb):
    return dict(obs=rb.buffer_obs.copy(), next_obs=rb.buffer_next_obs.copy(),
                actions=rb.buffer_actions.copy(), rewards=rb.buffer_rewards.copy(),
                dones=rb.buffer_dones.copy(), pos=rb.pos, size=rb.size,
                max_priority=np.float32(rb.max_priority), tree=rb.sum_tree.tree.copy())


def scripted_adds(rb, rng, steps, updates, log, ulog):
    """`steps` adds in the shapes and dtypes the training loop passes (1-element arrays of one
    env: u8 obs [1, ...], int64 actions, float64 rewards, bool terminations), with an
    update_priorities call after the adds listed in `updates`."""
    reward_values = np.array([-1.0, 0.0, 0.0, 1.0, 0.5, 0.1, 2.5, -0.3], np.float32)
    for t in range(steps):
        obs = rng.integers(0, 256, (1,) + OBS_SHAPE).astype(np.uint8)
        nxt = rng.integers(0, 256, (1,) + OBS_SHAPE).astype(np.uint8)
        action = rng.integers(0, 6, 1).astype(np.int64)
        reward = rng.choice(reward_values, 1).astype(np.float64)
        done = np.array([rng.random() < 0.22])
        rb.add(obs, action, reward, nxt, done)
        s = snapshot(rb)
        s.update(in_obs=obs[0], in_next_obs=nxt[0], in_action=action[0],
                 in_reward=np.float32(reward[0]), in_done=done[0])
        log.append(s)
        if t in updates and rb.size >= 2:
            k, scale = updates[t]
            idx = rng.integers(0, rb.size, k)
            idx[-1] = idx[0]  # a duplicated index: the last occurrence wins
            pri = (rng.standard_normal(k) * scale).astype(np.float32)
            rb.update_priorities(list(idx), pri)
            leaf64 = (np.abs(pri.astype(np.float64)) + rb.eps) ** rb.alpha
            ulog.append(dict(after_add=t, indices=idx.astype(np.int64), priorities=pri,
                             leaf64=leaf64, tree=rb.sum_tree.tree.copy(),
                             max_priority=np.float32(rb.max_priority)))


def gen_addseq(capacity, n_step, alpha, seed, steps=40):
    rng = np.random.default_rng(seed)
    gamma = 0.99
    rb = REPLAY_NS["PrioritizedReplayBuffer"](capacity, OBS_SHAPE, "cpu", n_step, gamma,
                                              alpha=alpha, beta=0.4, eps=1e-6)
    log, ulog = [], []
    # the first updates stay below 1 (max_priority remains 1.0: adds keep writing exactly 1), the
    # later ones raise it
    updates = {11: (3, 0.2), 19: (4, 0.2), 27: (4, 3.0), 35: (5, 3.0)}
    scripted_adds(rb, rng, steps, updates, log, ulog)
    assert max(s["size"] for s in log) == capacity and any(s["dones"].any() for s in log)
    assert len(ulog) == len(updates) and float(ulog[-1]["max_priority"]) > 1.0
    assert float(ulog[0]["max_priority"]) == 1.0
    out = {k: np.stack([np.asarray(s[k]) for s in log]) for k in log[0]}
    for j, u in enumerate(ulog):  # ragged batch sizes: one set of arrays per update
        for k, v in u.items():
            out[f"upd{j}_{k}"] = np.asarray(v)
    out.update(capacity=capacity, n_step=n_step, alpha=alpha, gamma=gamma, eps=1e-6,
               n_updates=len(ulog), gamma_pows=np.array([gamma ** i for i in range(n_step)]),
               **VERSIONS)
    np.savez_compressed(OUT / f"per_addseq_c{capacity}_n{n_step}.npz", **out)
    return rb


def gen_sample(capacity, n_step, B, seed):
    rng = np.random.default_rng(seed)
    rb = REPLAY_NS["PrioritizedReplayBuffer"](capacity, OBS_SHAPE, "cpu", n_step, 0.99, alpha=0.5,
                                              beta=0.4, eps=1e-6)
    log, ulog = [], []
    scripted_adds(rb, rng, 30, {12: (3, 0.7), 22: (4, 2.0)}, log, ulog)
    tree = rb.sum_tree.tree
    leaves = tree[capacity - 1:].astype(np.float64)
    bounds = np.cumsum(leaves)
    drawn = []
    real_uniform = np.random.uniform

    def recording(a, b):
        drawn.append((np.float32(a), np.float32(b), real_uniform(a, b)))
        assert isinstance(a, np.float32) and isinstance(b, np.float32)  # segment math stays f32
        return drawn[-1][2]

    np.random.seed(seed)
    res = {}
    for j, beta in enumerate((0.4, 0.85)):
        rb.beta = beta
        ubs = [d[2] for d in drawn]
        np.random.uniform = recording if j == 0 else (lambda a, b, it=iter(ubs): next(it))
        try:
            batch = rb.sample(B)
        finally:
            np.random.uniform = real_uniform
        idx = np.array(batch.indices, np.int64)
        probs = np.array([tree[i + capacity - 1] for i in idx])
        assert probs.dtype == np.float32 and (probs > 0).all()
        w = batch.weights.numpy().reshape(-1)
        assert w.dtype == np.float32
        w64 = (rb.size * probs.astype(np.float64) / np.float64(tree[0])) ** -beta
        res[j] = dict(beta=beta, indices=idx, probs=probs, weights=w, weights64=w64 / w64.max(),
                      obs=batch.observations.numpy(), next_obs=batch.next_observations.numpy(),
                      actions=batch.actions.numpy().reshape(-1),
                      rewards=batch.rewards.numpy().reshape(-1),
                      dones=batch.dones.numpy().reshape(-1))
    assert np.array_equal(res[0]["indices"], res[1]["indices"])
    ub = np.array([d[2] for d in drawn], np.float64)
    assert len(ub) == B and ub.dtype == np.float64
    # no upperbound near a cumulative leaf boundary: a summation detail never decides an index
    gap = np.abs(ub[:, None] - bounds[None, :]).min() / float(tree[0])
    assert gap > 1e-6, gap
    s = snapshot(rb)
    out = {"buf_" + k: np.asarray(v) for k, v in s.items()}
    out.update(upperbounds=ub, seg_lo=np.array([d[0] for d in drawn]),
               seg_hi=np.array([d[1] for d in drawn]), capacity=capacity, B=B, **VERSIONS)
    for j in res:
        for k, v in res[j].items():
            out[f"b{j}_{k}"] = np.asarray(v)
    np.savez_compressed(OUT / f"per_sample_c{capacity}.npz", **out)
    print(f"per_sample_c{capacity}: size {rb.size}, total {float(tree[0])!r}, boundary gap {gap:.2g}, "
          f"indices {res[0]['indices'].tolist()}")


# ---- loss ---------------------------------------------------------------------------------------
class Identity(nn.Module):
    def forward(self, x):
        return x


class StubHead(nn.Module):
    """Stands in for value_head / advantage_head: the seeded tensor for `observations` (trunk
    output 0) or for `next_observations` (trunk output 1)."""

    def __init__(self, on_obs, on_next):
        super().__init__()
        self.on_obs, self.on_next = on_obs, on_next

    def forward(self, h):
        return self.on_next if float(h[0, 0]) > 0.5 else self.on_obs


def stub_net(v_obs, a_obs, v_next, a_next, A, N, v_min, v_max, dtype):
    net = NoisyDuelingDistributionalPPObj(Envs((1, 1), A), N, v_min, v_max, encoder_dims=(1,),
                                          decoder_dims=(1,))
    net = net.to(dtype)  # the f32 linspace support, as it is or widened exactly to f64
    if dtype == torch.float64:
        net.delta_z = float(np.float32(net.delta_z))  # the divisor the f32 run rounds it to
    net.network = Identity()
    net.value_head = StubHead(v_obs, v_next)
    net.advantage_head = StubHead(a_obs, a_next)
    return net


def run_block(ins, A, N, v_min, v_max, gamma, n_step, dtype):
    B = ins["value"].shape[0]
    t = lambda k: torch.from_numpy(ins[k]).to(dtype)  # noqa: E731
    value, adv = t("value").requires_grad_(True), t("advantage").requires_grad_(True)
    q_network = stub_net(value, adv, t("value_next_online"), t("advantage_next_online"), A, N,
                         v_min, v_max, dtype)
    target_network = stub_net(None, None, t("value_next_target"), t("advantage_next_target"), A,
                              N, v_min, v_max, dtype)
    data = types.SimpleNamespace(
        observations=torch.zeros(B, 1, dtype=dtype),
        next_observations=torch.full((B, 1), 255.0, dtype=dtype),
        actions=torch.from_numpy(ins["actions"]).reshape(B, 1),
        rewards=t("rewards").reshape(B, 1), dones=torch.from_numpy(ins["dones"] != 0).reshape(B, 1),
        weights=t("weights").reshape(B, 1))
    if dtype == torch.float64:  # gamma ** n_step as the f32 run rounds it
        args = types.SimpleNamespace(gamma=float(np.float32(gamma ** n_step)), n_step=1)
    else:
        args = types.SimpleNamespace(gamma=gamma, n_step=n_step)
    args.batch_size, args.n_atoms = B, N
    ns = dict(torch=torch, data=data, args=args, q_network=q_network,
              target_network=target_network)
    exec(LOSS_CODE, ns)
    ns["loss"].backward()
    with torch.no_grad():
        q_values = (ns["pred_dist"] * q_network.support).sum(dim=1).mean()  # :710-713
    g = lambda k: ns[k].detach().numpy()  # noqa: E731
    return dict(best_actions=g("best_actions").astype(np.int64), target_pmfs=g("target_pmfs"),
                loss_per_sample=g("loss_per_sample"), loss=np.array(ns["loss"].item()),
                q_values=np.array(q_values.item()), dvalue=value.grad.numpy(),
                dadvantage=adv.grad.numpy(), pred_dist=g("pred_dist"), b=g("b"), l=g("l"),
                u=g("u"), tz=g("tz"), next_q_online=g("next_q_online"),
                support=q_network.support.numpy())


LO, HI = 1e-5, 1 - 1e-5


def loss_inputs(B, A, N, v, seed, scale, kind):
    rng = np.random.default_rng(seed)
    f = lambda *s: (rng.standard_normal(s) * scale).astype(np.float32)  # noqa: E731
    ins = dict(value=f(B, N), advantage=f(B, A * N), value_next_online=f(B, N),
               advantage_next_online=f(B, A * N), value_next_target=f(B, N),
               advantage_next_target=f(B, A * N),
               actions=rng.integers(0, A, B).astype(np.int64))
    if kind == "pong":
        rewards = rng.choice([-1.0, 0.0, 0.0, 0.0, 1.0, 2.97], B)
        dones = rng.random(B) < 0.2
    elif kind == "ties":  # integer rewards on a unit-spaced support: most b are integers
        rewards = rng.integers(-3, 4, B)
        dones = rng.random(B) < 0.5
    elif kind == "wide":
        rewards = rng.standard_normal(B) * 30
        dones = rng.random(B) < 0.2
    else:  # edges: both clamps, exact integers b on done rows, and ordinary rows
        rewards = np.array([-30.0, 30.0, -10.0, 10.0, -8.0, 0.0, 2.0, 6.0] +
                           list(rng.standard_normal(B - 8) * 4))
        dones = np.array([True, False, True, True, True, True, True, False] +
                         list(rng.random(B - 8) < 0.4))
    w = rng.uniform(0.05, 1.0, B)
    w[rng.integers(0, B)] = 1.0  # PER weights are divided by their maximum
    ins.update(rewards=rewards.astype(np.float32), dones=dones.astype(np.float32),
               weights=w.astype(np.float32))
    return ins


def gen_loss(name, B, A, N, v, gamma, n_step, seed, scale=1.0, kind="pong"):
    v_min, v_max = -v, v
    ins = loss_inputs(B, A, N, v, seed, scale, kind)
    r32 = run_block(ins, A, N, v_min, v_max, gamma, n_step, torch.float32)
    r64 = run_block(ins, A, N, v_min, v_max, gamma, n_step, torch.float64)
    assert np.array_equal(r32["support"].astype(np.float64), r64["support"])
    assert np.array_equal(r32["best_actions"], r64["best_actions"]), name
    # the double-Q action must not hang on the summation order of the expected value
    nq = r64["next_q_online"]
    top2 = np.sort(nq, axis=1)[:, -2:]
    gap = float((top2[:, 1] - top2[:, 0]).min() / np.abs(nq).max()) if A > 1 else 1.0
    assert gap > 1e-4, (name, gap)
    # no taken-action pmf near either log clamp (the clamped loss is discontinuous there)
    for r in (r32, r64):
        p = r["pred_dist"].astype(np.float64)
        rel, ab = float(np.abs(p / LO - 1).min()), float(np.abs(p - HI).min())
        assert rel > 1e-3 and ab > 1e-6, (name, rel, ab)
    b, l, tz = r32["b"], r32["l"], r32["tz"]
    frac_int = float((l == b).mean())
    if kind == "ties":
        assert (b == 0).any() and (b == N - 1).any() and frac_int > 0.5
    if kind == "edges":
        assert ins["dones"].any() and (tz == v_min).any() and (tz == v_max).any()
        inner = (tz > v_min) & (tz < v_max)
        assert (inner & (l == b)).any(), "an exact integer b off the clamps"
        assert (r32["u"] == N - 1).any() and (r32["l"] == 0).any()
    out = dict(ins, support=r32["support"], gamma=np.array(gamma), n_step=np.array(n_step),
               v_min=np.array(float(v_min)), v_max=np.array(float(v_max)), n_actions=np.array(A),
               seed=np.array(seed), **VERSIONS)
    for k in ("best_actions", "target_pmfs", "loss_per_sample", "loss", "q_values", "dvalue",
              "dadvantage"):
        out[k] = r32[k]
        if k != "best_actions":
            out[k + "64"] = r64[k]
    np.savez_compressed(OUT / f"rainbow_loss_{name}.npz", **out)
    print(f"rainbow_loss_{name}: integer b {frac_int:.2f}, online next-q gap {gap:.2g}, "
          f"loss {float(r32['loss'])!r}")


def main():
    torch.set_num_threads(8)
    gen_args_fields()
    gen_init("obj")
    gen_init("pixels")
    gen_addseq(6, 3, 0.5, seed=11)
    gen_addseq(8, 1, 0.6, seed=12)
    gen_addseq(8, 3, 0.5, seed=13)
    gen_addseq(6, 1, 0.5, seed=14)
    gen_sample(6, 3, 4, seed=21)
    gen_sample(8, 1, 8, seed=22)
    gen_loss("b32_a6_n51", 32, 6, 51, 10, 0.99, 3, seed=51)
    gen_loss("b7_a18_n101", 7, 18, 101, 100, 0.99, 3, seed=52, kind="wide")
    gen_loss("ties", 16, 3, 5, 2, 0.5, 1, seed=53, kind="ties")
    gen_loss("edges", 16, 4, 51, 10, 0.99, 3, seed=54, kind="edges")
    print("fixtures written to", OUT)


if __name__ == "__main__":
    main()
