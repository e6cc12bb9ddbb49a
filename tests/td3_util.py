"""What the TD3 / DDPG tests share, in plain torch / NumPy (cleanrl/td3_continuous_action.py,
ddpg_continuous_action.py):

  * stub_parameters / CASES / load_update: the update fixtures' parameters (a seeded CPU randn, the
    same bits on any machine, so they are not stored) and arrays (tests/golden/gen_golden_td3.py);
  * update_ref: the package's modules run through the scripts' update in plain torch, any dtype;
  * the NumPy twins of the library's streams: the replay's (row, env) indices, the Philox words of
    the acting / target streams, Box-Muller in f32 and f64;
  * StubEnv: a device env with A = 3, a non-zero action bias, terminations and truncations.
"""
from __future__ import annotations

import numpy as np
import torch

from contppo_util import philox4x32_10  # noqa: F401  (the Philox rounds in Python integers)
from lstm_util import FLOOR, bound, check, rel_err  # noqa: F401  (re-exported for the tests)
from rnd_util import MASK64, splitmix64

M32 = 0xFFFFFFFF
CONT_REPLAY_KEY = 0x7D3C0A7B5E91F2A3
TD3_ACT_KEY = 0x7D3AC7E5B1F00D42
TD3_TARGET_KEY = 0x7D37A26E7C11A9B5

# the update fixtures: (B, A, D), the Box's bounds, and the hyper-parameters they were run with
CASES = [(64, 1, 3), (33, 6, 5)]
BOUNDS = {1: ([-2.0], [2.0]),
          6: ([-1.0, -2.0, -0.5, -1.25, -3.0, -1.0], [1.5, 2.5, 1.0, 0.75, 1.0, 2.0])}
# (no saturated action +- the clipped noise falls on the scalar bounds -1 / 1.5)
HYPER = dict(gamma=0.99, policy_noise=0.5, noise_clip=0.5, tau=0.005)
NEAR = 1e-4
NETS = ("actor", "qf1", "qf2")
SKIP_GRADS = ("fc2.weight",)  # 65,536 elements each: fc2.bias and fc1.weight pin their factors


def stub_parameters(module, seed: int, gain: float = 1.0, near=None):
    """Overwrite the module's parameters in named_parameters() order with a seeded CPU
    generator's draws: randn * gain / sqrt(fan-in) (biases: 0.02 gain randn). near: the draws
    are scaled by 0.05 and added to that module's parameters (a twin close to it)."""
    g = torch.Generator().manual_seed(seed)
    base = dict(near.named_parameters()) if near is not None else {}
    with torch.no_grad():
        for k, p in module.named_parameters():
            if p.dim() == 2:
                v = gain * torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5
            else:
                v = 0.02 * gain * torch.randn(p.shape, generator=g)
            p.copy_(base[k] + 0.05 * v if near is not None else v)
    return module


def stub_networks(make, B: int, A: int, twin: bool):
    """The six (four) networks with their stub parameters: make(name) constructs one ("actor" or
    "q"). The targets are stubs of their own; the actors' gain saturates tanh on some rows."""
    s = 1000 * B + 10 * A
    nets = {"actor": stub_parameters(make("actor"), s + 1, 2.0),
            "target_actor": stub_parameters(make("actor"), s + 2, 2.0),
            "qf1": stub_parameters(make("q"), s + 3, 2.0),
            "qf1_target": stub_parameters(make("q"), s + 4, 2.0)}
    if twin:
        nets["qf2"] = stub_parameters(make("q"), s + 5, 2.0)
        # close to qf1_target, so that min(q1t, q2t) takes both
        nets["qf2_target"] = stub_parameters(make("q"), s + 6, 2.0, near=nets["qf1_target"])
    return nets


def stub_batch(B: int, A: int, D: int) -> dict:
    """The seeded batch of a fixture case: dones cycle 1, 0, 0; the target noise z is a seeded
    randn (policy_noise 0.5 against noise_clip 0.5: about a third of it is clipped)."""
    g = torch.Generator().manual_seed(B + 7 * A)
    low, high = (torch.tensor(v) for v in BOUNDS[A])
    t = {"obs": torch.randn(B, D, generator=g), "next_obs": torch.randn(B, D, generator=g),
         "actions": low + (high - low) * torch.rand(B, A, generator=g),
         "rewards": torch.randn(B, generator=g),
         "dones": (torch.arange(B) % 3 == 0).float(), "low": low, "high": high}
    torch.manual_seed(B + 7 * A)
    t["z"] = torch.randn_like(t["actions"])
    return t


def package_networks(B: int, A: int, D: int, twin: bool) -> dict:
    from oc_cleanrl_amd import td3

    spec = td3.box_spec(D, *BOUNDS[A])
    return stub_networks(lambda k: td3.Actor(spec) if k == "actor" else td3.QNetwork(spec),
                         B, A, twin)


def grad_names(nets: dict):
    """(net, parameter) of every gradient a fixture holds, in order."""
    return [(n, k) for n in NETS if n in nets for k, _ in nets[n].named_parameters()
            if k not in SKIP_GRADS]


def update_ref(nets: dict, t: dict, dtype, twin: bool, h: dict = HYPER) -> dict:
    """The scripts' update (td3 :238-274 / ddpg :215-238) on deep copies of `nets` cast to dtype,
    in plain torch through the modules' script-shaped forward(x, a), without optimizer steps:
    the tensors the fixtures hold."""
    import copy

    n = {k: copy.deepcopy(v).to(dtype) for k, v in nets.items()}
    c = {k: v.to(dtype) for k, v in t.items()}
    ta, ac = n["target_actor"], n["actor"]
    low0, high0 = float(t["low"][0]), float(t["high"][0])
    with torch.no_grad():
        if twin:
            noise = (c["z"] * h["policy_noise"]).clamp(-h["noise_clip"], h["noise_clip"]) \
                * ta.action_scale
            na = (ta(c["next_obs"]) + noise).clamp(low0, high0)
            nq = torch.min(n["qf1_target"](c["next_obs"], na), n["qf2_target"](c["next_obs"], na))
        else:
            na = ta(c["next_obs"])
            nq = n["qf1_target"](c["next_obs"], na)
        y = c["rewards"].flatten() + (1 - c["dones"].flatten()) * h["gamma"] * nq.view(-1)
    out = {"next_actions": na, "next_q_value": y}
    qs = [n["qf1"](c["obs"], c["actions"])] + ([n["qf2"](c["obs"], c["actions"])] if twin else [])
    for q in qs:
        q.retain_grad()
    losses = [torch.nn.functional.mse_loss(q.view(-1), y) for q in qs]
    sum(losses).backward()
    out["dq1"] = qs[0].grad.view(-1)
    if twin:
        out["dq2"] = qs[1].grad.view(-1)
    grads = {("qf1", k): p.grad.clone() for k, p in n["qf1"].named_parameters()}
    if twin:
        grads.update({("qf2", k): p.grad.clone() for k, p in n["qf2"].named_parameters()})
    mu = ac.fc_mu(ac.hidden(c["obs"]))
    mu.retain_grad()
    actor_loss = -n["qf1"](c["obs"], torch.tanh(mu) * ac.action_scale + ac.action_bias).mean()
    actor_loss.backward()
    out["dmu"] = mu.grad
    grads.update({("actor", k): p.grad for k, p in ac.named_parameters()})
    out["losses"] = torch.stack(losses + [actor_loss]).detach()
    out["grads"] = torch.cat([grads[k].reshape(-1) for k in grad_names(nets)])
    tau = h["tau"]
    out["polyak"] = torch.cat([
        (tau * p.data + (1 - tau) * tp.data).reshape(-1)
        for p, tp in ((ac.fc_mu.bias, ta.fc_mu.bias), (n["qf1"].fc3.weight, n["qf1_target"].fc3.weight))])
    return {k: v.detach() for k, v in out.items()}


FIXTURE_KEYS = ("next_actions", "next_q_value", "losses", "dq1", "dq2", "dmu", "polyak", "grads")


def fixture_name(algo: str, B: int, A: int) -> str:
    return f"{algo}_update_B{B}_A{A}.npz"


def assert_branches(t: dict, nets: dict, twin: bool, h: dict = HYPER):
    """The rows a TD3 fixture needs, asserted on the CPU: the target noise on both sides of both
    noise_clip bounds, the unclamped target action on both sides of both scalar action bounds,
    q1t on both sides of q2t, dones 0 and 1 -- and nothing within NEAR of a bound."""
    ta = nets["target_actor"]
    assert set(t["dones"].tolist()) == {0.0, 1.0}
    if not twin:
        return
    with torch.no_grad():
        zn = t["z"].double() * h["policy_noise"]
        c = h["noise_clip"]
        assert (zn < -c).any() and ((zn > -c) & (zn < c)).any() and (zn > c).any()
        assert float(torch.minimum((zn - c).abs(), (zn + c).abs()).min()) > NEAR
        d = ta.double()
        raw = d(t["next_obs"].double()) + zn.clamp(-c, c) * d.action_scale
        ta.float()
        lo, hi = float(t["low"][0]), float(t["high"][0])
        assert (raw < lo).any() and ((raw > lo) & (raw < hi)).any() and (raw > hi).any()
        assert float(torch.minimum((raw - lo).abs(), (raw - hi).abs()).min()) > NEAR
        na = raw.clamp(lo, hi).float()
        dq = nets["qf1_target"](t["next_obs"], na) - nets["qf2_target"](t["next_obs"], na)
        assert (dq < -NEAR).any() and (dq > NEAR).any()


# ---- the streams -----------------------------------------------------------------------------------------
def replay_indices_ref(seed: int, counter: int, B: int, pos: int, full: bool, size: int, E: int):
    """ContReplayBuffer.sample's (row, env) pairs [B, 2] at sample counter `counter`."""
    base = splitmix64((seed & MASK64) ^ CONT_REPLAY_KEY)
    upper = size if full else max(min(pos, size), 1)
    out = np.empty((B, 2), np.int64)
    for b in range(B):
        h = splitmix64((base + counter * 0x100000001B3 + b) & MASK64)
        out[b] = (h % upper, splitmix64(h) % E)
    return out


def philox_words(key: int, sub: int, rows: int, A: int):
    """Words 0 and 1 of the block (r * 64 + a, sub) under `key`, [rows, A, 2] (Python ints in
    uint64)."""
    out = np.empty((rows, A, 2), np.uint64)
    for r in range(rows):
        for a in range(A):
            blk = r * 64 + a
            w = philox4x32_10([blk & M32, blk >> 32, sub & M32, (sub >> 32) & M32],
                              [key & M32, key >> 32])
            out[r, a] = w[:2]
    return out


def act_words(seed: int, t: int, E: int, A: int):
    return philox_words((seed & MASK64) ^ TD3_ACT_KEY, t, E, A)


def target_words(seed: int, counter: int, B: int, A: int):
    return philox_words((seed & MASK64) ^ TD3_TARGET_KEY, counter, B, A)


def unit24(w, dtype=np.float32):
    return ((w >> np.uint64(8)).astype(dtype) * dtype(2.0 ** -24)).astype(dtype)


def box_muller(words, dtype=np.float32):
    """The kernels' Box-Muller on (word 0, word 1): u1 = ((w0 >> 8) + 1) 2^-24 in (0, 1], u2 =
    (w1 >> 8) 2^-24, z = sqrt(-2 log u1) cos(2 pi u2) -- with dtype float32 in the kernel's f32
    operations (2 pi as its f32 constant), with float64 the twin."""
    f = dtype
    u1 = (((words[..., 0] >> np.uint64(8)).astype(f) + f(1.0)) * f(2.0 ** -24)).astype(f)
    u2 = unit24(words[..., 1], f)
    two_pi = f(np.float32(6.2831855)) if f is np.float32 else f(2.0 * np.pi)
    r = np.sqrt((f(-2.0) * np.log(u1)).astype(f)).astype(f)
    return (r * np.cos((two_pi * u2).astype(f)).astype(f)).astype(f)


# ---- a device env with A = 3 ----------------------------------------------------------------------------------
class StubEnv:
    """PendulumVecEnv(raw=True)'s interface on torch ops (capturable): D = 5, A = 3, bounds with a
    non-zero bias; env e terminates every 5 + e steps and is truncated every 7 steps; the
    observation is a fixed mixing of the action and the step count, a terminal observation is the
    next one + 100."""
    n_actions = 3
    action_low, action_high = (-1.0, -2.0, -0.5), (1.5, 2.0, 1.0)

    def __init__(self, num_envs: int, device):
        self.E, dev, f = num_envs, torch.device(device), torch.float32
        self.frame = torch.zeros((num_envs, 5), dtype=f, device=dev)
        self.final_frame = torch.zeros((num_envs, 5), dtype=f, device=dev)
        self.reward = torch.zeros(num_envs, dtype=f, device=dev)
        self.done = torch.zeros(num_envs, dtype=f, device=dev)
        self.terminated = torch.zeros(num_envs, dtype=f, device=dev)
        self.t = torch.zeros(num_envs, dtype=f, device=dev)       # steps in the episode
        self.ret = torch.zeros(num_envs, dtype=f, device=dev)
        self.ep = torch.zeros(3, dtype=torch.float64, device=dev)  # return sum, length sum, count
        self.period = torch.arange(num_envs, dtype=f, device=dev) + 5
        g = torch.Generator().manual_seed(5)
        self.mix = torch.randn(3, 5, generator=g).to(dev)

    def _obs(self):
        return torch.tanh(self.t[:, None] * 0.3 + torch.arange(5, device=self.t.device))

    def reset(self):
        self.frame.copy_(self._obs())
        return self.frame

    def step(self, actions, step_offset: int = 0):
        self.t.add_(1)
        nxt = self._obs() + 0.1 * (actions @ self.mix)
        self.reward.copy_(-(actions ** 2).sum(1) + 0.1 * self.t)
        self.ret.add_(self.reward)
        self.terminated.copy_((self.t % self.period == 0).float())
        self.done.copy_(torch.maximum(self.terminated, (self.t % 7 == 0).float()))
        self.final_frame.copy_(nxt + 100.0)
        self.ep.add_(torch.stack([(self.ret * self.done).sum().double(),
                                  (self.t * self.done).sum().double(), self.done.sum().double()]))
        keep = 1 - self.done
        self.t.mul_(keep)
        self.ret.mul_(keep)
        self.frame.copy_(torch.where(self.done[:, None] > 0, self._obs(), nxt))

    def advance(self, n: int):
        pass

    def pop_episode_stats(self):
        s = self.ep.tolist()
        self.ep.zero_()
        return s
