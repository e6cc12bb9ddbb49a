"""Rainbow measurements on cuda:0 (not a gate; bench.py stays the flagship benchmark).

  1. the fused loss launch (ops.rainbow_loss_fwd_bwd) at B = 32, A = 6, N = 51 against the
     reference block's own torch ops (rainbow_atari_oc.py:655-701 + loss.backward(), restated
     below) on the same GPU and inputs: eager calls between two device synchronises, and the fused
     launch also as a replayed hipGraph of 100 launches;
  2. ops.PrioritizedReplay add / sample / update_priorities at capacity 1M, B = 32, per call
     (eager, and add + sample + update as one replayed graph), against a host sum tree walked by
     Python loops as the reference's classes do (:338-499, restated below) on this box's CPU;
  3. env steps per second of RainbowTrainer, C51Trainer and DQNTrainer (config 5) at the config-5
     sizes (SpaceInvaders obj-mode, 1 env, 1M-transition replay, batch 32, train_frequency 4) in
     the training phase.
Every case runs twice, alternating; both runs are reported.

    python tools/bench_rainbow.py [--steps K] [--warmup W] [--skip-trainer]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from oc_cleanrl_amd import ops  # noqa: E402
from oc_cleanrl_amd.c51 import C51Args, C51Trainer  # noqa: E402
from oc_cleanrl_amd.dqn import DQNArgs, DQNTrainer  # noqa: E402
from oc_cleanrl_amd.rainbow import RainbowArgs, RainbowTrainer  # noqa: E402


def dist(value, adv, A, N):
    adv = adv.view(-1, A, N)
    return torch.softmax(value.view(-1, 1, N) + adv - adv.mean(dim=1, keepdim=True), dim=2)


def torch_block(value, adv, v_no, a_no, v_nt, a_nt, support, actions, rewards, dones, weights,
                gamma_n, v_min, v_max):
    """The reference's loss block as torch ops (the per-sample index_add_ loop included) and its
    backward; returns (d loss / d value, d loss / d advantage, loss_per_sample)."""
    B, N = value.shape
    A = adv.shape[1] // N
    rows = torch.arange(B, device=value.device)
    value, adv = value.detach().requires_grad_(True), adv.detach().requires_grad_(True)
    with torch.no_grad():
        best = torch.argmax((dist(v_no, a_no, A, N) * support).sum(2), 1)
        next_pmfs = dist(v_nt, a_nt, A, N)[rows, best]
        next_atoms = rewards.view(B, 1) + gamma_n * support * (1 - dones.view(B, 1))
        b = (next_atoms.clamp(v_min, v_max) - v_min) / ((v_max - v_min) / (N - 1))
        lo, up = b.floor().clamp(0, N - 1), b.ceil().clamp(0, N - 1)
        m_lo = (up + (lo == b).float() - b) * next_pmfs
        m_up = (b - lo) * next_pmfs
        target = torch.zeros_like(next_pmfs)
        for i in range(B):
            target[i].index_add_(0, lo[i].long(), m_lo[i])
            target[i].index_add_(0, up[i].long(), m_up[i])
    pred = dist(value, adv, A, N)[rows, actions]
    per_sample = -(target * pred.clamp(min=1e-5, max=1 - 1e-5).log()).sum(1)
    (per_sample * weights).mean().backward()
    return value.grad, adv.grad, per_sample.detach()


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def graph_of(fn, n):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for _ in range(n):
            fn()
    g.replay()
    return g


def bench_loss(dev, B=32, A=6, N=51):
    rng = np.random.default_rng(0)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)  # noqa: E731
    heads = [f(rng.standard_normal((B, n))) for n in (N, A * N) * 3]
    support = torch.linspace(-10, 10, N).to(dev)
    actions = torch.from_numpy(rng.integers(0, A, B)).to(dev)
    rewards, dones = f(rng.choice([-1.0, 0.0, 1.0], B)), f(rng.random(B) < 0.2)
    weights = f(rng.uniform(0.1, 1.0, B))
    out = dict(dvalue=torch.empty_like(heads[0]), dadvantage=torch.empty_like(heads[1]),
               loss_per_sample=torch.empty(B, device=dev), stats=torch.empty(2, device=dev))
    torch.use_deterministic_algorithms(False)  # index_add_ on the GPU is an atomic scatter
    gamma_n = 0.99 ** 3
    fused = lambda: ops.rainbow_loss_fwd_bwd(*heads, support, actions, rewards, dones, weights,  # noqa: E731
                                             gamma_n, -10.0, 10.0, **out)
    ref = lambda: torch_block(*heads, support, actions, rewards, dones, weights, gamma_n, -10.0,  # noqa: E731
                              10.0)
    for _ in range(20):
        fused()
        dv, da, _ = ref()
    torch.cuda.synchronize()
    err = float((out["dadvantage"] - da).abs().max() / da.abs().max())
    runs = [(timed(fused, 2000), timed(ref, 30)) for _ in range(2)]  # alternating
    g = graph_of(fused, 100)
    return {"shape": {"B": B, "A": A, "N": N},
            "fused_eager_us_per_call": [round(a, 2) for a, _ in runs],
            "torch_block_eager_us_per_call": [round(b, 1) for _, b in runs],
            "fused_graph_us_per_launch": [round(timed(g.replay, 50) / 100, 2) for _ in range(2)],
            "dadvantage_max_diff_rel": err}


class HostReplay:
    """The reference's host replay restated for timing: a numpy f32 sum tree, Python loops."""

    def __init__(self, capacity, obs_shape):
        self.capacity, self.tree = capacity, np.zeros(2 * capacity - 1, np.float32)
        self.obs = np.zeros((capacity,) + obs_shape, np.uint8)
        self.next_obs = np.zeros_like(self.obs)
        self.pos = self.size = 0

    def update(self, idx, value):
        t = idx + self.capacity - 1
        self.tree[t] = value
        t = (t - 1) // 2
        while t >= 0:
            self.tree[t] = self.tree[2 * t + 1] + self.tree[2 * t + 2]
            t = (t - 1) // 2

    def add(self, obs, next_obs):
        self.obs[self.pos], self.next_obs[self.pos] = obs, next_obs
        self.update(self.pos, 1.0)
        self.pos = (self.pos + 1) % self.capacity
        self.size = min(self.size + 1, self.capacity)

    def sample(self, B, dev):
        seg, idx = self.tree[0] / B, []
        for i in range(B):
            v, t = np.random.uniform(seg * i, seg * (i + 1)), 0
            while 2 * t + 1 < len(self.tree):
                left = 2 * t + 1
                if v <= self.tree[left]:
                    t = left
                else:
                    v -= self.tree[left]
                    t = left + 1
            idx.append(t - (self.capacity - 1))
        probs = np.array([self.tree[i + self.capacity - 1] for i in idx])
        w = (self.size * probs / self.tree[0]) ** -0.4
        return (torch.from_numpy(self.obs[idx]).to(dev), torch.from_numpy(self.next_obs[idx]).to(dev),
                torch.from_numpy(w / w.max()).to(dev), idx)

    def update_priorities(self, idx, loss_dev):
        p = np.abs(loss_dev.detach().cpu().numpy()) + 1e-6
        for i, v in zip(idx, p):
            self.update(i, v ** 0.5)


def bench_replay(dev, capacity=1_000_000, B=32, obs_shape=(4, 12), fill=5000):
    rb = ops.PrioritizedReplay(capacity, obs_shape, dev, 3, 0.99, 0.5, 0.4, 1e-6,
                               total_timesteps=1e7, obs_dtype=torch.bfloat16, seed=1)
    host = HostReplay(capacity, obs_shape)
    obs = torch.rand((1,) + obs_shape, device=dev).bfloat16()
    act = torch.zeros(1, dtype=torch.int64, device=dev)
    rew, done = torch.ones(1, device=dev), torch.zeros(1, device=dev)
    hobs = np.zeros(obs_shape, np.uint8)
    for _ in range(fill):
        rb.add(obs, obs, act, rew, done)
        host.add(hobs, hobs)
    batch = rb.new_batch(B)
    loss = torch.rand(B, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    add = lambda: rb.add(obs, obs, act, rew, done)  # noqa: E731
    smp = lambda: rb.sample(B, out=batch, step=step)  # noqa: E731
    upd = lambda: rb.update_priorities(batch["indices"], loss)  # noqa: E731

    def host_round():
        t0 = time.perf_counter()
        host.add(hobs, hobs)
        t1 = time.perf_counter()
        *_, idx = host.sample(B, dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host.update_priorities(idx, loss)
        return np.array([t1 - t0, t2 - t1, time.perf_counter() - t2]) * 1e6

    def all3():
        add(), smp(), upd()

    for _ in range(20):
        all3()
    g = graph_of(all3, 10)
    res = {"capacity": capacity, "B": B}
    for run in range(2):  # alternating
        res[f"run{run}"] = {
            "device_eager_us": {n: round(timed(f, 1000), 2) for n, f in
                                (("add", add), ("sample", smp), ("update_priorities", upd))},
            "device_graph_us_add_sample_update": round(timed(g.replay, 100) / 10, 2),
            "host_us": dict(zip(("add", "sample", "update_priorities"),
                                np.mean([host_round() for _ in range(50)], 0).round(1).tolist()))}
    return res


def bench_trainer(cls, args, dev, steps, warmup):
    tr = cls(args, dev, log=False)
    tr.steps(args.learning_starts + warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.steps(steps)
    torch.cuda.synchronize()
    return round(steps / (time.perf_counter() - t0), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--skip-trainer", action="store_true")
    o = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"loss_kernel": bench_loss(dev), "replay": bench_replay(dev)}
    if not o.skip_trainer:
        kw = dict(env_id="ALE/SpaceInvaders-v5", obs_mode="obj", num_envs=1, buffer_size=1_000_000,
                  learning_starts=1000, total_timesteps=10_000_000, save_model=False)
        cases = (("rainbow", RainbowTrainer, RainbowArgs), ("c51", C51Trainer, C51Args),
                 ("dqn_config5", DQNTrainer, DQNArgs))
        out["trainer_env_steps_per_sec"] = {
            n: [bench_trainer(c, a(**kw), dev, o.steps, o.warmup) for _ in range(1)]
            for n, c, a in cases}
        for n, c, a in cases:  # the second, alternating run
            out["trainer_env_steps_per_sec"][n].append(bench_trainer(c, a(**kw), dev, o.steps,
                                                                     o.warmup))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
