"""C51 measurements on cuda:0 (not a gate; bench.py stays the flagship benchmark).

  1. the fused loss launch (ops.c51_loss_fwd_bwd) at B = 32, A = 6, N = 51 against the reference
     block's own torch ops (c51_atari_oc.py:339-359 + loss.backward(), restated below) on the same
     GPU and inputs: eager calls between two device synchronises, and the fused launch also as a
     replayed hipGraph of 100 launches (device time per launch without the host's enqueue cost);
  2. env steps per second of a C51Trainer at the config-5 sizes (SpaceInvaders obj-mode, 1 env,
     1M-transition replay, batch 32, train_frequency 4) in the training phase, as tools/dqn_bench.py
     measures config 5's DQNTrainer (run that beside this for the comparison).

    python tools/bench_c51.py [--steps K] [--warmup W] [--skip-trainer]
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


def torch_block(logits, logits_next, atoms, actions, rewards, dones, gamma, v_min, v_max):
    """The reference's loss block as torch ops (the per-sample index_add_ loop included) and
    its backward; returns d loss / d logits."""
    B, N = logits.shape[0], atoms.numel()
    A = logits.shape[1] // N
    rows = torch.arange(B, device=logits.device)
    lg = logits.detach().requires_grad_(True)
    with torch.no_grad():
        pm = torch.softmax(logits_next.view(B, A, N), dim=2)
        next_pmfs = pm[rows, torch.argmax((pm * atoms).sum(2), 1)]
        next_atoms = rewards.view(B, 1) + gamma * atoms * (1 - dones.view(B, 1))
        b = (next_atoms.clamp(v_min, v_max) - v_min) / (atoms[1] - atoms[0])
        lo, up = b.floor().clamp(0, N - 1), b.ceil().clamp(0, N - 1)
        m_lo = (up + (lo == up).float() - b) * next_pmfs
        m_up = (b - lo) * next_pmfs
        target = torch.zeros_like(next_pmfs)
        for i in range(B):
            target[i].index_add_(0, lo[i].long(), m_lo[i])
            target[i].index_add_(0, up[i].long(), m_up[i])
    old = torch.softmax(lg.view(B, A, N), dim=2)[rows, actions]
    loss = (-(target * old.clamp(min=1e-5, max=1 - 1e-5).log()).sum(-1)).mean()
    loss.backward()
    return lg.grad


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def bench_loss(dev, B=32, A=6, N=51):
    rng = np.random.default_rng(0)
    f = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)  # noqa: E731
    logits, logits_next = f(rng.standard_normal((B, A * N))), f(rng.standard_normal((B, A * N)))
    atoms = torch.linspace(-10, 10, N).to(dev)
    actions = torch.from_numpy(rng.integers(0, A, B)).to(dev)
    rewards, dones = f(rng.choice([-1.0, 0.0, 1.0], B)), f(rng.random(B) < 0.2)
    dl = torch.empty_like(logits)
    stats = torch.empty(2, device=dev)
    # index_add_ on the GPU is an atomic scatter: the reference block needs non-deterministic mode
    torch.use_deterministic_algorithms(False)
    fused = lambda: ops.c51_loss_fwd_bwd(logits, logits_next, atoms, actions, rewards, dones,  # noqa: E731
                                         0.99, -10.0, 10.0, dlogits=dl, stats=stats)
    ref = lambda: torch_block(logits, logits_next, atoms, actions, rewards, dones, 0.99, -10.0,  # noqa: E731
                              10.0)
    for _ in range(20):
        fused()
        g_ref = ref()
    torch.cuda.synchronize()
    err = float((dl - g_ref).abs().max() / g_ref.abs().max())
    runs = [(timed(fused, 2000), timed(ref, 30)) for _ in range(3)]  # alternating
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for _ in range(100):
            fused()
    g.replay()
    graph_us = [timed(g.replay, 50) / 100 for _ in range(3)]
    return {"shape": {"B": B, "A": A, "N": N},
            "fused_eager_us_per_call": [round(a, 2) for a, _ in runs],
            "torch_block_eager_us_per_call": [round(b, 1) for _, b in runs],
            "fused_graph_us_per_launch": [round(x, 2) for x in graph_us],
            "dlogits_max_diff_rel": err}


def bench_trainer(dev, steps, warmup):
    args = C51Args(env_id="ALE/SpaceInvaders-v5", obs_mode="obj", num_envs=1,
                   buffer_size=1_000_000, learning_starts=1000, total_timesteps=10_000_000,
                   save_model=False)
    tr = C51Trainer(args, dev, log=False)
    tr.steps(args.learning_starts + warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.steps(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    m = tr.metrics()
    return {"env_steps_per_sec": round(steps / dt, 1),
            "updates_per_sec": round(steps / args.train_frequency / dt, 1),
            "us_per_global_step": round(dt / steps * 1e6, 3), "steps": steps,
            "config": {"obs_mode": "obj", "num_envs": 1, "replay_rows": tr.rb.size,
                       "batch_size": args.batch_size, "n_atoms": args.n_atoms,
                       "cuda_graphs": tr._graphable()},
            "loss": m["losses/loss"], "data": "synthetic device env, random-init network"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--skip-trainer", action="store_true")
    o = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"loss_kernel": bench_loss(dev)}
    if not o.skip_trainer:
        out["trainer"] = bench_trainer(dev, o.steps, o.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
