"""Rates of ops.ln_chw_relu, the pixel PQN network's LayerNorm([C, H, W]) + ReLU.

    python tools/ln_chw_rate.py [--kernels-only | --trainer-only] [--iters K] [--rows R ...]

  kernels  forward + backward of ops.ln_chw_relu (channels_last rows, what the convolution
           kernels write) against torch's F.layer_norm + relu pair with autograd on the same
           rows, at the script's three widths x {8, 128, 256, 4096} rows, timed by graph replay
           (trainer.replay_time_us), warm; the two alternate, two runs each. Every line carries
           the bytes the algorithm needs (forward: x in, y out; backward: dy, x, y in, dx out) so
           that a kernel trace's times can be turned into bytes/s.
  trainer  env steps/s of pqn.PQNTrainer --architecture PQN --obs_mode dqn on the Synthetic
           backend (the script's 8 envs x 128 steps, 4 minibatches x 4 epochs): three warm-up
           iterations, then K replayed iterations timed by the host clock around a device
           synchronise, FUSED_LN_CHW_UPDATE on / off and FUSED_PQN off, three rounds.
Prints one JSON line per case and run.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from oc_cleanrl_amd import pqn as Q  # noqa: E402
from oc_cleanrl_amd.trainer import replay_time_us  # noqa: E402

SHAPES = [(32, 20, 20), (64, 9, 9), (64, 7, 7)]
ROWS = [8, 128, 256, 4096]
ENVS, STEPS = 8, 128


def ln_cases(dev, R, shape):
    ops = getattr(Q.ops, "ln_chw_relu", None)  # None on a tree without the kernel
    gen = torch.Generator(device="cpu").manual_seed(R + shape[0])
    cl = torch.channels_last
    x = torch.randn(R, *shape, generator=gen).to(dev).contiguous(memory_format=cl)
    g = torch.randn(R, *shape, generator=gen).to(dev).contiguous(memory_format=cl)
    w = (torch.rand(shape, generator=gen) + 0.5).to(dev).requires_grad_()
    b = torch.randn(shape, generator=gen).to(dev).requires_grad_()

    def run(fn):
        def body():
            w.grad = b.grad = None
            xs = x.detach().requires_grad_(True)
            fn(xs, w, b).backward(g)
        return body

    cases = {"ln_chw_torch": run(lambda x, w, b: F.relu(F.layer_norm(x, shape, w, b, 1e-5)))}
    if ops is not None:
        cases["ln_chw_hip"] = run(lambda x, w, b: ops(x, w, b))
    return cases


def trainer_rate(dev, fused: bool, ln_update: bool, iters: int):
    old = Q.FUSED_PQN, getattr(Q, "FUSED_LN_CHW_UPDATE", None)
    Q.FUSED_PQN, Q.FUSED_LN_CHW_UPDATE = fused, ln_update
    args = Q.finalize(Q.PQNArgs(architecture="PQN", obs_mode="dqn", num_envs=ENVS,
                                num_steps=STEPS, total_timesteps=ENVS * STEPS * 100_000,
                                save_model=False))
    tr = Q.PQNTrainer(args, dev, log=False)
    try:
        for _ in range(3):  # eager, capture, one replay
            tr.train_iteration(collect_metrics=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            tr.train_iteration(collect_metrics=False)
        torch.cuda.synchronize()
        return ENVS * STEPS * iters / (time.perf_counter() - t0), bool(tr.graphs_ready)
    finally:
        tr.close()
        Q.FUSED_PQN, Q.FUSED_LN_CHW_UPDATE = old


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--trainer-only", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rows", type=int, nargs="*", default=ROWS,
                    help="row counts of the kernel cases (one count: a kernel trace's per-kernel "
                         "statistics are then one shape each)")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if not a.trainer_only:
        for shape in SHAPES:
            E = shape[0] * shape[1] * shape[2]
            for R in a.rows:
                cases = ln_cases(dev, R, shape)
                for run in (1, 2):  # alternating
                    for name, body in cases.items():
                        us = replay_time_us(body, reps=8, rounds=3)
                        print(json.dumps({"case": name, "rows": R, "E": E, "run": run,
                                          "us": round(us, 2), "fwd_bytes": 8 * R * E,
                                          "bwd_bytes": 16 * R * E}), flush=True)
                del cases
                torch.cuda.empty_cache()
    if not a.kernels_only:
        has = hasattr(Q.ops, "ln_chw_relu")
        settings = [(True, True), (True, False), (False, False)] if has else \
            [(True, False), (False, False)]
        for run in (1, 2, 3):
            for fused, ln_update in settings:
                sps, graphs = trainer_rate(dev, fused, ln_update, a.iters)
                print(json.dumps({"case": "trainer_pixels", "envs": ENVS, "steps": STEPS,
                                  "fused": fused, "ln_chw_update": ln_update, "graphs": graphs,
                                  "run": run, "env_steps_per_s": round(sps)}), flush=True)


if __name__ == "__main__":
    main()
