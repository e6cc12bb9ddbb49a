"""Rates of the PQN learner and its LayerNorm + ReLU kernel.

    python tools/pqn_rate.py [--skip-trainer] [--iters K]

  trainer  env steps/s of pqn.PQNTrainer at 128 envs x 128 steps on the Synthetic object env (the
           script's 4 minibatches x 4 epochs, the default PQN_OBJ network), FUSED_PQN on and off:
           three eager / capture / replay warm-up iterations, then K replayed iterations timed by
           the host clock around a device synchronise; the two settings alternate, three rounds,
           every round printed (the median is the figure to quote)
  ln_relu  ops.ln_relu forward + backward against torch's F.layer_norm + relu pair with
           autograd, at the workload's row shapes (update: minibatch rows x frames for the
           encoder, minibatch rows for the decoder; rollout: the envs' rows, forward only), timed
           by graph replay (trainer.replay_time_us), warm; two alternating runs
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

from oc_cleanrl_amd import ops  # noqa: E402
from oc_cleanrl_amd import pqn as Q  # noqa: E402
from oc_cleanrl_amd.trainer import replay_time_us  # noqa: E402

ENVS, STEPS = 128, 128


def ln_cases(dev, R, E, train: bool):
    gen = torch.Generator(device="cpu").manual_seed(R + E)
    x = torch.randn(R, E, generator=gen).to(dev)
    w = (torch.rand(E, generator=gen) + 0.5).to(dev).requires_grad_(train)
    b = torch.randn(E, generator=gen).to(dev).requires_grad_(train)
    g = torch.randn(R, E, generator=gen).to(dev)

    def run(fn):
        def body():
            if not train:
                with torch.no_grad():
                    fn(x, w, b)
                return
            w.grad = b.grad = None
            xs = x.detach().requires_grad_(True)
            fn(xs, w, b).backward(g)
        return body

    return {"ln_relu_hip": run(lambda x, w, b: ops.ln_relu(x, w, b)),
            "ln_relu_torch": run(lambda x, w, b: F.relu(F.layer_norm(x, (E,), w, b, 1e-5)))}


def trainer_rate(dev, fused: bool, iters: int):
    Q.FUSED_PQN = fused
    args = Q.finalize(Q.PQNArgs(num_envs=ENVS, num_steps=STEPS,
                                total_timesteps=ENVS * STEPS * 100_000, save_model=False))
    tr = Q.PQNTrainer(args, dev, log=False)
    try:
        for _ in range(3):  # eager, capture, one replay
            tr.train_iteration(collect_metrics=False)
        assert tr.graphs_ready
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            tr.train_iteration(collect_metrics=False)
        torch.cuda.synchronize()
        return ENVS * STEPS * iters / (time.perf_counter() - t0)
    finally:
        tr.close()
        Q.FUSED_PQN = True


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-trainer", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    M, W = ENVS * STEPS // 4, 4
    shapes = [(M * W, 128, True), (M * W, 64, True), (M, 128, True),
              (ENVS * W, 128, False), (ENVS * W, 64, False), (ENVS, 128, False)]
    groups = [({"rows": R, "E": E, "phase": "update" if tr else "rollout"},
               ln_cases(dev, R, E, tr)) for R, E, tr in shapes]
    for run in (1, 2):  # alternating: every case once per round
        for shape, cases in groups:
            for name, body in cases.items():
                us = replay_time_us(body, reps=16, rounds=3)
                print(json.dumps({"case": name, **shape, "run": run, "us": round(us, 2)}),
                      flush=True)
    if not a.skip_trainer:
        for run in (1, 2, 3):
            for fused in (True, False):
                sps = trainer_rate(dev, fused, a.iters)
                print(json.dumps({"case": "trainer", "envs": ENVS, "steps": STEPS, "fused": fused,
                                  "run": run, "env_steps_per_s": round(sps)}), flush=True)


if __name__ == "__main__":
    main()
