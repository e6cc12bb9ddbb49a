"""Timings of the LSTM kernels and the recurrent trainer.

    python tools/bench_lstm.py [--skip-trainer]

Every case runs twice, alternating in one session; the yardstick is torch's own path on the same
GPU and inputs. Kernel cases are timed by graph replay (trainer.replay_time_us: back-to-back
copies of the closure captured into one hipGraph):
  seq      ops.lstm_seq forward + backward (the input projection and the two parameter-gradient
           GEMMs included) against the per-step nn.LSTM loop with autograd (ppo_atari_lstm.py:
           148-156), T = 128, I = 512, H = 128, B = 2 (the reference's minibatch) and B = 32
  step     ops.lstm_step against one nn.LSTM step with the two mask products, N = 8 and N = 128
  trainer  one LSTMTrainer iteration (8 envs x 128 steps, the script's defaults on the PPObj
           trunk), FUSED_LSTM on and off, wall time per iteration
Every case, torch's included, is captured; the trainer's iterations are replayed graphs timed by
the host clock around a device synchronise. Prints one JSON line per case and run.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import torch
import torch.nn as nn

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from oc_cleanrl_amd import lstm as L  # noqa: E402
from oc_cleanrl_amd import ops  # noqa: E402
from oc_cleanrl_amd.agents import linear_act  # noqa: E402
from oc_cleanrl_amd.trainer import replay_time_us  # noqa: E402


def seq_cases(dev, B, T=128, I=512, H=128):
    gen = torch.Generator(device="cpu").manual_seed(0)
    mod = nn.LSTM(I, H).to(dev)
    x = torch.randn(T * B, I, generator=gen).to(dev)
    done = (torch.rand(T, B, generator=gen) < 0.05).float().to(dev)
    g = torch.randn(T * B, H, generator=gen).to(dev)
    state = (torch.randn(1, B, H, generator=gen).to(dev), torch.randn(1, B, H, generator=gen).to(dev))
    ih = SimpleNamespace(weight=mod.weight_ih_l0, bias=mod.bias_ih_l0)

    def fused():
        mod.zero_grad()
        xs = x.detach().requires_grad_(True)
        pre = linear_act(xs, ih, False).view(T, B, 4 * H)
        out, _ = ops.lstm_seq(pre, mod.weight_hh_l0, mod.bias_hh_l0, done, state[0][0], state[1][0])
        out.view(T * B, H).backward(g)

    def loop():
        mod.zero_grad()
        xs = x.detach().requires_grad_(True)
        st, outs = state, []
        for h, d in zip(xs.view(T, B, I), done):
            m = (1.0 - d).view(1, -1, 1)
            h, st = mod(h.unsqueeze(0), (m * st[0], m * st[1]))
            outs.append(h)
        torch.flatten(torch.cat(outs), 0, 1).backward(g)

    return {"seq_hip": (fused, 8), "seq_torch": (loop, 2)}


def step_cases(dev, N, I=512, H=128):
    gen = torch.Generator(device="cpu").manual_seed(1)
    mod = nn.LSTM(I, H).to(dev)
    x = torch.randn(N, I, generator=gen).to(dev)
    done = (torch.rand(N, generator=gen) < 0.05).float().to(dev)
    h, c = torch.randn(N, H, generator=gen).to(dev), torch.randn(N, H, generator=gen).to(dev)
    hs, cs = h.clone().unsqueeze(0), c.clone().unsqueeze(0)

    def fused():
        ops.lstm_step(x, mod.weight_ih_l0, mod.bias_ih_l0, mod.weight_hh_l0, mod.bias_hh_l0, done,
                      h, c)

    def torch_step():
        with torch.no_grad():
            m = (1.0 - done).view(1, -1, 1)
            mod(x.unsqueeze(0), (m * hs, m * cs))

    return {"step_hip": (fused, 64), "step_torch": (torch_step, 16)}


def trainer_us(dev, fused: bool, iters: int = 4):
    L.FUSED_LSTM = fused
    args = L.finalize(L.LSTMArgs(total_timesteps=8 * 128 * 1000, save_model=False))
    tr = L.LSTMTrainer(args, dev, log=False)
    try:
        for _ in range(3):  # eager, capture, one replay
            tr.train_iteration(collect_metrics=False)
        assert tr.graphs_ready
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            tr.train_iteration(collect_metrics=False)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e6
    finally:
        tr.close()
        L.FUSED_LSTM = True


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-trainer", action="store_true")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    groups = [("seq", {"B": B}, seq_cases(dev, B)) for B in (2, 32)] + \
        [("step", {"N": N}, step_cases(dev, N)) for N in (8, 128)]
    for run in (1, 2):  # alternating: every case once per round
        for _, shape, cases in groups:
            for name, (body, reps) in cases.items():
                us = replay_time_us(body, reps=reps, rounds=3)
                print(json.dumps({"case": name, **shape, "run": run, "us": round(us, 2)}),
                      flush=True)
    if not a.skip_trainer:
        for run in (1, 2):
            for fused in (True, False):
                us = trainer_us(dev, fused)
                print(json.dumps({"case": "trainer_iteration", "fused": fused, "run": run,
                                  "us": round(us)}), flush=True)


if __name__ == "__main__":
    main()
