"""Timings of the counter-based dropout kernels and of the transformer trainer at dropout = 0.1
(DESIGN.md 13), with the method of tools/bench_transformer.py: replayed hipGraphs of back-to-back
launches, every case twice, alternating in one session after a warm-up.

    python tools/bench_transformer_dropout.py [--skip-trainer] [--S 8]

  ops      ops.mha forward+backward at p = 0.1 against p = 0 and against the torch ops it
           replaces at p = 0.1 (bmm / mask / softmax / dropout / bmm); ops.dropout
           forward+backward against torch.nn.functional.dropout on [B * S, 128]: the reference's
           update shape (320 samples x S, emb 128, heads 8) and a scaled one (4096 x S = 16)
  trainer  TransformerTrainer env steps/s at dropout = 0.1 with --fused-dropout and without
           (torch's layer modules, the default route): 128 envs x 128 steps, emb 128, heads 8,
           blocks 3
Prints one JSON line per case and run.
"""
from __future__ import annotations

import argparse
import json
import math
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from bench_transformer import graph_us  # noqa: E402

from oc_cleanrl_amd import ops  # noqa: E402
from oc_cleanrl_amd import transformer as T  # noqa: E402

P = 0.1


def torch_mha_dropout(qkv, valid, heads, dout):
    B, S, E3 = qkv.shape
    E = E3 // 3
    q = qkv.detach().requires_grad_(True)
    qh, kh, vh = (t.reshape(B, S, heads, E // heads).transpose(1, 2) for t in q.split(E, dim=2))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(E // heads)
    s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    out = (F.dropout(torch.softmax(s, -1), P) @ vh).transpose(1, 2).reshape(B, S, E)
    out.backward(dout)
    return q.grad


def op_cases(dev, B, S, E=128, heads=8):
    gen = torch.Generator(device="cpu").manual_seed(0)
    qkv = torch.randn(B, S, 3 * E, generator=gen).to(dev)
    dout = torch.randn(B, S, E, generator=gen).to(dev)
    n = torch.randint(max(1, S // 2), S + 1, (B,), generator=gen)
    valid = (torch.arange(S)[None] < n[:, None]).to(dev)
    kv = valid.to(torch.uint8)
    x = torch.randn(B * S, E, generator=gen).to(dev)
    dy = torch.randn(B * S, E, generator=gen).to(dev)
    rng = ops.philox_state(1, dev)

    def mha_p0():
        out, lse = ops.mha_fwd(qkv, kv, heads)
        ops.mha_bwd(qkv, kv, out, lse, dout, heads)

    def mha_p():
        out, lse = ops.mha_dropout_fwd(qkv, kv, heads, rng, 0, P)
        ops.mha_dropout_bwd(qkv, kv, out, lse, dout, heads, rng, 0, P)

    def drop_hip():
        ops.dropout_fwd(x, rng, 1, P)
        ops.dropout_fwd(dy, rng, 1, P)

    def drop_torch():
        xs = x.detach().requires_grad_(True)
        F.dropout(xs, P).backward(dy)

    return {"mha_hip_p0": mha_p0, "mha_hip_p0.1": mha_p,
            "mha_torch_p0.1": lambda: torch_mha_dropout(qkv, valid, heads, dout),
            "dropout_hip": drop_hip, "dropout_torch": drop_torch}


def trainer_sps(dev, fused_dropout: bool, S: int, iters: int = 6) -> float:
    args = T.finalize(T.TransformerArgs(num_envs=128, num_steps=128, buffer_window_size=S,
                                        dropout=P, fused_dropout=fused_dropout,
                                        total_timesteps=128 * 128 * 1000, save_model=False))
    tr = T.TransformerTrainer(args, dev, log=False)
    try:
        for _ in range(3):  # eager, capture, one replay
            tr.train_iteration(collect_metrics=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            tr.train_iteration(collect_metrics=False)
        torch.cuda.synchronize()
        return iters * args.batch_size / (time.perf_counter() - t0)
    finally:
        tr.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=8, help="objects per observation at the update shape")
    ap.add_argument("--skip-trainer", action="store_true")
    ap.add_argument("--skip-ops", action="store_true")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if not a.skip_ops:
        for shape, (B, S) in (("update", (320, a.S)), ("scaled", (4096, 16))):
            cases = op_cases(dev, B, S)
            for run in (1, 2):  # alternating: every case once per round
                for name, body in cases.items():
                    print(json.dumps({"case": name, "shape": shape, "B": B, "S": S, "run": run,
                                      "us": round(graph_us(body), 2)}), flush=True)
    if not a.skip_trainer:
        for run in (1, 2):
            for fused_dropout in (True, False):
                sps = trainer_sps(dev, fused_dropout, a.S)
                print(json.dumps({"case": "trainer", "dropout": P, "fused_dropout": fused_dropout,
                                  "S": a.S, "run": run, "env_steps_per_s": round(sps)}),
                      flush=True)


if __name__ == "__main__":
    main()
