"""Timings of the transformer block kernels and the transformer trainer.

    python tools/bench_transformer.py [--skip-trainer] [--S 8]

Every case runs twice, alternating in one session after a warm-up, each window bracketed by a
device synchronise; the yardstick is torch's own path on the same GPU and inputs.
  ops      mha forward+backward and add_layernorm forward+backward as replayed hipGraphs of
           back-to-back launches (the kernel's own time), against the torch ops they replace,
           captured the same way: the reference's update shape (320 samples x S, emb 128, heads 8)
           and a scaled one (4096 samples x S = 16)
  trainer  TransformerTrainer env steps/s at --dropout 0, fused path on (with torch's or the HIP
           add + LayerNorm) and off: 128 envs x 128 steps, emb 128, heads 8, blocks 3
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

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from oc_cleanrl_amd import ops  # noqa: E402
from oc_cleanrl_amd import transformer as T  # noqa: E402

REPS = 50  # launches per graph


def graph_us(body, rounds: int = 5) -> float:
    """Median time of one `body` inside a replayed hipGraph of REPS back-to-back copies."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            body()
    g.replay()
    times = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.replay()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / REPS * 1e6)
    return sorted(times)[len(times) // 2]


def torch_mha(qkv, valid, heads, dout):
    B, S, E3 = qkv.shape
    E = E3 // 3
    q = qkv.detach().requires_grad_(True)
    qh, kh, vh = (t.reshape(B, S, heads, E // heads).transpose(1, 2) for t in q.split(E, dim=2))
    s = qh @ kh.transpose(-1, -2) / math.sqrt(E // heads)
    s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    out = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, S, E)
    out.backward(dout)
    return q.grad


def op_cases(dev, B, S, E=128, heads=8):
    gen = torch.Generator(device="cpu").manual_seed(0)
    qkv = torch.randn(B, S, 3 * E, generator=gen).to(dev)
    dout = torch.randn(B, S, E, generator=gen).to(dev)
    n = torch.randint(max(1, S // 2), S + 1, (B,), generator=gen)
    valid = (torch.arange(S)[None] < n[:, None]).to(dev)
    kv = valid.to(torch.uint8)
    x, res = torch.randn(B * S, E, generator=gen).to(dev), torch.randn(B * S, E, generator=gen).to(dev)
    w, b = torch.randn(E, generator=gen).to(dev), torch.randn(E, generator=gen).to(dev)
    dy = torch.randn(B * S, E, generator=gen).to(dev)

    def hip_mha():
        out, lse = ops.mha_fwd(qkv, kv, heads)
        ops.mha_bwd(qkv, kv, out, lse, dout, heads)

    def hip_ln():
        _, mean, rstd = ops.add_layernorm_fwd(x, res, w, b, 1e-5)
        ops.add_layernorm_bwd(dy, x, res, w, mean, rstd)

    def torch_ln():
        xs, rs = x.detach().requires_grad_(True), res.detach().requires_grad_(True)
        ws, bs = w.detach().requires_grad_(True), b.detach().requires_grad_(True)
        F.layer_norm(xs + rs, (E,), ws, bs, 1e-5).backward(dy)

    return {"mha_hip": hip_mha, "mha_torch": lambda: torch_mha(qkv, valid, heads, dout),
            "add_layernorm_hip": hip_ln, "add_layernorm_torch": torch_ln}


def trainer_sps(dev, fused: bool, S: int, iters: int = 6, ln_hip: bool = False) -> float:
    T.FUSED_ATTN, T.ADD_LAYERNORM_HIP = fused, ln_hip
    args = T.finalize(T.TransformerArgs(num_envs=128, num_steps=128, buffer_window_size=S,
                                        dropout=0.0, total_timesteps=128 * 128 * 1000,
                                        save_model=False))
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
        T.FUSED_ATTN, T.ADD_LAYERNORM_HIP = True, False


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--S", type=int, default=8, help="objects per observation at the update shape")
    ap.add_argument("--skip-trainer", action="store_true")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    for shape, (B, S) in (("update", (320, a.S)), ("scaled", (4096, 16))):
        cases = op_cases(dev, B, S)
        for run in (1, 2):  # alternating: every case once per round
            for name, body in cases.items():
                print(json.dumps({"case": name, "shape": shape, "B": B, "S": S, "run": run,
                                  "us": round(graph_us(body), 2)}), flush=True)
    if not a.skip_trainer:
        for run in (1, 2):
            for fused, ln_hip in ((True, False), (True, True), (False, False)):
                sps = trainer_sps(dev, fused, a.S, ln_hip=ln_hip)
                print(json.dumps({"case": "trainer", "fused": fused, "add_layernorm_hip": ln_hip,
                                  "S": a.S, "run": run, "env_steps_per_s": round(sps)}),
                      flush=True)


if __name__ == "__main__":
    main()
