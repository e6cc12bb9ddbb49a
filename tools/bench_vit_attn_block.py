"""ops.vit_attn_block against the chain of launches it replaces (ops.ln_relu, the bias-free to_qkv,
ops.vit_attn, to_out and torch's add: vit.FUSED_ATTN = False), S = 49, D = 128, 8 heads, and the ViT
learner's rate with the switch off, on everywhere and on inside the routed range.

    python tools/bench_vit_attn_block.py [--samples 10 320 1280 4096] [--learner]

Per sample count: forward + backward and forward only (no_grad), median [min .. max] of 7 timed
loops in microseconds per call. --learner: env steps / s at the script's defaults on the synthetic
backend, 3 warm iterations, then three timed pairs of iterations per setting."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oc_cleanrl_amd import ops, vit  # noqa: E402

S, D, HEADS = 49, 128, 8


def chain(x, attn, T):
    qkv = vit._linear_nobias(vit._norm(x, attn.norm), attn.to_qkv)
    a = ops.vit_attn(qkv.view(-1, T, qkv.shape[1]), attn.heads)
    return vit._linear_nobias(a.view(x.shape[0], -1), attn.to_out) + x


def timed_loops(fn, iters, loops=7):
    for _ in range(3):
        fn()
    out = []
    for _ in range(loops):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return f"{statistics.median(out):.1f} [{min(out):.1f} .. {max(out):.1f}]"


def kernel_table(samples, dev):
    attn = vit.Attention(D, HEADS).to(dev)
    for B in samples:
        x = torch.randn(B * S, D, device=dev, requires_grad=True)
        dy = torch.randn(B * S, D, device=dev)
        iters = max(3, min(200, 40_000 // B))

        def both(f):
            attn.zero_grad(set_to_none=True)
            x.grad = None
            f(x, attn, S).backward(dy)

        def fwd(f):
            with torch.no_grad():
                f(x, attn, S)

        print(f"B {B}: fwd+bwd us  fused {timed_loops(lambda: both(ops.vit_attn_block), iters)}  "
              f"chain {timed_loops(lambda: both(chain), iters)}", flush=True)
        print(f"B {B}: fwd only us fused {timed_loops(lambda: fwd(ops.vit_attn_block), iters)}  "
              f"chain {timed_loops(lambda: fwd(chain), iters)}", flush=True)


def learner_rate(dev, lo, hi):
    for on, rng in ((False, (1, 0)), (True, (1, 1 << 30)), (True, (lo, hi))):
        vit.FUSED_ATTN = on
        ops.VIT_ATTN_BLOCK_MIN_SAMPLES, ops.VIT_ATTN_BLOCK_MAX_SAMPLES = rng
        args = vit.finalize(vit.ViTArgs(save_model=False, gemm_table=False, track=False,
                                        capture_video=False))
        tr = vit.ViTTrainer(args, dev, log=False)
        for _ in range(3):
            tr.train_iteration()
        rates = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(2):
                tr.train_iteration()
            torch.cuda.synchronize()
            rates.append(2 * args.num_envs * args.num_steps / (time.perf_counter() - t0))
        tr.close()
        print(f"learner FUSED_ATTN={on} samples in {rng}: {statistics.median(rates):.0f} env steps/s "
              f"[{min(rates):.0f} .. {max(rates):.0f}]", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, nargs="*", default=[10, 320, 1280, 4096])
    ap.add_argument("--learner", action="store_true")
    ap.add_argument("--range", type=int, nargs=2, default=[32, 1024],
                    help="the third learner setting: fused for lo <= samples <= hi")
    a = ap.parse_args()
    d = torch.device("cuda:0")
    kernel_table(a.samples, d)
    if a.learner:
        learner_rate(d, *a.range)
