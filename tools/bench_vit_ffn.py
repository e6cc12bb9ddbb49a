"""ops.vit_ffn against the chain of launches it replaces (ops.ln_relu, linear_act, torch's GELU and
add: vit.FUSED_FFN = False), D = H = 128, and the ViT learner's rate with the switch on and off.

    python tools/bench_vit_ffn.py [--rows 490 15680 200704] [--learner]

Per row count: forward + backward and forward only (no_grad), median [min .. max] of 7 timed loops
in microseconds per call. --learner: env steps / s at the script's defaults on the synthetic
backend, 3 warm iterations, then three timed pairs of iterations per setting."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oc_cleanrl_amd import ops, vit  # noqa: E402
from oc_cleanrl_amd.agents import linear_act  # noqa: E402


def chain(x, ff):
    h = F.gelu(linear_act(vit._norm(x, ff.net[0]), ff.net[1], False))
    return linear_act(h, ff.net[3], False) + x


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


def kernel_table(rows_list, dev):
    ff = vit.FeedForward(128, 128).to(dev)
    for rows in rows_list:
        x = torch.randn(rows, 128, device=dev, requires_grad=True)
        dy = torch.randn(rows, 128, device=dev)
        iters = max(3, min(200, 4_000_000 // rows))

        def both(f):
            ff.zero_grad(set_to_none=True)
            x.grad = None
            f(x, ff).backward(dy)

        def fwd(f):
            with torch.no_grad():
                f(x, ff)

        print(f"rows {rows}: fwd+bwd us  fused {timed_loops(lambda: both(ops.vit_ffn), iters)}  "
              f"chain {timed_loops(lambda: both(chain), iters)}", flush=True)
        print(f"rows {rows}: fwd only us fused {timed_loops(lambda: fwd(ops.vit_ffn), iters)}  "
              f"chain {timed_loops(lambda: fwd(chain), iters)}", flush=True)


def learner_rate(dev):
    routed = (ops.VIT_FFN_MIN_ROWS, ops.VIT_FFN_MAX_ROWS)
    for on, cap in ((True, routed), (True, (1, 1 << 30)), (False, routed)):
        vit.FUSED_FFN, (ops.VIT_FFN_MIN_ROWS, ops.VIT_FFN_MAX_ROWS) = on, cap
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
        print(f"learner FUSED_FFN={on} rows in {cap}: {statistics.median(rates):.0f} env steps/s "
              f"[{min(rates):.0f} .. {max(rates):.0f}]", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="*", default=[490, 15680, 200704])
    ap.add_argument("--learner", action="store_true")
    a = ap.parse_args()
    d = torch.device("cuda:0")
    kernel_table(a.rows, d)
    if a.learner:
        learner_rate(d)
