"""MaDi masker measurements: the fused forward at 128 and 256 stacks, the fused forward
+ backward at a minibatch of 320 stacks (the script's 10 envs), the torch-module path of the same
tree beside them with its peak memory, and the learner's env steps/s at 10 envs. The results file
is rewritten after every case. All kernel times are hipGraph replays (trainer.replay_time_us).

--large N adds the forward + backward at N stacks (config 3's minibatch is 8192), --torch-large
the torch modules there (17.7 MiB of activations per stack: its peak memory or its allocation
failure), --envs the end-to-end run's env count. They are not in the default run: no call of more
than 512 stacks has run to its end on hardware, and ops.madi_ok routes such calls
to the torch modules.

    python tools/exp_madi.py [--out profiles/madi/exp_madi.json] [--skip-e2e] [--large 8192]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oc_cleanrl_amd import madi, ops  # noqa: E402
from oc_cleanrl_amd.trainer import replay_time_us  # noqa: E402

W, H, F = 4, 84, 32
MFMA_PEAK = 157e12  # f32-input MFMA, FLOP/s


def case(n, dev):
    gen = torch.Generator().manual_seed(0)
    x = torch.randint(0, 256, (n, W, H, H), generator=gen).to(torch.uint8).to(dev)
    torch.manual_seed(0)
    m = madi.MaskerNet((W, H, H), 3, F).to(dev)
    return x, m


def fused(n, dev, backward):
    x, m = case(n, dev)
    ws = tuple(w.detach() for w in m.weights())
    out = torch.empty((n, W, H, H), device=dev).contiguous(memory_format=torch.channels_last)
    g = torch.randn_like(out)
    grads = tuple(torch.empty_like(w) for w in ws)
    wsb = ops.madi_workspace(F, dev)
    reps = 4 if n > 1024 else 16
    t_f = replay_time_us(lambda: ops.madi_mask(x, None, ws, out=out), reps, 3)
    rec = {"stacks": n, "fused_fwd_us": t_f,
           "middle_layer_mfma_fraction": 2 * n * W * H * H * 9 * F * F / (t_f * 1e-6) / MFMA_PEAK}
    if backward:
        rec["fused_bwd_us"] = replay_time_us(
            lambda: ops.madi_mask_bwd(x, None, ws, g, grads, wsb), reps, 3)
    return rec


def torch_path(n, dev, backward):
    x, m = case(n, dev)
    xf = x.float()
    g = torch.randn_like(xf)
    rec = {}
    torch.cuda.reset_peak_memory_stats(dev)
    try:
        def fb():
            y = m.torch_forward(xf)
            if backward:
                torch.autograd.grad(y, m.weights(), g)

        if backward:
            fb()
        else:
            with torch.no_grad():
                fb()
        torch.cuda.synchronize()
        reps = 2 if n > 1024 else 8
        if backward:
            rec["torch_fwd_bwd_us"] = replay_time_us(fb, reps, 3)
        else:
            with torch.no_grad():
                rec["torch_fwd_us"] = replay_time_us(fb, reps, 3)
    except torch.OutOfMemoryError as e:
        rec["torch_error"] = str(e).splitlines()[0][:200]
    rec["torch_peak_gib"] = torch.cuda.max_memory_allocated(dev) / 2 ** 30
    return rec


def end_to_end(dev, envs=10, iters=5, fused_update=False):
    """Env steps/s of the learner (torch_deterministic as the script defaults it) with the update's
    masker on the torch modules or on the kernels."""
    ops.MADI_FUSED_UPDATE = fused_update
    a = madi.finalize(madi.MaDiArgs(num_envs=envs, total_timesteps=envs * 128 * iters,
                                    save_model=False))
    tr = madi.MaDiTrainer(a, dev, log=False)
    times = []
    for _ in range(iters):
        t0 = time.perf_counter()
        tr.train_iteration()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    first = tr.agent.network[0]
    x = torch.empty((tr.M, W, H, H), device=dev).contiguous(memory_format=tr.net_format)
    x.requires_grad_()
    return {"envs": envs, "iteration_s": times, "steps_per_s": envs * 128 / min(times[2:]),
            "minibatch": tr.M, "fused_rollout": tr.fused_rollout, "fused_update": tr.fused_update,
            "first_conv_x6_with_dgrad": bool(ops.conv_x6_ok(x, first.weight, 4, wgrad=True,
                                                            dgrad=True))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/madi/exp_madi.json")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--only-e2e", action="store_true")
    ap.add_argument("--envs", type=int, default=10, help="envs of the end-to-end run")
    ap.add_argument("--large", type=int, default=0,
                    help="also time the forward + backward at this many stacks (config 3: 8192)")
    ap.add_argument("--torch-large", action="store_true",
                    help="... and the torch modules there (17.7 MiB of activations per stack)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"forward": [], "forward_backward": []}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)

    def record(key, rec):
        if isinstance(res.get(key), list):
            res[key].append(rec)
        else:
            res[key] = rec
        print(json.dumps(rec), flush=True)
        out.write_text(json.dumps(res, indent=1) + "\n")  # after every case

    for n in () if a.only_e2e else (128, 256):
        record("forward", {**fused(n, dev, False), **torch_path(n, dev, False)})
    for n in () if a.only_e2e else (320,) + ((a.large,) if a.large else ()):
        ref = torch_path(n, dev, True) if n == 320 or a.torch_large else {}
        record("forward_backward", {**fused(n, dev, True), **ref})
        torch.cuda.empty_cache()
    if not a.skip_e2e:
        res["end_to_end"] = []
        for fu in (False, True):
            record("end_to_end", end_to_end(dev, a.envs, fused_update=fu))


if __name__ == "__main__":
    main()
