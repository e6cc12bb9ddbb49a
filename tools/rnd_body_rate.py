"""The pixel RND body on its two routes, device-event times:

  forward, both networks, R = 128 (the rollout's curiosity step): ops.rnd_body_forward against
    ops.rnd_normalize + the torch modules;
  forward + backward, the predictor, R = 4096 (a minibatch of the script's 128 x 128 / 4):
    ops.rnd_body against ops.rnd_normalize's rows gathered + the torch modules.

    python tools/rnd_body_rate.py [--out FILE] [--runs 2]

Each run alternates the two routes; one JSON line per run."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oc_cleanrl_amd import ops, rnd  # noqa: E402

P = 84 * 84


def _time(fn, reps: int) -> float:
    """Mean microseconds of fn over reps back-to-back calls, after a warm-up."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = rnd.RNDModel("RND").to(dev)
    pc, tc = ops.rnd_body_convs(model.predictor), ops.rnd_body_convs(model.target)
    pbody, tbody = model.predictor[:7], model.target[:7]
    B = 128 * 128
    stacks = torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, device=dev)
    frames = stacks.view(B, 4, P)[:, 3]
    state = ops.rms_state(P, dev)
    ops.rms_update(frames, state)
    buf = torch.empty((B, P), dtype=torch.float32, device=dev)
    ops.rnd_normalize(frames, state, buf)  # the torch route's batch buffer (made once per rollout)
    idx = torch.randperm(B, device=dev)[:4096]
    dout = torch.randn(4096, 3136, device=dev)
    small = torch.empty((128, P), dtype=torch.float32, device=dev)
    params = [p for m in pc for p in (m.weight, m.bias)]

    def fwd_fused():
        ops.rnd_body_forward(frames[:128], None, state, pc, tc)

    def fwd_torch():
        with torch.no_grad():
            x = ops.rnd_normalize(frames[:128], state, small).view(-1, 1, 84, 84)
            pbody(x), tbody(x)

    def fb_fused():
        torch.autograd.grad(ops.rnd_body(frames, idx, state, pc), params, dout)

    def fb_torch():
        x = buf.index_select(0, idx).view(-1, 1, 84, 84)
        torch.autograd.grad(pbody(x), params, dout)

    lines = []
    for run in range(a.runs):
        rec = {"run": run,
               "fwd2_R128_fused_us": _time(fwd_fused, a.reps),
               "fwd2_R128_torch_us": _time(fwd_torch, a.reps),
               "fwdbwd_R4096_fused_us": _time(fb_fused, a.reps),
               "fwdbwd_R4096_torch_us": _time(fb_torch, a.reps)}
        lines.append(json.dumps({k: round(v, 1) if isinstance(v, float) else v
                                 for k, v in rec.items()}))
        print(lines[-1], flush=True)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
