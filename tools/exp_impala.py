"""IMPALA tower measurements: QNetworkImpala's three ConvSequences on the fused units
(ops.impala_sequence) beside the torch modules of the same network, as hipGraph replays
(trainer.replay_time_us): the tower forward at 1 and 8 acting rows and at a batch of 32, forward +
backward at 32 with torch's deterministic mode on and off, and the QDagger learner's online
steps/s both ways under torch_deterministic=True. Every case gets its input the way the learner
gives it: NCHW x / 255 (the fused path's channels_last copy is inside its time). The results
file is rewritten after every case.

    python tools/exp_impala.py [--out profiles/impala/exp_impala.json] [--skip-e2e]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/exp_impala.py --trace 20
        # per-kernel times of 20 eager fused forwards at batch 32 (the C = 32 kernels' share of
        # the f32-MFMA ceiling: MACS_C32 against the summed time of the kernels named in 25.4)
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oc_cleanrl_amd import dqn, ops, qdagger  # noqa: E402
from oc_cleanrl_amd.agents import fused_trunk  # noqa: E402
from oc_cleanrl_amd.trainer import replay_time_us  # noqa: E402

OBS, A = (4, 84, 84), 6
MFMA_PEAK = 157e12  # f32-input MFMA, FLOP/s
# MACs per image of the C = 32 convolutions (sequence 2: conv 16 -> 32 at 42 x 42, four 32 -> 32 at
# 21 x 21; sequence 3: conv at 21 x 21, four at 11 x 11) and of the whole tower
MACS_C32 = 9 * (16 * 32 * 42 * 42 + 4 * 32 * 32 * 21 * 21 + 32 * 32 * 21 * 21 + 4 * 32 * 32 * 11 * 11)
MACS = MACS_C32 + 9 * (4 * 16 * 84 * 84 + 4 * 16 * 16 * 42 * 42)


def tower(net, x, fused):
    ops.IMPALA_FUSED = fused
    try:
        return fused_trunk(net.network[:3], x)
    finally:
        ops.IMPALA_FUSED = True


def forward_case(n, dev):
    torch.manual_seed(0)
    net = qdagger.QNetworkImpala(OBS, A).to(dev)
    x = torch.randint(0, 256, (n,) + OBS, device=dev).float() / 255.0
    rec = {"rows": n}
    with torch.no_grad():
        for name, f in (("fused", True), ("torch", False)):
            rec[name + "_fwd_us"] = replay_time_us(lambda: tower(net, x, f), 16, 3)
    rec["tower_mfma_fraction"] = 2 * n * MACS / (rec["fused_fwd_us"] * 1e-6) / MFMA_PEAK
    return rec


def backward_case(n, dev):
    torch.manual_seed(0)
    net = qdagger.QNetworkImpala(OBS, A).to(dev)
    x = torch.randint(0, 256, (n,) + OBS, device=dev).float() / 255.0
    g = torch.randn((n, 32, 11, 11), device=dev)

    def step(f):
        for p in net.parameters():
            p.grad = None
        tower(net, x, f).backward(g)

    rec = {"rows": n, "input": "NCHW", "fused_fwd_bwd_us": replay_time_us(lambda: step(True), 8, 3)}
    for det in (True, False):
        torch.use_deterministic_algorithms(det)
        torch.backends.cudnn.deterministic = det
        rec[f"torch_fwd_bwd_us_deterministic_{det}"] = replay_time_us(lambda: step(False), 8, 3)
    # the same modules fed a channels_last input (not what the learner does)
    xc = x.contiguous(memory_format=torch.channels_last)
    x, x_nchw = xc, x
    rec["torch_fwd_bwd_us_channels_last_input"] = replay_time_us(lambda: step(False), 8, 3)
    x = x_nchw
    torch.use_deterministic_algorithms(False)
    torch.backends.cudnn.deterministic = False
    return rec


def trace(reps, dev):
    """`reps` eager fused forwards at batch 32, for a kernel trace."""
    torch.manual_seed(0)
    net = qdagger.QNetworkImpala(OBS, A).to(dev)
    x = torch.randint(0, 256, (32,) + OBS, device=dev).float() / 255.0
    with torch.no_grad():
        for _ in range(reps):
            tower(net, x, True)
    torch.cuda.synchronize()


def learner(fused, dev, teacher):
    ops.IMPALA_FUSED = fused
    try:
        a = qdagger.QDaggerArgs(obs_mode="dqn", student_network="impala", teacher_model_path=teacher,
                                teacher_return=5.0, teacher_steps=64, offline_steps=16,
                                buffer_size=4096, learning_starts=0, total_timesteps=100_000)
        tr = qdagger.QDaggerTrainer(a, dev, log=False)
        tr.steps(64)  # fill, offline, capture
        torch.cuda.synchronize()
        t0, n = time.perf_counter(), 1024
        tr.steps(n)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)
    finally:
        ops.IMPALA_FUSED = True


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/impala/exp_impala.json")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--trace", type=int, default=0, help="only N eager fused forwards")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    if args.trace:
        return trace(args.trace, dev)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res = {"device": torch.cuda.get_device_name(0), "macs_per_image": MACS, "forward": []}

    def save():
        out.write_text(json.dumps(res, indent=1) + "\n")

    for n in (1, 8, 32):
        res["forward"].append(forward_case(n, dev))
        save()
    res["forward_backward"] = backward_case(32, dev)
    save()
    if not args.skip_e2e:
        with tempfile.TemporaryDirectory() as d:
            teacher = str(Path(d) / "teacher.pt")
            torch.manual_seed(3)
            torch.save(dqn.QNetwork(OBS, A).state_dict(), teacher)
            res["learner_steps_per_s"] = {"torch_deterministic": True}
            for name, f in (("fused", True), ("torch", False)):
                res["learner_steps_per_s"][name] = learner(f, dev, teacher)
                save()
        # A chunk of the learner is 4 acting forwards at 1 row and one train step (the student's
        # forward + backward and the target's forward at 32 rows; the teacher is a NatureCNN on
        # both sides): the chunk-time difference the micro-benchmarks predict against the measured
        fw = {r["rows"]: r["torch_fwd_us"] - r["fused_fwd_us"] for r in res["forward"]}
        fb = res["forward_backward"]
        sps = res["learner_steps_per_s"]
        res["chunk_us_saved"] = {
            "predicted": fb["torch_fwd_bwd_us_deterministic_True"] - fb["fused_fwd_bwd_us"]
            + fw[32] + 4 * fw[1],
            "measured": 4e6 / sps["torch"] - 4e6 / sps["fused"]}
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
