"""Rates of the QDagger learner against the DQN learner it is built on.

    python tools/qdagger_rate.py [--steps N] [--timeout S]

Three figures from one session, each measured in a child process of its own under a time limit
(the parent never opens the GPU), at the shapes of BASELINE config 5 (SpaceInvaders-v5, obs_mode
obj, 1 env, the default QNetworkObj, a 1M-transition replay, batch 32, train_frequency 4):
  qdagger_online   env steps/s of QDaggerTrainer's online phase (graph replay), with a teacher of
                   the student's own dims
  dqn_online       the same figure for DQNTrainer, all steps past learning_starts
  qdagger_offline  train steps/s of QDaggerTrainer's offline phase (graph replay)
Each child warms up (eager step, capture, replays), then times N steps by the host clock around a
device synchronise, three rounds; every round is printed as one JSON line (quote the median).
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CASES = ("qdagger_online", "dqn_online", "qdagger_offline")
SHAPES = dict(env_id="ALE/SpaceInvaders-v5", obs_mode="obj", num_envs=1, buffer_size=1_000_000,
              total_timesteps=10_000_000, save_model=False)
WARM = 2000  # steps before the clock starts (config 5 warms up 1000 + 3 bench steps)


def timed(dev, fn, unit: int, rounds: int = 3):
    import torch

    for r in range(rounds):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        yield r + 1, unit / (time.perf_counter() - t0)


def child(case: str, steps: int):
    import torch

    from oc_cleanrl_amd.dqn import DQNArgs, DQNTrainer, make_qnet
    from oc_cleanrl_amd.qdagger import QDaggerArgs, QDaggerTrainer, env_shapes

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if case == "dqn_online":
        tr = DQNTrainer(DQNArgs(learning_starts=1000, **SHAPES), dev, log=False)
        tr.steps(1000 + WARM)
        run, key = (lambda: tr.steps(steps)), "env_steps_per_s"
    else:
        with tempfile.TemporaryDirectory() as d:
            a = QDaggerArgs(teacher_steps=4000, offline_steps=WARM + 3 * steps, learning_starts=0,
                            teacher_return=5.0, teacher_model_path=str(Path(d) / "teacher.pt"),
                            **SHAPES)
            torch.manual_seed(7)
            torch.save(make_qnet(a, *env_shapes(a)).state_dict(), a.teacher_model_path)
            tr = QDaggerTrainer(a, dev, log=False)
        tr.run_teacher_fill()
        if case == "qdagger_offline":
            tr.run_offline(WARM)
            run, key = (lambda: tr.run_offline(steps)), "train_steps_per_s"
        else:
            tr.run_offline()
            tr.steps(WARM)
            run, key = (lambda: tr.steps(steps)), "env_steps_per_s"
    for r, rate in timed(dev, run, steps):
        print(json.dumps({"case": case, "round": r, "steps": steps, key: round(rate, 1)}),
              flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--timeout", type=float, default=150.0, help="per case, seconds")
    ap.add_argument("--case", choices=CASES, default=None, help="(internal) run one case here")
    a = ap.parse_args(argv)
    if a.case:
        return child(a.case, a.steps)
    for case in CASES:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--case", case, "--steps",
               str(a.steps)]
        try:
            rc = subprocess.run(cmd, timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:  # nothing more on the GPU after a failure
            raise SystemExit(f"{case}: exit status {rc}")


if __name__ == "__main__":
    main()
