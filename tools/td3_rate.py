"""Rates of the TD3 / DDPG learner and its kernels.

    python tools/td3_rate.py [--skip-trainer] [--skip-run] [--steps K] [--out DIR]

  trainer  env steps/s of td3.TD3Trainer in the train phase (learning_starts 64, measured after
           it) on Pendulum-v1 at the scripts' defaults (1 env, batch 256) and at 16 envs, TD3 and
           DDPG, hipGraphs on, FUSED_TD3 on and off alternating, three rounds: K steps replayed,
           timed by the host clock around a device synchronise; every round is written, with the
           median and the spread (max - min) / median per setting. The baseline is the plain-torch
           path of the same trainer (there is no earlier learner to compare with).
  kernels  per-launch device time of the six kernels and of the torch ops each replaces at batch
           256, A = 1, D = 3, by graph replay (trainer.replay_time_us), warm, two alternating runs
  run      one learning run of TD3 on Pendulum-v1 (seed 1, learning_starts 1000, 20000 steps):
           its episodic returns -> run_returns.json (a single, unrepeated run)
Writes DIR/td3_rate.jsonl (default profiles/td3) and prints every line.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oc_cleanrl_amd import ddpg, ops, td3  # noqa: E402
from oc_cleanrl_amd.trainer import replay_time_us  # noqa: E402

WARM = 64  # learning_starts of the rate runs


def make(algo: str, envs: int, fused: bool, dev, **kw):
    td3.FUSED_TD3 = fused
    cls = td3.TD3Args if algo == "td3" else ddpg.DDPGArgs
    try:
        return td3.TD3Trainer(cls(num_envs=envs, learning_starts=float(WARM), **kw), dev, log=False)
    finally:
        td3.FUSED_TD3 = True


def trainer_rate(dev, algo: str, envs: int, fused: bool, steps: int) -> float:
    tr = make(algo, envs, fused, dev)
    tr.steps(WARM + 8)  # fill, the chunk around learning_starts, train: eager, capture, replay
    assert set(tr.graphs) == {"fill", "train"}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.steps(steps)
    torch.cuda.synchronize()
    return envs * steps / (time.perf_counter() - t0)


def kernel_cases(dev, B: int = 256, A: int = 1, D: int = 3, E: int = 1):
    g = torch.Generator().manual_seed(B)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    lo, hi = torch.full((A,), -2.0, device=dev), torch.full((A,), 2.0, device=dev)
    scale, bias = (hi - lo) / 2, (hi + lo) / 2
    h, w, b = torch.relu(rn(E, 256)), rn(A, 256) / 16, rn(A)
    step = torch.full((1,), 10 ** 6, dtype=torch.int64, device=dev)
    acts = torch.zeros((E, A), device=dev)
    rb = ops.ContReplayBuffer(4096, E, D, A, dev, seed=1)
    obs, nxt, fin, done, rew = rn(E, D), rn(E, D), rn(E, D), torch.zeros(E, device=dev), rn(E)
    for _ in range(64):
        rb.add(obs, nxt, fin, done, acts, rew)
    batch = rb.batch(B)
    mu, nxa, xa = rn(B, A), rn(B, D + A), rn(B, D + A)
    q1t, q2t, q1, q2, r, d = rn(B, 1), rn(B, 1), rn(B, 1), rn(B, 1), rn(B, 1), torch.zeros(B, 1, device=dev)
    dq1, dq2, st = torch.zeros_like(q1), torch.zeros_like(q2), torch.zeros(4, device=dev)
    p, t = rn(200000), rn(200000)
    p2, t2 = rn(70000), rn(70000)
    mu_g = mu.clone().requires_grad_()
    dxa = rn(B, D + A)
    leaf = [q1.clone().requires_grad_(), q2.clone().requires_grad_()]

    def act_torch():
        z = ops.td3_noise(1, step, E, A)
        a = torch.tanh(td3.act_mu(h, w, b)) * scale + bias
        acts.copy_(torch.clamp(a + (scale * 0.1) * z, lo, hi))

    def target_torch():
        z = ops.td3_target_noise(1, rb.counter, B, A)
        n = (z * 0.2).clamp(-0.5, 0.5) * scale
        nxa[:, D:].copy_((torch.tanh(mu) * scale + bias + n).clamp(-2.0, 2.0))

    def critic_torch():
        for x in leaf:
            x.grad = None
        y = r.flatten() + (1 - d.flatten()) * 0.99 * torch.min(q1t, q2t).view(-1)
        l1 = torch.nn.functional.mse_loss(leaf[0].view(-1), y)
        l2 = torch.nn.functional.mse_loss(leaf[1].view(-1), y)
        (l1 + l2).backward()
        st.copy_(torch.stack([l1, l2, leaf[0].mean(), leaf[1].mean()]).detach())

    def policy_fused():
        mu_g.grad = None
        ops.td3_policy_actions(mu_g, xa, scale, bias).backward(dxa)

    def policy_torch():
        mu_g.grad = None
        torch.cat([xa[:, :D], torch.tanh(mu_g) * scale + bias], 1).backward(dxa)

    def polyak_torch():
        t.copy_(0.005 * p + 0.995 * t)
        t2.copy_(0.005 * p2 + 0.995 * t2)

    return {
        "cont_replay_add": lambda: rb.add(obs, nxt, fin, done, acts, rew, carry=True),
        "cont_replay_sample": lambda: rb.sample(B, out=batch),
        "td3_act": lambda: ops.td3_act(h, w, b, scale, bias, lo, hi, 1, step, 0, 0.1, acts),
        "td3_act_torch": act_torch,
        "td3_target_actions": lambda: ops.td3_target_actions(mu, scale, bias, nxa, 1, rb.counter,
                                                             0.2, 0.5, -2.0, 2.0),
        "td3_target_actions_torch": target_torch,
        "td3_critic_loss_fwd_bwd": lambda: ops.td3_critic_loss_fwd_bwd(
            q1t, q2t, q1, q2, r, d, 0.99, dq1=dq1, dq2=dq2, stats=st),
        "td3_critic_loss_torch": critic_torch,
        "td3_policy_actions_fwd_bwd": policy_fused,
        "td3_policy_actions_torch": policy_torch,
        "polyak": lambda: ops.polyak_([(p, t), (p2, t2)], 0.005),
        "polyak_torch": polyak_torch,
    }


def learning_run(dev, out: Path, steps: int = 20000):
    tr = td3.TD3Trainer(td3.TD3Args(seed=1, learning_starts=1000.0, total_timesteps=steps), dev,
                        log=False)
    curve = []
    while tr.global_step < steps:
        tr.steps(1000)
        m = tr.metrics()
        curve.append({"global_step": tr.global_step,
                      "episodic_return": m.get("charts/episodic_return")})
    (out / "run_returns.json").write_text(json.dumps(
        {"env_id": "Pendulum-v1", "seed": 1, "learning_starts": 1000, "steps": steps,
         "note": "a single, unrepeated run; mean return of the episodes ended in each 1000 steps",
         "curve": curve}, indent=1))
    return curve


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-trainer", action="store_true")
    ap.add_argument("--skip-run", action="store_true")
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "td3"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    with open(out / "td3_rate.jsonl", "w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        cases = kernel_cases(dev)
        for run in (1, 2):
            for name, body in cases.items():
                emit({"case": name, "batch": 256, "run": run,
                      "us": round(replay_time_us(body, reps=16, rounds=3), 2)})
        if not a.skip_trainer:
            rates: dict = {}
            for run in (1, 2, 3):
                for algo in ("td3", "ddpg"):
                    for envs in (1, 16):
                        for fused in (True, False):
                            sps = trainer_rate(dev, algo, envs, fused, a.steps)
                            rates.setdefault((algo, envs, fused), []).append(sps)
                            emit({"case": "trainer", "algo": algo, "envs": envs, "fused": fused,
                                  "run": run, "env_steps_per_s": round(sps)})
            for (algo, envs, fused), v in rates.items():
                med = statistics.median(v)
                emit({"case": "trainer_median", "algo": algo, "envs": envs, "fused": fused,
                      "env_steps_per_s": round(med), "spread": round((max(v) - min(v)) / med, 4)})
        if not a.skip_run:
            curve = learning_run(dev, out)
            emit({"case": "learning_run", "last": curve[-1]})


if __name__ == "__main__":
    main()
