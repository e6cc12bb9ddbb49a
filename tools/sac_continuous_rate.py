"""Rates of the continuous SAC learner and its kernels.

    python tools/sac_continuous_rate.py [--skip-trainer] [--skip-run] [--steps K] [--out DIR]

  trainer  env steps/s of sac_continuous.ContSACTrainer in the train phase (learning_starts 64,
           measured after it) on Pendulum-v1 at the script's defaults (1 env, batch 256) and at 16
           envs, hipGraphs on, FUSED_CSAC on and off alternating, three rounds: K steps replayed,
           timed by the host clock around a device synchronise; every round is written, with the
           median and the spread (max - min) / median per setting. The baseline is the plain-torch
           path of the same trainer (there is no earlier learner to compare with).
  kernels  per-launch device time of the new kernels and of the torch ops each replaces at batch
           256, A = 1, D = 3, by graph replay (trainer.replay_time_us), warm, two alternating runs
  run      one learning run on Pendulum-v1 (seed 1, learning_starts 1000, 20000 steps): its
           episodic returns -> run_returns.json (a single, unrepeated run)
Writes DIR/sac_continuous_rate.jsonl (default profiles/sac_continuous) and prints every line.
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

from oc_cleanrl_amd import ops, td3  # noqa: E402
from oc_cleanrl_amd import sac_continuous as sc  # noqa: E402
from oc_cleanrl_amd.trainer import replay_time_us  # noqa: E402

WARM = 64  # learning_starts of the rate runs


def make(envs: int, fused: bool, dev, **kw):
    sc.FUSED_CSAC = fused
    try:
        return sc.ContSACTrainer(sc.ContSACArgs(num_envs=envs, learning_starts=float(WARM), **kw),
                                 dev, log=False)
    finally:
        sc.FUSED_CSAC = True


def trainer_rate(dev, envs: int, fused: bool, steps: int) -> float:
    tr = make(envs, fused, dev)
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
    h, wm, bm, wl, bl = torch.relu(rn(E, 256)), rn(A, 256) / 16, rn(A), rn(A, 256) / 16, rn(A)
    step = torch.full((1,), 10 ** 6, dtype=torch.int64, device=dev)
    ctr = torch.full((1,), 5, dtype=torch.int64, device=dev)
    acts = torch.zeros((E, A), device=dev)
    mean, r, nxa, xa = rn(B, A), rn(B, A), rn(B, D + A), rn(B, D + A)
    q1t, q2t, q1, q2, rew, lp = (rn(B, 1) for _ in range(6))
    d = torch.zeros(B, 1, device=dev)
    dq1, dq2, dlp = torch.zeros_like(q1), torch.zeros_like(q2), torch.zeros_like(q1)
    st, loss = torch.zeros(4, device=dev), torch.zeros(1, device=dev)
    mean_g, r_g = mean.clone().requires_grad_(), r.clone().requires_grad_()
    dxa = rn(B, D + A)
    leaf = [q1.clone().requires_grad_(), q2.clone().requires_grad_(), lp.clone().requires_grad_()]
    temp = ops.SacTemperature(dev, True, 0.2, lr=1e-3, target_entropy=-float(A), eps=1e-8)
    temp_t = ops.SacTemperature(dev, True, 0.2, lr=1e-3, target_entropy=-float(A), eps=1e-8)
    host = type("T", (), {"temp": temp_t, "alpha_loss": loss})()  # _alpha_step_torch's self

    def act_torch():
        z = ops.csac_noise(1, step, E, A)
        m, rr = td3.act_mu(h, wm, bm), td3.act_mu(h, wl, bl)
        acts.copy_(torch.tanh(m + torch.exp(sc.log_std_of(rr)) * z) * scale + bias)

    def target_torch():
        a, _ = sc.squash(mean, r, ops.csac_noise(1, ctr, B, A, draw=0), scale, bias)
        nxa[:, D:].copy_(a)

    def clear():
        for x in leaf + [mean_g, r_g]:
            x.grad = None

    def critic_torch():
        clear()
        y = rew.flatten() + (1 - d.flatten()) * 0.99 * (torch.min(q1t, q2t) - temp.alpha * lp).view(-1)
        l1 = torch.nn.functional.mse_loss(leaf[0].view(-1), y)
        l2 = torch.nn.functional.mse_loss(leaf[1].view(-1), y)
        (l1 + l2).backward()
        st.copy_(torch.stack([l1, l2, leaf[0].mean(), leaf[1].mean()]).detach())

    def sample_fused():
        clear()
        out, lg = ops.csac_sample(mean_g, r_g, xa, scale, bias, 1, ctr, 1)
        torch.autograd.backward([out, lg], [dxa, dlp])

    def sample_torch():
        clear()
        a, lg = sc.SquashTorch.apply(mean_g, r_g, ops.csac_noise(1, ctr, B, A, draw=1), scale, bias)
        torch.autograd.backward([torch.cat([xa[:, :D], a], 1), lg], [dxa, dlp])

    def actor_torch():
        clear()
        lv = ((temp.alpha * leaf[2]) - torch.min(leaf[0], leaf[1])).mean()
        lv.backward()
        loss.copy_(lv.detach().view(1))

    return {
        "csac_act": lambda: ops.csac_act(h, wm, bm, wl, bl, scale, bias, lo, hi, 1, step, 0, acts),
        "csac_act_torch": act_torch,
        "csac_sample_forward": lambda: ops.csac_sample_forward(mean, r, scale, bias, 1, ctr, 0,
                                                               xa=nxa),
        "csac_sample_forward_torch": target_torch,
        "csac_critic_loss_fwd_bwd": lambda: ops.csac_critic_loss_fwd_bwd(
            q1t, q2t, q1, q2, rew, d, lp, temp.alpha, 0.99, dq1=dq1, dq2=dq2, stats=st),
        "csac_critic_loss_torch": critic_torch,
        "csac_sample_fwd_bwd": sample_fused,
        "csac_sample_torch": sample_torch,
        "csac_actor_loss_fwd_bwd": lambda: ops.csac_actor_loss_fwd_bwd(
            q1, q2, lp, temp.alpha, dq1=dq1, dq2=dq2, dlogp=dlp, loss=loss),
        "csac_actor_loss_torch": actor_torch,
        "csac_alpha_step": lambda: ops.csac_alpha_step(lp, temp, loss=loss),
        "csac_alpha_step_torch": lambda: sc.ContSACTrainer._alpha_step_torch(host, lp),
    }


def learning_run(dev, out: Path, steps: int = 20000):
    tr = sc.ContSACTrainer(sc.ContSACArgs(seed=1, learning_starts=1000.0, total_timesteps=steps),
                           dev, log=False)
    curve = []
    while tr.global_step < steps:
        tr.steps(1000)
        m = tr.metrics()
        curve.append({"global_step": tr.global_step,
                      "episodic_return": m.get("charts/episodic_return"),
                      "alpha": m.get("losses/alpha")})
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sac_continuous"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    with open(out / "sac_continuous_rate.jsonl", "w") as f:
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
                for envs in (1, 16):
                    for fused in (True, False):
                        sps = trainer_rate(dev, envs, fused, a.steps)
                        rates.setdefault((envs, fused), []).append(sps)
                        emit({"case": "trainer", "envs": envs, "fused": fused, "run": run,
                              "env_steps_per_s": round(sps)})
            for (envs, fused), v in rates.items():
                med = statistics.median(v)
                emit({"case": "trainer_median", "envs": envs, "fused": fused,
                      "env_steps_per_s": round(med), "spread": round((max(v) - min(v)) / med, 4)})
        if not a.skip_run:
            curve = learning_run(dev, out)
            emit({"case": "learning_run", "last": curve[-1]})


if __name__ == "__main__":
    main()
