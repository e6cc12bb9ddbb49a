"""Rates of the continuous-action PPO learner and its four kernels.

    python tools/contppo_rate.py [--skip-trainer] [--iters K]

  trainer  env steps/s of contppo.ContPPOTrainer on Pendulum-v1 at the script's defaults (1 env x
           2048 steps, 32 minibatches x 10 epochs) and at 64 envs x 32 steps, FUSED_CONT on and
           off: three eager / capture / replay warm-up iterations, then K replayed iterations timed
           by the host clock around a device synchronise; the two settings alternate, three
           rounds, every round printed (the median is the figure to quote)
  kernels  per-launch device time of ops.gauss_head_sample, ops.gauss_ppo_loss_fwd_bwd,
           ops.env_normalize and ops.pendulum_step (the fused launch, and the raw launch) at the
           two workloads' shapes, timed by graph replay (trainer.replay_time_us), warm; beside the
           two Gaussian kernels, the plain-torch ops they replace; two alternating runs
Prints one JSON line per case and run.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from oc_cleanrl_amd import contppo as C  # noqa: E402
from oc_cleanrl_amd import ops  # noqa: E402
from oc_cleanrl_amd.trainer import replay_time_us  # noqa: E402

WORKLOADS = [(1, 2048), (64, 32)]  # (envs, steps); 32 minibatches either way: M = 64


def kernel_cases(dev, N: int, M: int, A: int = 1):
    g = torch.Generator().manual_seed(N + M)
    rn = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    mean, z, value, logstd = rn(N, A), rn(N, A), rn(N), (0.1 * rn(A))
    act, lp, val = torch.empty_like(mean), torch.empty(N, device=dev), torch.empty(N, device=dev)
    mm, ma, mv = rn(M, A), rn(M, A), rn(M)
    olp, adv, ret, vold = rn(M) - 1.0, rn(M), rn(M), rn(M)
    stats_in = torch.stack([adv.mean(), adv.std()])
    dmean, dvalue = torch.empty_like(mm), torch.empty(M, device=dev)
    dls, st = torch.empty(A, device=dev), torch.empty(len(ops.STAT_NAMES), device=dev)
    hyper = dict(clip_coef=0.2, ent_coef=0.0, vf_coef=0.5, norm_adv=True, clip_vloss=True)

    def head_torch():
        std = torch.exp(logstd.expand_as(mean))
        a = z.mul(std).add(mean)
        act.copy_(a)
        lp.copy_(C.gauss_logprob_rows(mean, std, a))
        val.copy_(value)

    leaf = [t.clone().requires_grad_() for t in (mm, logstd.view(1, -1), mv)]

    def loss_torch():
        for t in leaf:
            t.grad = None
        probs = torch.distributions.Normal(leaf[0], torch.exp(leaf[1].expand_as(leaf[0])),
                                           validate_args=False)
        ratio = (probs.log_prob(ma).sum(1) - olp).exp()
        ad = (adv - adv.mean()) / (adv.std() + 1e-8)
        pg = torch.max(-ad * ratio, -ad * torch.clamp(ratio, 0.8, 1.2)).mean()
        vc = vold + torch.clamp(leaf[2] - vold, -0.2, 0.2)
        vl = 0.5 * torch.max((leaf[2] - ret) ** 2, (vc - ret) ** 2).mean()
        (pg - 0.0 * probs.entropy().sum(1).mean() + vl * 0.5).backward()

    state = torch.zeros((N, 2), dtype=torch.float64, device=dev)
    counters = torch.zeros((N, 2), dtype=torch.int64, device=dev)
    norm = ops.cont_norm_state(N, 3, dev)
    obs, fin = torch.zeros((N, 3), device=dev), torch.zeros((N, 3), device=dev)
    nobs, rew, nrew = torch.zeros((N, 3), device=dev), torch.zeros(N, device=dev), \
        torch.zeros(N, device=dev)
    done, ep = torch.zeros(N, device=dev), torch.zeros((N, 5), device=dev)
    torque = rn(N)
    return {
        "gauss_head_sample": lambda: ops.gauss_head_sample(mean, logstd, z, value, act, lp, val),
        "gauss_head_torch": head_torch,
        "gauss_ppo_loss_fwd_bwd": lambda: ops.gauss_ppo_loss_fwd_bwd(
            mm, logstd, mv, ma, olp, adv, ret, vold, adv_stats=stats_in, dmean=dmean,
            dvalue=dvalue, dlogstd=dls, stats=st, **hyper),
        "gauss_ppo_loss_torch": loss_torch,
        "pendulum_step_fused": lambda: ops.pendulum_step(1, torque, state, counters, nobs, nrew,
                                                         done, ep, norm_state=norm),
        "pendulum_step_raw": lambda: ops.pendulum_step(1, torque, state, counters, obs, rew, done,
                                                       ep, final_obs_out=fin),
        "env_normalize": lambda: ops.env_normalize(obs, norm, nobs, rew, nrew, fin,
                                                   truncated=done),
    }


def trainer_rate(dev, envs: int, steps: int, fused: bool, iters: int):
    C.FUSED_CONT = fused
    args = C.finalize(C.ContPPOArgs(num_envs=envs, num_steps=steps,
                                    total_timesteps=envs * steps * 100_000, save_model=False))
    tr = C.ContPPOTrainer(args, dev, log=False)
    try:
        for _ in range(3):  # eager, capture, one replay
            tr.train_iteration(collect_metrics=False)
        assert tr.graphs_ready
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            tr.train_iteration(collect_metrics=False)
        torch.cuda.synchronize()
        return envs * steps * iters / (time.perf_counter() - t0)
    finally:
        tr.close()
        C.FUSED_CONT = True


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-trainer", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    groups = [({"envs": n, "minibatch": 64}, kernel_cases(dev, n, 64)) for n, _ in WORKLOADS]
    for run in (1, 2):  # alternating: every case once per round
        for shape, cases in groups:
            for name, body in cases.items():
                us = replay_time_us(body, reps=16, rounds=3)
                print(json.dumps({"case": name, **shape, "run": run, "us": round(us, 2)}),
                      flush=True)
    if not a.skip_trainer:
        for run in (1, 2, 3):
            for envs, steps in WORKLOADS:
                for fused in (True, False):
                    sps = trainer_rate(dev, envs, steps, fused, a.iters)
                    print(json.dumps({"case": "trainer", "envs": envs, "steps": steps,
                                      "fused": fused, "run": run, "env_steps_per_s": round(sps)}),
                          flush=True)


if __name__ == "__main__":
    main()
