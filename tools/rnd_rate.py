"""Rates of the RND learner and its six kernels.

    python tools/rnd_rate.py [--skip-trainer] [--iters K]

  kernels  each of ops.rms_update, rnd_normalize (batch and rollout rows), rnd_curiosity,
           rnd_reward_norm, rnd_gae and rnd_aux_loss_fwd_bwd against the torch ops
           rnd.RNDTrainer runs in its place with FUSED_RND off, on one trainer's own buffers at
           the script's 128 envs x 128 steps (4 minibatches, the default RND_OBJ networks), timed
           by graph replay (trainer.replay_time_us), warm; two alternating runs
  trainer  env steps/s of rnd.RNDTrainer at that size on the Synthetic object env, FUSED_RND on
           and off: three eager / capture / replay warm-up iterations, then K replayed iterations
           timed by the host clock around a device synchronise; the two settings alternate,
           three rounds, every round printed (the median is the figure to quote)
Prints one JSON line per case and run.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from oc_cleanrl_amd import ops  # noqa: E402
from oc_cleanrl_amd import rnd as R  # noqa: E402
from oc_cleanrl_amd.trainer import replay_time_us  # noqa: E402

ENVS, STEPS = 128, 128


def _args(warmup_rounds: int = 1):
    return R.finalize(R.RNDArgs(num_envs=ENVS, num_steps=STEPS,
                                num_iterations_obs_norm_init=warmup_rounds,
                                total_timesteps=ENVS * STEPS * 100_000, save_model=False))


def kernel_cases(tr):
    """{case: (kernel closure, torch closure)} on the trainer's buffers after one iteration."""
    a, T, M = tr.args, tr.T, tr.M
    batch, step = tr._newest(tr.obs[:T]), tr._newest(tr.obs[1])
    x = tr.rnd_obs[:M].contiguous()
    with torch.no_grad():
        pf_n, tf_n = tr.rnd.predict_features(tr.rnd_in), tr.rnd.target_features(tr.rnd_in)
        pf, tf = tr.rnd.predict_features(x), tr.rnd.target_features(x)
    vi, ret = tr.int_values[:T].reshape(-1)[:M].contiguous(), tr.int_returns.view(-1)[:M]
    stats = torch.zeros(3, device=tr.dev)

    def torch_path(fn):
        def body():
            tr.fused = False
            try:
                fn()
            finally:
                tr.fused = True
        return body

    def aux_torch():
        p, v = pf.detach().requires_grad_(), vi.detach().requires_grad_()
        mask = ops.rnd_mask(tr.seed, tr.mask_counter, M, a.update_proportion)
        tr.mask_counter.add_(1)
        fwd = F.mse_loss(p, tf, reduction="none").mean(-1)
        fwd = (fwd * mask).sum() / torch.clamp(mask.sum(), min=1.0)
        (0.5 * ((v - ret) ** 2).mean() * a.vf_coef + fwd).backward()

    gae = lambda: ops.rnd_gae(  # noqa: E731
        tr.rewards, tr.ext_values[:T], tr.dones[:T], tr.ext_values[T], tr.dones[T], tr.curiosity,
        tr.int_values[:T], tr.int_values[T], a.gamma, a.int_gamma, a.gae_lambda, a.int_coef,
        a.ext_coef, tr.ext_advantages, tr.ext_returns, tr.int_advantages, tr.int_returns,
        tr.advantages)
    return {
        "rms_update": (lambda: ops.rms_update(batch, tr.obs_rms),
                       torch_path(lambda: tr._rms_update(batch))),
        "rnd_normalize_batch": (lambda: ops.rnd_normalize(batch, tr.obs_rms, tr.rnd_obs),
                                torch_path(lambda: tr._normalize(batch, tr.rnd_obs))),
        "rnd_normalize_step": (lambda: ops.rnd_normalize(step, tr.obs_rms, tr.rnd_in),
                               torch_path(lambda: tr._normalize(step, tr.rnd_in))),
        "rnd_curiosity": (lambda: ops.rnd_curiosity(pf_n, tf_n, tr.curiosity[0]),
                          lambda: tr.curiosity[0].copy_((tf_n - pf_n).pow(2).sum(1) / 2)),
        "rnd_reward_norm": (lambda: ops.rnd_reward_norm(tr.curiosity, tr.rewems, tr.reward_rms,
                                                        a.int_gamma),
                            tr._reward_norm_torch),
        "rnd_gae": (gae, tr._gae_torch),
        "rnd_aux_loss": (lambda: ops.rnd_aux_loss_fwd_bwd(
            pf, tf, vi, ret, tr.seed, tr.mask_counter, a.update_proportion, a.vf_coef, tr.dpred,
            tr.dv_int, stats), aux_torch),
    }


def trainer_rate(dev, fused: bool, iters: int):
    R.FUSED_RND = fused
    tr = R.RNDTrainer(_args(), dev, log=False)
    try:
        for _ in range(3):  # eager, capture, one replay
            tr.train_iteration(collect_metrics=False)
        assert tr.graphs_ready
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            tr.train_iteration(collect_metrics=False)
        torch.cuda.synchronize()
        return ENVS * STEPS * iters / (time.perf_counter() - t0)
    finally:
        tr.close()
        R.FUSED_RND = True


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-trainer", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    tr = R.RNDTrainer(_args(), dev, log=False)
    tr.args.cuda_graphs = False
    tr.train_iteration(collect_metrics=False)
    cases = kernel_cases(tr)
    for run in (1, 2):  # alternating: every case once per round
        for name, (hip, ref) in cases.items():
            for kind, body in (("hip", hip), ("torch", ref)):
                us = replay_time_us(body, reps=8, rounds=3)
                print(json.dumps({"case": name, "path": kind, "run": run, "us": round(us, 2)}),
                      flush=True)
    tr.close()
    if not a.skip_trainer:
        for run in (1, 2, 3):
            for fused in (True, False):
                sps = trainer_rate(dev, fused, a.iters)
                print(json.dumps({"case": "trainer", "envs": ENVS, "steps": STEPS, "fused": fused,
                                  "run": run, "env_steps_per_s": round(sps)}), flush=True)


if __name__ == "__main__":
    main()
