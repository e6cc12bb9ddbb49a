"""Rates of the PPG learner and its three new entries.

    python tools/ppg_rate.py [--skip-trainer] [--phases K] [--n-iteration N]

  kernels  ops.ppg_aux_gather, ops.ppg_aux_loss_fwd_bwd and ops.FlatAdamSegments' step (tail in
           and out) against the torch ops ppg.PPGTrainer runs in their place with FUSED_PPG off, on
           one trainer's own buffers at the script's 64 envs x 256 steps (8 minibatches,
           num_aux_rollouts 4: auxiliary minibatches of 1024 rows; the default PPG_OBJ networks),
           timed by graph replay (trainer.replay_time_us), warm; two alternating runs
  trainer  env steps/s of ppg.PPGTrainer over whole phases (n_iteration policy iterations + the
           auxiliary phase) at that size on the Synthetic object env, FUSED_PPG on and off: two
           warm-up phases (eager, then capture), then K replayed phases timed by the host clock
           around a device synchronise, the policy iterations and the auxiliary phase also timed
           apart; the two settings alternate, three rounds, every round printed (the median is
           the figure to quote); then PPOTrainer (PPO_OBJ, the same networks and sizes, one epoch)
           for the policy phase's rate
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

from oc_cleanrl_amd import ops  # noqa: E402
from oc_cleanrl_amd import ppg as P  # noqa: E402
from oc_cleanrl_amd.args import Args, finalize  # noqa: E402
from oc_cleanrl_amd.trainer import PPOTrainer, replay_time_us  # noqa: E402

ENVS, STEPS = 64, 256


def _args(n_iteration: int):
    return P.finalize(P.PPGArgs(num_envs=ENVS, num_steps=STEPS, n_iteration=n_iteration,
                                total_timesteps=ENVS * STEPS * 100_000, save_model=False))


def kernel_cases(tr):
    """{case: (kernel closure, torch closure)} on the trainer's buffers after one phase."""
    a, K = tr.args, tr.K
    cols = tr.aux_perm_dev[:K]
    with torch.no_grad():
        logits, value, aux = tr.agent.heads3(tr.agent.trunk(tr.aux_mb_obs))
    logits, value, aux = logits.contiguous(), value.view(-1).contiguous(), aux.view(-1).contiguous()
    stats = torch.zeros(3, device=tr.dev)
    masked = P._MaskedAdam(tr.optimizer)

    def gather_torch():
        tr.fused = False
        try:
            tr._aux_gather(cols)
        finally:
            tr.fused = True

    def loss_torch():
        lg, v, av = (t.detach().requires_grad_() for t in (logits, value, aux))
        kl, al, rl = P.aux_losses_torch(lg, v, av, tr.aux_mb_pi, tr.aux_mb_ret)
        stats.copy_(torch.stack([kl.detach(), al.detach(), rl.detach()]))
        (al + a.beta_clone * kl + rl).backward()

    return {
        "ppg_aux_gather": (lambda: tr._aux_gather(cols), gather_torch),
        "ppg_aux_loss": (lambda: ops.ppg_aux_loss_fwd_bwd(
            logits, value, aux, tr.aux_mb_pi, tr.aux_mb_ret, a.beta_clone, tr.aux_dlogits,
            tr.aux_dvalue, tr.aux_daux, stats), loss_torch),
        "adam_seg_policy": (lambda: tr.optimizer.step(False), lambda: masked.step(False)),
        "adam_seg_aux": (lambda: tr.optimizer.step(True), lambda: masked.step(True)),
    }


def trainer_rate(dev, fused: bool, phases: int, n_iteration: int) -> dict:
    P.FUSED_PPG = fused
    tr = P.PPGTrainer(_args(n_iteration), dev, log=False)
    try:
        for _ in range(2 * n_iteration):  # an eager phase, then the captures
            tr.train_iteration(collect_metrics=False)
        assert tr.graphs_ready and tr.g_aux is not None
        inner, spent = tr.auxiliary_phase, [0.0]

        def timed_aux():
            torch.cuda.synchronize()
            t = time.perf_counter()
            m = inner()
            torch.cuda.synchronize()
            spent[0] += time.perf_counter() - t
            return m

        tr.auxiliary_phase = timed_aux
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(phases * n_iteration):
            tr.train_iteration(collect_metrics=False)
        torch.cuda.synchronize()
        total = time.perf_counter() - t0
        steps = ENVS * STEPS * n_iteration * phases
        return {"env_steps_per_s": round(steps / total),
                "policy_env_steps_per_s": round(steps / (total - spent[0])),
                "aux_phase_ms": round(1e3 * spent[0] / phases, 2)}
    finally:
        tr.close()
        P.FUSED_PPG = True


def ppo_rate(dev, iters: int) -> float:
    d = P.PPGArgs()
    args = finalize(Args(env_id=d.env_id, obs_mode="obj", architecture="PPO_OBJ", num_envs=ENVS,
                         num_steps=STEPS, num_minibatches=d.num_minibatches, update_epochs=1,
                         learning_rate=d.learning_rate, gamma=d.gamma, clip_coef=d.clip_coef,
                         anneal_lr=False, encoder_dims=d.encoder_dims, decoder_dims=d.decoder_dims,
                         total_timesteps=ENVS * STEPS * 100_000, save_model=False), 1)
    tr = PPOTrainer(args, dev, log=False)
    try:
        for _ in range(3):
            tr.train_iteration(collect_metrics=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            tr.train_iteration(collect_metrics=False)
        torch.cuda.synchronize()
        return ENVS * STEPS * iters / (time.perf_counter() - t0)
    finally:
        tr.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-trainer", action="store_true")
    ap.add_argument("--phases", type=int, default=2)
    ap.add_argument("--n-iteration", type=int, default=P.PPGArgs().n_iteration)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    tr = P.PPGTrainer(_args(1), dev, log=False)  # one iteration a phase: the buffers filled once
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
                r = trainer_rate(dev, fused, a.phases, a.n_iteration)
                print(json.dumps({"case": "trainer", "envs": ENVS, "steps": STEPS,
                                  "n_iteration": a.n_iteration, "fused": fused, "run": run, **r}),
                      flush=True)
            sps = ppo_rate(dev, a.n_iteration)
            print(json.dumps({"case": "ppo_trainer", "envs": ENVS, "steps": STEPS, "run": run,
                              "env_steps_per_s": round(sps)}), flush=True)


if __name__ == "__main__":
    main()
