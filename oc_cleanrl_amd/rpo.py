"""`python -m oc_cleanrl_amd.rpo [rpo_continuous_action.py flags]` — Robust Policy Optimization.

The same learner as `python -m oc_cleanrl_amd.contppo` (contppo.ContPPOTrainer) with
cleanrl/rpo_continuous_action.py's defaults (Args :17-79: 8M steps, rpo_alpha 0.5): during the
update, uniform noise in [-rpo_alpha, rpo_alpha) is added to the policy mean before the log-prob
(:138-141), inside ops.gauss_ppo_loss_fwd_bwd's launch. The noise is the library's own Philox
stream (ops.rpo_noise), not torch's CPU uniform_; env_id defaults to Pendulum-v1 as in contppo."""
from __future__ import annotations

from .contppo import main as _main

# rpo_continuous_action.py:17-79 where it differs from ppo_continuous_action.py's Args
RPO_DEFAULTS = dict(exp_name="rpo_continuous_action", total_timesteps=8_000_000, rpo_alpha=0.5)


def main(argv=None):
    return _main(argv, defaults=RPO_DEFAULTS,
                 description="oc_cleanrl_amd RPO (rpo_continuous_action.py surface)")


if __name__ == "__main__":
    main()
