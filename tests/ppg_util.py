"""The steps of cleanrl/ppg_procgen.py beyond PPO, restated in plain torch ops. Dtype-generic: run
on float64 copies of f32 inputs they are the float64 twin; run in float32 they are "torch's own
computation", whose error sets the bound.

The error rule is the project's (lstm_util.check): a tensor's error against the f64
twin, relative to the twin's largest element, is at most max(3 x the f32 computation's own error,
4 * 2^-23).
"""
from __future__ import annotations

import torch
import torch.distributions as td

from lstm_util import check, rel_err, trunk  # noqa: F401  (re-exported for the tests)
from rnd_util import AdamRef, clip_coef, ppo_loss_ref  # noqa: F401


def flatten01(arr):
    return arr.reshape((-1, *arr.shape[2:]))


def aux_ref(new_logits, new_value, new_aux, old_logits, returns, beta_clone: float, dtype):
    """(stats [3] = {kl_loss, aux_value_loss, real_value_loss}, dlogits, dvalue, daux) of the
    script's joint loss (:453-461) by autograd on `dtype` copies."""
    c = lambda t: t.detach().cpu().to(dtype)  # noqa: E731
    lg, v, av = (c(t).requires_grad_() for t in (new_logits, new_value, new_aux))
    ret = c(returns)
    old_pi = td.Categorical(logits=c(old_logits))
    kl = td.kl_divergence(old_pi, td.Categorical(logits=lg)).mean()
    real = 0.5 * ((v - ret) ** 2).mean()
    auxl = 0.5 * ((av - ret) ** 2).mean()
    ((auxl + beta_clone * kl) + real).backward()
    return torch.stack([kl.detach(), auxl.detach(), real.detach()]), lg.grad, v.grad, av.grad


def aux_losses(logits, value, aux_value, old_logits, returns):
    """(kl_loss, aux_value_loss, real_value_loss), differentiable, in the operands' dtype."""
    kl = td.kl_divergence(td.Categorical(logits=old_logits), td.Categorical(logits=logits)).mean()
    return (kl, 0.5 * ((aux_value - returns) ** 2).mean(),
            0.5 * ((value - returns) ** 2).mean())


def agent_ref(p: dict, x):
    """PPGAgent (PPG_OBJ) on the state dict p: (logits, value on the detached trunk output, aux
    value)."""
    h = trunk(p, x, False)
    lin = lambda k, t: t @ p[k + ".weight"].t() + p[k + ".bias"]  # noqa: E731
    return lin("actor", h), lin("critic", h.detach()), lin("aux_critic", h)


def policy_loss_ref(logits, value, actions, logprobs, adv, returns, values, a):
    """The script's policy-phase loss (:356-389) on one minibatch; adv is already normalised."""
    dist = td.Categorical(logits=logits)
    ratio = (dist.log_prob(actions) - logprobs).exp()
    pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - a.clip_coef, 1 + a.clip_coef)).mean()
    v = value.view(-1)
    if a.clip_vloss:
        vc = values + torch.clamp(v - values, -a.clip_coef, a.clip_coef)
        vl = 0.5 * torch.max((v - returns) ** 2, (vc - returns) ** 2).mean()
    else:
        vl = 0.5 * ((v - returns) ** 2).mean()
    return pg - a.ent_coef * dist.entropy().mean() + vl * a.vf_coef


class SegAdamRef(AdamRef):
    """torch.optim.Adam with a step count per parameter: a parameter whose gradient is None is
    skipped (its moments and count stay)."""

    def __init__(self, params, eps: float = 1e-8, betas=(0.9, 0.999)):
        super().__init__(params, eps, betas)
        self.ts = [0] * len(self.params)

    def step(self, grads):
        b1, b2 = self.betas
        for i, (p, m, v, g) in enumerate(zip(self.params, self.m, self.v, grads)):
            if g is None:
                continue
            self.ts[i] += 1
            t = self.ts[i]
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = v.sqrt() / (1 - b2 ** t) ** 0.5 + self.eps
            p.addcdiv_(m, denom, value=-self.lr / (1 - b1 ** t))
