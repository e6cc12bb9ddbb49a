"""Discrete SAC (cleanrl/sac_atari.py:283-335) restated in plain torch ops on tensors and state
dicts. Dtype-generic: run on float64 copies of f32 inputs it is the float64 twin; run in float32 it
is "the f32 torch computation" whose own error sets the bound.

The error rule of DESIGN.md 11 (lstm_util.check): a tensor's error against the f64 twin, relative
to the twin's largest element, is at most max(3 x the f32 torch computation's own error,
4 * 2^-23).

The acting stream of ocppo_sac_act is restated in Python integers and f64 (act_ref).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from lstm_util import FLOOR, bound, check, rel_err  # noqa: F401  (the rule, shared)

class Checks:
    """The rule over many tensors: every pair is measured and printed, `done()` asserts that none
    missed (so one miss does not hide the figures after it)."""

    def __init__(self):
        self.missed = []

    def check(self, name, got, f32, twin):
        e, own = rel_err(got, twin), rel_err(f32, twin)
        print(f"{name}: {e:.3g} / {own:.3g}")
        if not e <= bound(own):
            self.missed.append((name, e, own))

    def done(self):
        assert not self.missed, self.missed


M64 = (1 << 64) - 1
SAC_ACT_KEY = 0x5AC0D15C2E7E5EED  # kSacActKey (csrc/ocppo_sac.hip)


# ---- the networks as plain ops on a state dict -----------------------------------------------------
def mlp_ref(p: dict, x, prefix: str = "network."):
    """The PPObj Linear / ReLU stack + head of ActorObj / SoftQNetworkObj: every Linear but the
    last is followed by a ReLU; the Flatten sits where a Linear's input width changes."""
    idx = sorted({int(k[len(prefix):].split(".")[0]) for k in p if k.startswith(prefix)})
    h = x
    for n, i in enumerate(idx):
        w, b = p[f"{prefix}{i}.weight"], p[f"{prefix}{i}.bias"]
        if h.shape[-1] != w.shape[1]:
            h = h.flatten(1)
        h = h @ w.t() + b
        if n + 1 < len(idx):
            h = F.relu(h)
    return h


def get_action_ref(logits):
    """Actor.get_action's (log_pi, probs) (:165-169)."""
    probs = torch.distributions.Categorical(logits=logits).probs
    return F.log_softmax(logits, dim=1), probs


# ---- the two loss blocks -------------------------------------------------------------------------------
def critic_ref(next_logits, q1t, q2t, q1, q2, actions, rewards, dones, gamma: float, alpha: float):
    """:283-302 with the gradients w.r.t. q1 / q2 by autograd. alpha: a Python float (the script
    holds `.item()`)."""
    q1 = q1.detach().clone().requires_grad_()
    q2 = q2.detach().clone().requires_grad_()
    with torch.no_grad():
        logp, p = get_action_ref(next_logits)
        v = (p * (torch.min(q1t, q2t) - alpha * logp)).sum(dim=1)
        y = rewards.flatten() + (1 - dones.flatten()) * gamma * v
    a = actions.view(-1, 1).long()
    q1a, q2a = q1.gather(1, a).view(-1), q2.gather(1, a).view(-1)
    l1, l2 = F.mse_loss(q1a, y), F.mse_loss(q2a, y)
    (l1 + l2).backward()
    return dict(y=y, qf1_loss=l1.detach(), qf2_loss=l2.detach(), qf1_values=q1a.detach().mean(),
                qf2_values=q2a.detach().mean(), dq1=q1.grad, dq2=q2.grad)


def actor_ref(logits, q1, q2, alpha: float, log_alpha, target_entropy: float):
    """:309-328 without the optimizer steps: the policy loss with d / d logits and the temperature
    loss with d / d log_alpha, both by autograd. log_alpha: a one-element tensor."""
    logits = logits.detach().clone().requires_grad_()
    log_alpha = log_alpha.detach().clone().requires_grad_()
    logp, p = get_action_ref(logits)
    minq = torch.min(q1, q2).detach()
    actor_loss = (p * ((alpha * logp) - minq)).mean()
    actor_loss.backward()
    alpha_loss = (p.detach() * (-log_alpha.exp() * (logp + target_entropy).detach())).mean()
    alpha_loss.backward()
    return dict(actor_loss=actor_loss.detach(), dlogits=logits.grad,
                alpha_loss=alpha_loss.detach(), dlog_alpha=log_alpha.grad,
                entropy=-(p * logp).sum(1).mean().detach())


def dlogits_formula(logits, q1, q2, alpha: float):
    """The kernel's hand-written gradient: p_k (g_k - sum_j p_j g_j) / (B A) with
    g = alpha * logp - min(q1, q2) (the alpha * p * dlogp terms cancel), in the form the kernel
    evaluates, p_k sum_j p_j (g_k - g_j) / (B A)."""
    logp, p = get_action_ref(logits)
    g = alpha * logp - torch.min(q1, q2)
    diff = g.unsqueeze(2) - g.unsqueeze(1)  # [B, k, j] = g_k - g_j
    return p * (p.unsqueeze(1) * diff).sum(2) / logits.numel()


# ---- the acting stream (ocppo_sac_act) --------------------------------------------------------------
def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def unit53(h: int) -> float:
    return (h >> 11) * (1.0 / 9007199254740992.0)


def act_ref(logits, seed: int, t: int, learning_starts: int):
    """(actions, gap) for logits [E, A]: the action of every env at global step t and, in the
    sampling phase, the relative gap between the two largest p_j / e_j of the row (inf for A = 1
    and in the random phase)."""
    E, A = logits.shape
    ht = splitmix64((splitmix64((seed & M64) ^ SAC_ACT_KEY) + t) & M64)
    p = torch.distributions.Categorical(logits=logits.double().cpu()).probs.tolist()
    actions, gaps = [], []
    for e in range(E):
        he = splitmix64((ht + e + 1) & M64)
        if t < learning_starts:
            actions.append(he % A)
            gaps.append(math.inf)
            continue
        r = []
        for j in range(A):
            u = unit53(splitmix64((he + j + 1) & M64))
            ej = -math.log(1.0 - u)
            r.append(p[e][j] / ej if ej > 0 else math.inf)
        best = max(range(A), key=lambda j: (r[j], -j))  # first maximum
        actions.append(best)
        top = sorted(r, reverse=True)
        gaps.append(math.inf if A == 1 or top[0] == 0 else (top[0] - top[1]) / top[0])
    return actions, gaps


# ---- the whole update (:283-335) on state dicts ----------------------------------------------------
class SACRef:
    """The script's train step on `dtype` copies of three state dicts (the object-vector networks
    of mlp_ref), with torch.optim.Adam(eps=1e-4) three times as at :223-231 and alpha carried as a
    Python float."""

    def __init__(self, actor_sd, qf1_sd, qf2_sd, dtype, gamma, q_lr, policy_lr, target_entropy,
                 autotune=True, alpha=0.2):
        leaf = lambda sd: {k: v.detach().cpu().to(dtype).clone().requires_grad_()  # noqa: E731
                           for k, v in sd.items()}
        self.actor, self.qf1, self.qf2 = leaf(actor_sd), leaf(qf1_sd), leaf(qf2_sd)
        self.qf1_t = {k: v.detach().clone() for k, v in self.qf1.items()}
        self.qf2_t = {k: v.detach().clone() for k, v in self.qf2.items()}
        self.dtype, self.gamma, self.te, self.autotune = dtype, gamma, target_entropy, autotune
        self.q_opt = torch.optim.Adam(list(self.qf1.values()) + list(self.qf2.values()), lr=q_lr,
                                      eps=1e-4)
        self.a_opt = torch.optim.Adam(list(self.actor.values()), lr=policy_lr, eps=1e-4)
        if autotune:
            self.log_alpha = torch.zeros(1, dtype=dtype, requires_grad=True)
            self.alpha = self.log_alpha.exp().item()
            self.t_opt = torch.optim.Adam([self.log_alpha], lr=q_lr, eps=1e-4)
        else:
            self.alpha = alpha

    def update(self, d: dict) -> dict:
        c = lambda t: t.detach().cpu().to(self.dtype)  # noqa: E731
        obs, nxt = c(d["observations"]), c(d["next_observations"])
        rewards, dones, actions = c(d["rewards"]), c(d["dones"]), d["actions"].cpu().long()
        alpha = self.alpha
        with torch.no_grad():
            nlogp, np_ = get_action_ref(mlp_ref(self.actor, nxt))
            q1n, q2n = mlp_ref(self.qf1_t, nxt), mlp_ref(self.qf2_t, nxt)
            v = (np_ * (torch.min(q1n, q2n) - alpha * nlogp)).sum(dim=1)
            y = rewards.flatten() + (1 - dones.flatten()) * self.gamma * v
        q1a = mlp_ref(self.qf1, obs).gather(1, actions.view(-1, 1)).view(-1)
        q2a = mlp_ref(self.qf2, obs).gather(1, actions.view(-1, 1)).view(-1)
        l1, l2 = F.mse_loss(q1a, y), F.mse_loss(q2a, y)
        self.q_opt.zero_grad()
        (l1 + l2).backward()
        self.q_opt.step()
        logp, p = get_action_ref(mlp_ref(self.actor, obs))
        with torch.no_grad():
            minq = torch.min(mlp_ref(self.qf1, obs), mlp_ref(self.qf2, obs))
        actor_loss = (p * ((alpha * logp) - minq)).mean()
        self.a_opt.zero_grad()
        actor_loss.backward()
        self.a_opt.step()
        alpha_loss = torch.zeros((), dtype=self.dtype)
        if self.autotune:
            alpha_loss = (p.detach() * (-self.log_alpha.exp() * (logp + self.te).detach())).mean()
            self.t_opt.zero_grad()
            alpha_loss.backward()
            self.t_opt.step()
            self.alpha = self.log_alpha.exp().item()
        return {"losses/qf1_values": q1a.mean().item(), "losses/qf2_values": q2a.mean().item(),
                "losses/qf1_loss": l1.item(), "losses/qf2_loss": l2.item(),
                "losses/qf_loss": (l1 + l2).item() / 2.0, "losses/actor_loss": actor_loss.item(),
                "losses/alpha": self.alpha, "losses/alpha_loss": alpha_loss.item()}
