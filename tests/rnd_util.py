"""The steps of cleanrl/ppo_rnd_envpool.py beyond PPO, restated in plain torch / NumPy ops.
Dtype-generic: run on float64 copies of f32 inputs they are the float64 twin; run in float32 they
are "torch's own computation", whose error sets the bound.

The error rule is the project's (lstm_util.check): a tensor's error against the f64 twin, relative
to the twin's largest element, is at most max(3 x the f32 computation's own error, 4 * 2^-23).
For the f64 running statistics the rule is transposed (check64): the twin is exact (rational
arithmetic on the f32 / f64 inputs, rounded once), the "own" error is NumPy's f64 result, the
floor 4 * 2^-52.

The update mask's stream (ocppo_rnd_aux_loss_fwd_bwd / ocppo_rnd_mask) is restated in Python
integers (mask_ref).
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

from lstm_util import check, rel_err, trunk  # noqa: F401  (re-exported for the tests)

FLOOR64 = 4 * 2.0 ** -52


def check64(name, got, own, twin):
    """The rule for an f64 statistic: prints (measured, NumPy's own), asserts."""
    e, o = rel_err(got, twin), rel_err(own, twin)
    print(f"{name}: {e:.3g} / {o:.3g}")
    assert e <= max(3 * o, FLOOR64), (name, e, o)
    return e, o


# ---- RunningMeanStd (gym), f64 -----------------------------------------------------------------------
def rms_init(C: int):
    return np.zeros(C), np.ones(C), 1e-4


def rms_merge(mean, var, count, bm, bv, bc):
    """update_from_moments, in whatever arithmetic the operands carry."""
    delta = bm - mean
    tot = count + bc
    new_mean = mean + delta * bc / tot
    m2 = var * count + bv * bc + delta * delta * count * bc / tot
    return new_mean, m2 / tot, tot


def rms_update_np(state, x):
    """NumPy's f64 RunningMeanStd.update(x): x [R, C]."""
    x = np.asarray(x, np.float64)
    return rms_merge(*state, x.mean(0), x.var(0), x.shape[0])


def rms_update_exact(state, x):
    """The same in rational arithmetic from the same f64 state, rounded to f64 at the end:
    returns ((mean, var, count) as f64 arrays, the rational state for a further update)."""
    x = np.asarray(x, np.float64)
    R, C = x.shape
    mean, var, count = state
    fr = (lambda v: v if isinstance(v, Fraction) else Fraction(float(v)))  # noqa: E731
    out_m, out_v = [], []
    cnt = fr(count)
    for c in range(C):
        col = [Fraction(float(v)) for v in x[:, c]]
        bm = sum(col) / R
        bv = sum((v - bm) ** 2 for v in col) / R
        m, v, tot = rms_merge(fr(mean[c]), fr(var[c]), cnt, bm, bv, Fraction(R))
        out_m.append(m)
        out_v.append(v)
    exact = (out_m, out_v, tot)
    return (np.array([float(v) for v in out_m]), np.array([float(v) for v in out_v]),
            float(tot)), exact


def normalize_ref(x, mean, var):
    """((x - mean) / sqrt(var)).clip(-5, 5) in f64 (:365-370 before .float())."""
    x = np.asarray(x, np.float64)
    return np.clip((x - mean) / np.sqrt(var), -5, 5)


def curiosity_ref(pred, target):
    """(target - pred).pow(2).sum(1) / 2 in the operands' dtype (:373)."""
    return (target - pred).pow(2).sum(1) / 2


# ---- reward filter + running variance (:390-400) ---------------------------------------------------
def reward_filter_np(cur, rewems, int_gamma: float):
    """The script's RewardForwardFilter over cur.T in f32 NumPy: cur [T, N] f32, rewems [T] f32
    or None -> (per_env [N, T] f32, rewems)."""
    out = []
    for rews in np.asarray(cur, np.float32).T:
        rewems = rews if rewems is None else rewems * int_gamma + rews
        out.append(rewems)
    return np.array(out), rewems


def reward_stats_np(state, per_env):
    """update_from_moments(mean, std^2, len(per_env)) in NumPy f64 on the f32 filter output."""
    p = np.asarray(per_env, np.float64)
    return rms_merge(*state, p.mean(), p.std() ** 2, len(p))


def reward_stats_exact(state, per_env):
    vals = [Fraction(float(v)) for v in np.asarray(per_env, np.float64).reshape(-1)]
    bm = sum(vals) / len(vals)
    bv = sum((v - bm) ** 2 for v in vals) / len(vals)
    m, v, c = rms_merge(*(Fraction(float(s)) for s in state), bm, bv, Fraction(len(per_env)))
    return float(m), float(v), float(c)


# ---- both GAE scans (:406-442) -----------------------------------------------------------------------
def gae_ref(rewards, ext_values, dones, next_ext, next_done, curiosity, int_values, next_int,
            gamma, int_gamma, gae_lambda, int_coef, ext_coef):
    """The script's loop on [T, N] tensors of one dtype: (ext_adv, ext_ret, int_adv, int_ret,
    combined adv)."""
    T = rewards.shape[0]
    ext_adv, int_adv = torch.zeros_like(rewards), torch.zeros_like(curiosity)
    ext_last = int_last = 0
    for t in reversed(range(T)):
        if t == T - 1:
            ext_nnt, int_nnt = 1.0 - next_done, 1.0
            ext_nv, int_nv = next_ext, next_int
        else:
            ext_nnt, int_nnt = 1.0 - dones[t + 1], 1.0
            ext_nv, int_nv = ext_values[t + 1], int_values[t + 1]
        ext_delta = rewards[t] + gamma * ext_nv * ext_nnt - ext_values[t]
        int_delta = curiosity[t] + int_gamma * int_nv * int_nnt - int_values[t]
        ext_adv[t] = ext_last = ext_delta + gamma * gae_lambda * ext_nnt * ext_last
        int_adv[t] = int_last = int_delta + int_gamma * gae_lambda * int_nnt * int_last
    return (ext_adv, ext_adv + ext_values, int_adv, int_adv + int_values,
            int_adv * int_coef + ext_adv * ext_coef)


# ---- the update mask's stream ------------------------------------------------------------------------
MASK64 = (1 << 64) - 1
RND_MASK_KEY = 0x52E4D0A5C3B17F29


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def unit53(h: int) -> float:
    return (h >> 11) * (1.0 / 9007199254740992.0)


def mask_ref(seed: int, counter: int, M: int, update_proportion: float):
    h = splitmix64((splitmix64((seed & MASK64) ^ RND_MASK_KEY) + counter) & MASK64)
    return torch.tensor([1.0 if unit53(splitmix64((h + r + 1) & MASK64)) < update_proportion
                         else 0.0 for r in range(M)], dtype=torch.float32)


# ---- intrinsic value loss + masked forward loss (:463-472, :509) -----------------------------------
def aux_ref(pred, target, v_int, ret_int, mask, vf_coef: float, dtype):
    """(stats [3], dpred, dv_int) of loss = vf_coef * int_v_loss + forward_loss by autograd on
    `dtype` copies, given the mask."""
    c = lambda t: t.detach().cpu().to(dtype)  # noqa: E731
    p, v = c(pred).requires_grad_(), c(v_int).requires_grad_()
    m = c(mask)
    fl = F.mse_loss(p, c(target), reduction="none").mean(-1)
    fwd = (fl * m).sum() / torch.max(m.sum(), torch.tensor([1], dtype=dtype))
    int_v = 0.5 * ((v - c(ret_int)) ** 2).mean()
    (int_v * vf_coef + fwd).sum().backward()
    return torch.stack([int_v.detach(), fwd.detach().view(()), m.sum()]), p.grad, v.grad


# ---- the networks from their state dicts ---------------------------------------------------------------
def agent_ref(p: dict, x):
    """RNDAgent (RND_OBJ) on the state dict p: (logits, ext value, int value)."""
    h = trunk(p, x, False)
    lin = lambda k, t: t @ p[k + ".weight"].t() + p[k + ".bias"]  # noqa: E731
    logits = lin("actor.2", F.relu(lin("actor.0", h)))
    s = F.relu(lin("extra_layer.0", h)) + h
    return logits, lin("critic_ext", s), lin("critic_int", s)


def rnd_features_ref(p: dict, x, which: str):
    """RNDModel (RND_OBJ) predictor / target features on the state dict p."""
    idx = sorted({int(k.split(".")[1]) for k in p if k.startswith(which + ".")})
    h = x
    for n, i in enumerate(idx):
        h = h @ p[f"{which}.{i}.weight"].t() + p[f"{which}.{i}.bias"]
        if n < 2:
            h = F.leaky_relu(h)
        elif n + 1 < len(idx):
            h = F.relu(h)
    return h


def ppo_loss_ref(logits, value, actions, logprobs, adv, returns, values, a):
    """The script's policy + extrinsic value loss (:473-507) on one minibatch."""
    dist = torch.distributions.Categorical(logits=logits)
    logratio = dist.log_prob(actions) - logprobs
    ratio = logratio.exp()
    if a.norm_adv:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - a.clip_coef, 1 + a.clip_coef)).mean()
    v = value.view(-1)
    if a.clip_vloss:
        vc = values + torch.clamp(v - values, -a.clip_coef, a.clip_coef)
        vl = 0.5 * torch.max((v - returns) ** 2, (vc - returns) ** 2).mean()
    else:
        vl = 0.5 * ((v - returns) ** 2).mean()
    return pg - a.ent_coef * dist.entropy().mean() + vl * a.vf_coef


class AdamRef:
    """torch.optim.Adam (eps as given, no weight decay) on a list of tensors, in their dtype."""

    def __init__(self, params, eps: float = 1e-5, betas=(0.9, 0.999)):
        self.params = [p.clone() for p in params]
        self.m = [torch.zeros_like(p) for p in params]
        self.v = [torch.zeros_like(p) for p in params]
        self.t, self.eps, self.betas, self.lr = 0, eps, betas, 0.0

    def step(self, grads):
        b1, b2 = self.betas
        self.t += 1
        for p, m, v, g in zip(self.params, self.m, self.v, grads):
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = v.sqrt() / (1 - b2 ** self.t) ** 0.5 + self.eps
            p.addcdiv_(m, denom, value=-self.lr / (1 - b1 ** self.t))


def clip_coef(grads, max_norm: float):
    total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads)).to(grads[0].dtype)
    return torch.clamp(max_norm / (total + 1e-6), max=1.0), total
