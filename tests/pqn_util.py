"""PQN (cleanrl/pqn_atari_envpool.py) restated in plain torch ops on tensors and state dicts.
Dtype-generic: run on float64 copies of f32 inputs it is the float64 twin; run in float32 it is
"the f32 torch computation" whose own error sets the bound.

The error rule of DESIGN.md 11 (lstm_util.check): a tensor's error against the f64 twin, relative
to the twin's largest element, is at most max(3 x the f32 torch computation's own error,
4 * 2^-23). Bitwise where a test says so.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from lstm_util import FLOOR, bound, check, rel_err  # noqa: F401  (the rule, shared)


def q_lambda_ref(rewards, values, dones, next_q, next_done, gamma: float, q_lambda: float):
    """pqn_atari_envpool.py:248-261, the loop as written (Python scalars times tensors, so torch
    rounds gamma, q_lambda and 1 - q_lambda to the tensors' dtype once each)."""
    T = rewards.shape[0]
    returns = torch.zeros_like(rewards)
    for t in reversed(range(T)):
        if t == T - 1:
            next_value, _ = torch.max(next_q, dim=-1)
            nextnonterminal = 1.0 - next_done
            returns[t] = rewards[t] + gamma * next_value * nextnonterminal
        else:
            nextnonterminal = 1.0 - dones[t + 1]
            next_value = values[t + 1]
            returns[t] = (rewards[t] + gamma * (q_lambda * returns[t + 1]
                                                + (1 - q_lambda) * next_value) * nextnonterminal)
    return returns


def ln_relu_ref(x, weight, bias, eps: float = 1e-5, relu: bool = True):
    y = F.layer_norm(x, (x.shape[-1],), weight, bias, eps)
    return F.relu(y) if relu else y


def ln_relu_case(x, weight, bias, dy, eps, relu, dtype):
    """y, mean, rstd and the gradients of sum(y * dy) on `dtype` CPU copies."""
    cast = lambda t: t.detach().cpu().to(dtype)  # noqa: E731
    x, w, b = (cast(t).requires_grad_() for t in (x, weight, bias))
    y = ln_relu_ref(x, w, b, eps, relu)
    (y * cast(dy)).sum().backward()
    mean = x.detach().mean(-1)
    var = ((x.detach() - mean.unsqueeze(-1)) ** 2).mean(-1)
    return dict(y=y.detach(), mean=mean, rstd=1.0 / torch.sqrt(var + eps), dx=x.grad, dw=w.grad,
                db=b.grad)


def q_network_ref(p: dict, x):
    """The Linear -> LayerNorm -> ReLU stack and Q head from a state dict `p` with keys
    network.<i>.weight / .bias as PQNetwork("PQN_OBJ") names them: a 1-D weight is a LayerNorm, a
    2-D one a Linear; the Flatten sits where a Linear's input width changes; the last Linear is
    the Q head (no norm, no ReLU). x [rows, W, F]."""
    idx = sorted({int(k.split(".")[1]) for k in p if k.startswith("network.")})
    h = x
    for n, i in enumerate(idx):
        w, b = p[f"network.{i}.weight"], p[f"network.{i}.bias"]
        if w.dim() == 1:
            h = F.relu(F.layer_norm(h, (w.shape[0],), w, b, 1e-5))
        else:
            if h.shape[-1] != w.shape[1]:
                h = h.flatten(1)
            h = h @ w.t() + b
    return h


def linear_schedule(start_e: float, end_e: float, duration: float, t: int) -> float:
    """pqn_atari_envpool.py:141-143."""
    slope = (end_e - start_e) / duration
    return max(slope * t + start_e, end_e)


def mse_step(q, actions, returns):
    """:276-277 and the backward: (loss, mean q(s, a), dq)."""
    q = q.detach().clone().requires_grad_()
    old_val = q.gather(1, actions.unsqueeze(-1).long()).squeeze(-1)
    loss = F.mse_loss(returns, old_val)
    loss.backward()
    return loss.detach(), old_val.detach().mean(), q.grad


def clip_coef(grads, max_norm: float):
    """nn.utils.clip_grad_norm_'s coefficient for the list of gradients."""
    total = torch.sqrt(sum((g.double() ** 2).sum() for g in grads)).to(grads[0].dtype)
    return torch.clamp(max_norm / (total + 1e-6), max=1.0), total


class RAdamRef:
    """torch.optim.RAdam (defaults: betas (0.9, 0.999), eps 1e-8, no weight decay) from the
    formula of its documentation, on plain tensors of any float dtype."""

    def __init__(self, params, lr: float, betas=(0.9, 0.999), eps: float = 1e-8):
        self.params = params
        self.lr, self.betas, self.eps = lr, betas, eps
        self.m = [torch.zeros_like(p) for p in params]
        self.v = [torch.zeros_like(p) for p in params]
        self.t = 0

    def step(self, grads):
        b1, b2 = self.betas
        self.t += 1
        t = self.t
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        rho_inf = 2 / (1 - b2) - 1
        rho_t = rho_inf - 2 * t * (b2 ** t) / bc2
        for p, g, m, v in zip(self.params, grads, self.m, self.v):
            m.lerp_(g, 1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            mhat = m / bc1
            if rho_t > 5.0:
                rect = math.sqrt((rho_t - 4) * (rho_t - 2) * rho_inf /
                                 ((rho_inf - 4) * (rho_inf - 2) * rho_t))
                adaptive = math.sqrt(bc2) / (v.sqrt() + self.eps)
                p.add_(mhat * self.lr * adaptive * rect * -1.0)
            else:
                p.add_(mhat * self.lr * -1.0)
        return rho_t
