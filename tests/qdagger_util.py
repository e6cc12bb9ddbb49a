"""QDagger's loss and episodic-return ring restated for the tests.

`loss_twin` is plain torch written from the formulas of include/ocppo.h (dtype-generic: on float64
copies of f32 inputs it is the float64 twin, in float32 it is "the f32 torch computation" whose
own error sets the bound of lstm_util.check); `loss_autograd` is the same loss under autograd, for
the trainer's restatement. `episode_ring_ref` is a Python deque(maxlen=10) plus the coefficient
formula of qdagger_dqn_atari_impalacnn.py:408-411.
"""
from __future__ import annotations

from collections import deque

import numpy as np
import torch

RING = 10


def loss_terms(q, q_next, q_teacher, actions, rewards, dones, gamma, temperature, coeff):
    """(loss, q_loss, distill, mean q(s,a)) as differentiable torch scalars."""
    dt = q.dtype
    y = rewards + torch.tensor(gamma, dtype=dt) * q_next.max(dim=1).values * (1 - dones)
    old = q.gather(1, actions.reshape(-1, 1)).squeeze(1)
    q_loss = ((y - old) ** 2).mean()
    t, s = q_teacher / temperature, q / temperature
    distill = (-torch.softmax(t, -1) * (torch.log_softmax(s, -1) - torch.log_softmax(t, -1))).sum()
    return q_loss + coeff * distill, q_loss, distill, old.mean()


def loss_twin(q, q_next, q_teacher, actions, rewards, dones, gamma, temperature, coeff,
              dtype=torch.float64):
    """stats [5] and dq [B, A] from the closed-form gradient, in `dtype`, on the host."""
    c = lambda x: x.detach().cpu().to(dtype)  # noqa: E731
    q, q_next, q_teacher, rewards, dones = map(c, (q, q_next, q_teacher, rewards, dones))
    actions = actions.detach().cpu().reshape(-1)
    coeff = 1.0 if coeff is None else float(coeff)
    B = q.shape[0]
    loss, q_loss, distill, qm = loss_terms(q, q_next, q_teacher, actions, rewards, dones, gamma,
                                           temperature, coeff)
    y = rewards + torch.tensor(gamma, dtype=dtype) * q_next.max(dim=1).values * (1 - dones)
    old = q.gather(1, actions.reshape(-1, 1)).squeeze(1)
    p_t, p_s = torch.softmax(q_teacher / temperature, -1), torch.softmax(q / temperature, -1)
    dq = (coeff / temperature) * (p_s * p_t.sum(-1, keepdim=True) - p_t)
    dq[torch.arange(B), actions] += (2.0 / B) * (old - y)
    stats = torch.stack([loss, q_loss, distill, qm, torch.tensor(coeff, dtype=dtype)])
    return stats, dq


def td_grad(q, q_next, actions, rewards, dones, gamma, dtype=torch.float64):
    """The TD half's gradient alone."""
    z = torch.zeros_like(q)
    return loss_twin(q, q_next, z, actions, rewards, dones, gamma, 1.0, 0.0, dtype)[1]


def episode_ring_ref(steps, num_envs: int, teacher_mean: float):
    """steps: a sequence of (reward [E], done [E]). Yields after every step
    (returns oldest first, run_ret [E] as float32, coefficient as float32): the script's
    `episodic_returns.append` in ascending env order and its coefficient."""
    ring: deque = deque(maxlen=RING)
    run = np.zeros(num_envs, dtype=np.float32)
    for reward, done in steps:
        for e in range(num_envs):
            run[e] = np.float32(run[e] + np.float32(reward[e]))
            if done[e]:
                ring.append(float(run[e]))
                run[e] = 0
        if len(ring) < RING:
            coeff = 1.0
        else:
            mean = 0.0
            for r in ring:  # oldest to newest, in float64
                mean += r
            coeff = max(1 - (mean / RING) / teacher_mean, 0)
        yield list(ring), run.copy(), np.float32(coeff)


def ring_layout(returns_in_push_order):
    """(ring [10] f32, head, count) of the device ring after pushing `returns_in_push_order`."""
    ring = np.zeros(RING, dtype=np.float32)
    head = count = 0
    for r in returns_in_push_order:
        ring[head] = r
        head = (head + 1) % RING
        count = min(count + 1, RING)
    return ring, head, count
