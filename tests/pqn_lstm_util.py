"""The recurrent PQN network and targets of cleanrl/pqn_atari_envpool_lstm.py restated in plain
torch ops on a state dict (keys network.*, lstm.*, q_func.*). Dtype-generic: on float64 copies it
is the float64 twin, in float32 "the f32 torch computation" whose own error sets the bound
(lstm_util.check: the rule of DESIGN.md 11).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from lstm_util import FLOOR, bound, check, lstm_cell, rel_err  # noqa: F401  (the rule, shared)
from pqn_util import RAdamRef, clip_coef, q_lambda_ref  # noqa: F401  (:283-296 is PQN's loop)


def trunk_ref(p: dict, x, pixels: bool):
    """network.* of the state dict p on x: the pixel stack of :120-134 (x / 255 first, :144), or
    the object-vector Linear -> LayerNorm -> ReLU stack (a 1-D weight is a LayerNorm; the Flatten
    sits where a Linear's input width changes)."""
    idx = sorted({int(k.split(".")[1]) for k in p if k.startswith("network.")})
    h = x / 255.0 if pixels else x
    for i in idx:
        w, b = p[f"network.{i}.weight"], p[f"network.{i}.bias"]
        if w.dim() == 4:
            stride = {8: 4, 4: 2, 3: 1}[w.shape[-1]]
            h = F.conv2d(h, w, b, stride=stride)
        elif w.dim() == 2:
            if h.shape[-1] != w.shape[1]:
                h = h.flatten(1)
            h = h @ w.t() + b
        else:  # LayerNorm over the weight's shape, then the ReLU that follows every one
            h = F.relu(F.layer_norm(h, tuple(w.shape), w, b, 1e-5))
    return h


def forward_ref(p: dict, x, lstm_state, done, pixels: bool = False):
    """QNetwork.forward (:143-165) as a plain loop: x [T * B, ...] time-major, lstm_state
    (h, c) [1, B, H], done [T * B] -> (q [T * B, A], new_hidden [T * B, H], (h, c) [1, B, H]).
    The state entering a step is multiplied by 1 - done of that step."""
    h, c = lstm_state[0][0], lstm_state[1][0]
    B = h.shape[0]
    hid = trunk_ref(p, x, pixels)
    hid = hid.reshape(-1, B, hid.shape[-1])
    done = done.reshape(-1, B)
    out = []
    for xt, d in zip(hid, done):
        m = (1.0 - d).unsqueeze(-1)
        h, c = lstm_cell(xt, m * h, m * c, p["lstm.weight_ih_l0"], p["lstm.bias_ih_l0"],
                         p["lstm.weight_hh_l0"], p["lstm.bias_hh_l0"])
        out.append(h)
    new_hidden = torch.cat(out)
    q = new_hidden @ p["q_func.weight"].t() + p["q_func.bias"]
    return q, new_hidden, (h.unsqueeze(0), c.unsqueeze(0))


def head_loss_ref(h, wq, bq, actions, returns, dtype):
    """The update's head and loss (:318-325) on `dtype` CPU copies, through autograd: Linear ->
    one-hot masked sum -> F.mse_loss. A dict of q_a, loss, q_mean, dh, dwq, dbq."""
    cast = lambda t: t.detach().cpu().to(dtype)  # noqa: E731
    h, wq, bq = (cast(t).requires_grad_() for t in (h, wq, bq))
    a = actions.detach().cpu().long().clamp(0, wq.shape[0] - 1)
    q = F.linear(h, wq, bq)
    q_a = (q * F.one_hot(a, wq.shape[0]).to(dtype)).sum(1)
    loss = F.mse_loss(cast(returns), q_a)
    loss.backward()
    return dict(q_a=q_a.detach(), loss=loss.detach(), q_mean=q_a.detach().mean(), dh=h.grad,
                dwq=wq.grad, dbq=bq.grad)
