"""The masked LSTM recurrence of cleanrl/ppo_atari_lstm.py:140-158 and the agent around it,
restated in plain torch ops on a dict of parameters. Dtype-generic: run on float64 copies of f32
inputs and weights it is the float64 twin for shapes the fixtures do not cover
(tests/test_lstm_cpu.py checks it against them); run in float32 it is "the f32 torch loop" whose
own error sets the bound.

The error rule of DESIGN.md 11: a tensor's error against the f64 twin, relative to the twin's
largest element, is at most max(3 x the f32 torch computation's own error, 4 * 2^-23).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

FLOOR = 4 * 2.0 ** -23
# fixtures hold tensors of more than FULL_MAX elements as (shape, float64 sum, the elements at
# pick_indices): the committed-file size limit
FULL_MAX, PICKS = 40000, 4096


def pick_indices(size: int):
    import numpy as np

    return np.linspace(0, size - 1, PICKS).astype(np.int64)


def packed(fx: dict, key: str, arr):
    """(fixture values, the matching view of `arr`) for a tensor the fixture holds whole or as a
    sample; also checks the shape and, for a sample, returns the float64 sums as a third/fourth
    value (None for whole tensors)."""
    import numpy as np

    arr = np.asarray(arr)
    if key in fx:
        assert fx[key].shape == arr.shape, key
        return fx[key], arr, None, None
    assert tuple(fx[key + "::shape"]) == arr.shape, key
    return (fx[key + "::pick"], arr.reshape(-1)[pick_indices(arr.size)],
            float(fx[key + "::sum"]), float(arr.astype(np.float64).sum()))


def rel_err(a, twin) -> float:
    """max |a - twin| / max |twin| (in float64)."""
    a, twin = torch.as_tensor(a).double().cpu(), torch.as_tensor(twin).double().cpu()
    m = float(twin.abs().max())
    return float((a - twin).abs().max()) / (m if m > 0 else 1.0)


def bound(own: float) -> float:
    return max(3 * own, FLOOR)


def check(name, got, f32, twin):
    """Assert the rule for one tensor; prints the (measured, torch's-own) pair first."""
    e, own = rel_err(got, twin), rel_err(f32, twin)
    print(f"{name}: {e:.3g} / {own:.3g}")
    assert e <= bound(own), (name, e, own)
    return e, own


def lstm_cell(x, h, c, w_ih, b_ih, w_hh, b_hh):
    """nn.LSTM's cell, gate order i | f | g | o."""
    z = (x @ w_ih.t() + b_ih) + (h @ w_hh.t() + b_hh)
    i, f, g, o = z.chunk(4, dim=-1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def lstm_seq_ref(x, w_ih, b_ih, w_hh, b_hh, done, h0, c0):
    """x [T, B, I], done [T, B], h0 / c0 [B, H] -> (h_out [T, B, H], hT, cT): the state entering
    step t is multiplied by 1 - done[t] (:152-153)."""
    h, c = h0, c0
    out = []
    for t in range(x.shape[0]):
        m = (1.0 - done[t]).unsqueeze(-1)
        h, c = lstm_cell(x[t], m * h, m * c, w_ih, b_ih, w_hh, b_hh)
        out.append(h)
    return torch.stack(out), h, c


def seq_case(T, B, I, H, done, h0, c0, x, w_ih, b_ih, w_hh, b_hh, g, dtype):
    """Forward + every gradient of loss = sum(h_out * g) on `dtype` copies: a dict of h_out, hT,
    cT, dx, dw_ih, db_ih, dw_hh, db_hh (and dpre = the gradient at x W_ih^T + b_ih)."""
    cast = lambda t: t.detach().cpu().to(dtype)  # noqa: E731
    x, w_ih, b_ih, w_hh, b_hh = (cast(t).requires_grad_() for t in (x, w_ih, b_ih, w_hh, b_hh))
    pre = (x @ w_ih.t() + b_ih)
    pre.retain_grad()
    zero_b = torch.zeros_like(b_ih)
    eye = torch.eye(4 * H, dtype=dtype)
    h_out, hT, cT = lstm_seq_ref(pre, eye, zero_b, w_hh, b_hh, cast(done), cast(h0), cast(c0))
    (h_out * cast(g)).sum().backward()
    return dict(h_out=h_out.detach(), hT=hT.detach(), cT=cT.detach(), dpre=pre.grad, dx=x.grad,
                dw_ih=w_ih.grad, db_ih=b_ih.grad, dw_hh=w_hh.grad, db_hh=b_hh.grad)


def trunk(p, x, pixels: bool):
    """The reference network (:120-130) or a PPObj Linear/ReLU stack, from the state dict p."""
    if pixels:
        h = x / 255.0
        h = F.relu(F.conv2d(h, p["network.0.weight"], p["network.0.bias"], stride=4))
        h = F.relu(F.conv2d(h, p["network.2.weight"], p["network.2.bias"], stride=2))
        h = F.relu(F.conv2d(h, p["network.4.weight"], p["network.4.bias"], stride=1))
        return F.relu(h.flatten(1) @ p["network.7.weight"].t() + p["network.7.bias"])
    idx = sorted({int(k.split(".")[1]) for k in p if k.startswith("network.")})
    shapes = [p[f"network.{i}.weight"].shape for i in idx]
    h = x
    for n, i in enumerate(idx):
        if n and shapes[n][1] != shapes[n - 1][0]:  # the Flatten between encoder and decoder
            h = h.flatten(1)
        h = F.relu(h @ p[f"network.{i}.weight"].t() + p[f"network.{i}.bias"])
    return h


def agent_ref(p, x, done, h0, c0, pixels: bool):
    """Agent.get_states + heads on the state dict p: (new_hidden [T * B, H], hT, cT, logits,
    value). x [T * B, ...] time-major, h0 / c0 [B, H]."""
    B = h0.shape[0]
    hid = trunk(p, x, pixels)
    T = hid.shape[0] // B
    out, hT, cT = lstm_seq_ref(hid.view(T, B, -1), p["lstm.weight_ih_l0"], p["lstm.bias_ih_l0"],
                               p["lstm.weight_hh_l0"], p["lstm.bias_hh_l0"], done.view(T, B), h0,
                               c0)
    out = out.reshape(T * B, -1)
    logits = out @ p["actor.weight"].t() + p["actor.bias"]
    value = out @ p["critic.weight"].t() + p["critic.bias"]
    return out, hT, cT, logits, value
