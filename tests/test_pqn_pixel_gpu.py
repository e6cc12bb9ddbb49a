"""The pixel PQN networks (pqn_atari_envpool.py / _lstm.py: Conv -> LayerNorm([C, H, W]) -> ReLU
three times) with their wide LayerNorms on ops.ln_chw_relu, in the rollout and -- under
pqn.FUSED_LN_CHW_UPDATE -- with autograd: against the float64 twin of the same state dict by the
DESIGN 11 rule (pqn_util.check), the torch path (FUSED_PQN = False) being the f32 computation."""
from __future__ import annotations

import copy

import pytest
import torch

import pqn_util as U

pytestmark = pytest.mark.gpu

B, A = 3, 6


def _make(kind, dev):
    from oc_cleanrl_amd import pqn, pqn_lstm
    from oc_cleanrl_amd.agents import EnvSpec

    torch.manual_seed(5)
    if kind == "PQN":
        return pqn.PQNetwork(EnvSpec((4, 84, 84), A), "PQN").to(dev)
    return pqn_lstm.PQNLSTMNetwork(EnvSpec((1, 84, 84), A), "PQN_LSTM").to(dev)


def _q_and_grads(net, x, dq, fused: bool, update: bool = True):
    """Q values and every parameter's gradient of sum(q * dq)."""
    from oc_cleanrl_amd import pqn

    old = pqn.FUSED_PQN, pqn.FUSED_LN_CHW_UPDATE
    pqn.FUSED_PQN, pqn.FUSED_LN_CHW_UPDATE = fused, update
    try:
        net.zero_grad()
        if hasattr(net, "lstm"):
            z = torch.zeros(1, B, net.lstm.hidden_size, dtype=x.dtype, device=x.device)
            q, _ = net(x, (z, z.clone()), torch.zeros(B, dtype=x.dtype, device=x.device))
        else:
            q = net(x)
        (q * dq).sum().backward()
        out = {"q": q.detach()}
        out.update({k: p.grad.clone() for k, p in net.named_parameters()})
        return out
    finally:
        pqn.FUSED_PQN, pqn.FUSED_LN_CHW_UPDATE = old


@pytest.mark.parametrize("kind", ["PQN", "PQN_LSTM"])
def test_network_against_the_f64_twin(dev, kind):
    from oc_cleanrl_amd import ops

    net = _make(kind, dev)
    g = torch.Generator().manual_seed(11)
    x = torch.randint(0, 256, (B,) + ((4,) if kind == "PQN" else (1,)) + (84, 84),
                      generator=g).float()
    dq = torch.randn(B, A, generator=g)
    # the script's three LayerNorms are inside the kernel's contract, in either memory format
    h = x.to(dev) / 255.0
    norms = 0
    for m in net.network:
        if isinstance(m, torch.nn.LayerNorm) and len(m.normalized_shape) == 3:
            assert ops.ln_chw_ok(h, m)
            assert ops.ln_chw_ok(h.contiguous(memory_format=torch.channels_last), m)
            norms += 1
        h = m(h)
    assert norms == 3
    twin_net = copy.deepcopy(net).cpu().double()
    twin = _q_and_grads(twin_net, x.double(), dq.double(), fused=False)
    f32 = _q_and_grads(net, x.to(dev), dq.to(dev), fused=False)
    got = _q_and_grads(net, x.to(dev), dq.to(dev), fused=True)
    for k in twin:
        U.check(f"{kind} {k}", got[k], f32[k], twin[k])
    # the rollout's route (no autograd), where the Flatten may meet either memory format
    from oc_cleanrl_amd import pqn

    with torch.no_grad():
        hid = net.trunk(x.to(dev).contiguous(memory_format=torch.channels_last))
        hid64 = twin_net.trunk(x.double())
        old, pqn.FUSED_PQN = pqn.FUSED_PQN, False
        try:
            hid32 = net.trunk(x.to(dev))
        finally:
            pqn.FUSED_PQN = old
    U.check(f"{kind} trunk (rollout route)", hid, hid32, hid64)


def test_pixel_trainer_iteration_is_deterministic(dev):
    from oc_cleanrl_amd import pqn

    def run():
        args = pqn.finalize(pqn.PQNArgs(architecture="PQN", obs_mode="dqn", num_envs=2,
                                        num_steps=4, num_minibatches=2, update_epochs=1,
                                        total_timesteps=8, save_model=False, seed=3))
        tr = pqn.PQNTrainer(args, dev, log=False)
        tr.train_iteration()
        torch.cuda.synchronize()
        return tr.optimizer.params.detach().cpu().clone()

    old, pqn.FUSED_LN_CHW_UPDATE = pqn.FUSED_LN_CHW_UPDATE, True
    try:
        first, second = run(), run()
    finally:
        pqn.FUSED_LN_CHW_UPDATE = old
    assert bool(torch.isfinite(first).all()) and torch.equal(first, second)
