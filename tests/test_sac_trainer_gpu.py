"""SACTrainer (oc_cleanrl_amd/sac.py) on the MI355X: three train steps against the float64 twin of
tests/sac_util.py, eager against hipGraph chunks, the target update, the pixel networks' fused
forward and the command line."""
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

import sac_util as su
from conftest import ROOT

pytestmark = pytest.mark.gpu

KEYS = ("losses/qf1_values", "losses/qf2_values", "losses/qf1_loss", "losses/qf2_loss",
        "losses/qf_loss", "losses/actor_loss", "losses/alpha", "losses/alpha_loss")


def sac_args(**kw):
    from oc_cleanrl_amd.sac import SACArgs

    base = dict(backend="Synthetic", obs_mode="obj", num_envs=1, encoder_dims=(32,),
                decoder_dims=(32,), batch_size=8, buffer_size=64, learning_starts=8,
                update_frequency=4, target_network_frequency=8, save_model=False)
    base.update(kw)
    return SACArgs(**base)


def make(dev, **kw):
    from oc_cleanrl_amd.sac import SACTrainer

    return SACTrainer(sac_args(**kw), dev, log=False)


def fixed_batches(tr, n: int):
    g = torch.Generator().manual_seed(99)
    B, out = tr.args.batch_size, []
    for _ in range(n):
        d = {"observations": torch.randn((B,) + tr.obs_shape, generator=g),
             "next_observations": torch.randn((B,) + tr.obs_shape, generator=g),
             "actions": torch.randint(0, tr.A, (B, 1), generator=g),
             "rewards": torch.sign(torch.randn(B, 1, generator=g)),
             "dones": (torch.rand(B, 1, generator=g) < 0.25).float()}
        out.append(d)
    return out


def t64(v: float):
    return torch.tensor(v, dtype=torch.float64)


def test_three_updates_match_the_twin(dev):
    """The same three batches through update() and through the script's train step restated on
    f64 / f32 CPU copies: the second and third step see the Adam states and the carried alpha, and
    each actor loss sees the critics after that step's critic update."""
    tr = make(dev, cuda_graphs=False)
    assert tr.opt.eps == tr.actor_opt.eps == 1e-4 and tr.temp.eps == 1e-4
    assert tr.temp.target_entropy == float(-0.89 * torch.log(1 / torch.tensor(tr.A)))
    sds = [{k: v.detach().clone().cpu() for k, v in m.state_dict().items()}
           for m in (tr.actor, tr.q.qf1, tr.q.qf2)]
    batches = fixed_batches(tr, 3)

    def reference(dt):
        gamma = 0.99 if dt == torch.float32 else float(np.float32(0.99))
        ref = su.SACRef(*sds, dt, gamma, tr.args.q_lr, tr.args.policy_lr, tr.temp.target_entropy)
        return ref, [ref.update(d) for d in batches]

    twin, m64 = reference(torch.float64)
    f32, m32 = reference(torch.float32)
    ck = su.Checks()
    for i, d in enumerate(batches):
        tr.update({k: v.to(dev) for k, v in d.items()})
        m = tr.metrics()
        assert set(KEYS) <= set(m)
        for k in KEYS:
            ck.check(f"step {i + 1} {k}", t64(m[k]), t64(m32[i][k]), t64(m64[i][k]))
    ck.check("alpha", tr.temp.alpha, t64(f32.alpha), t64(twin.alpha))
    for name, net, r32, r64 in (("actor", tr.actor, f32.actor, twin.actor),
                                ("qf1", tr.q.qf1, f32.qf1, twin.qf1),
                                ("qf2", tr.q.qf2, f32.qf2, twin.qf2)):
        for k, v in net.state_dict().items():
            ck.check(f"{name} {k}", v, r32[k].detach(), r64[k].detach())
    assert tr.temp.step.item() == 3 and tr.temp.alpha.item() != 1.0
    ck.done()


def state_of(tr):
    return [tr.opt.params, tr.actor_opt.params, tr.t_flat, tr.temp.alpha, tr.temp.log_alpha,
            tr.rb.state, tr.rb.obs, tr.rb.actions, tr.rb.rewards, tr.rb.dones, tr.q_stats,
            tr.pi_stats]


def test_eager_and_graph_chunks_are_bit_identical(dev):
    a, b = make(dev, cuda_graphs=False), make(dev, cuda_graphs=True)
    a.steps(24)
    b.steps(24)
    torch.cuda.synchronize()
    assert b.graphs and not a.graphs
    for x, y in zip(state_of(a), state_of(b)):
        assert torch.equal(x, y)
    assert a.temp.step.item() == 4  # train steps at 12, 16, 20, 24
    # both acting phases ran: the replay holds actions of the random and of the sampling phase
    assert a.rb.state[0].item() == 24


@pytest.mark.parametrize("tau", [1.0, 0.5])
def test_target_update(dev, tau):
    tr = make(dev, tau=tau, cuda_graphs=False)
    t0 = tr.t_flat.clone()
    assert torch.equal(t0, tr.opt.params)
    tr.steps(12)  # one train step at 12, no target update since the one due at 8 (not learning yet)
    assert torch.equal(tr.t_flat, t0) and not torch.equal(tr.opt.params, t0)
    tr.steps(4)   # train step at 16, then the target update
    torch.cuda.synchronize()
    want = tau * tr.opt.params + (1.0 - tau) * t0
    assert torch.equal(tr.t_flat, want)
    if tau == 1.0:
        for t, p in zip(tr.target.parameters(), tr.q.parameters()):
            assert torch.equal(t, p)
    else:
        assert not torch.equal(tr.t_flat, tr.opt.params)
    for p in tr.target.parameters():
        assert not p.requires_grad


def test_pixel_networks_fused_forward(dev):
    from oc_cleanrl_amd.sac import Actor, SoftQNetwork

    torch.manual_seed(5)
    x = torch.randint(0, 256, (2, 4, 84, 84)).float()
    for cls, fused in ((Actor, "logits"), (SoftQNetwork, "q_values")):
        net = cls((4, 84, 84), 6)
        ref = lambda dt: (net.to(dt)(x.to(dt) / 255.0) if cls is Actor  # noqa: E731
                          else net.to(dt)(x.to(dt))).detach()
        twin = ref(torch.float64)
        f32 = ref(torch.float32)
        g = net.to(torch.float32).to(dev)
        with torch.no_grad():
            got = getattr(g, fused)(x.to(dev))
        assert got.shape == (2, 6)
        su.check(f"{cls.__name__}.{fused}", got, f32, twin)


def test_command_line_writes_metrics(tmp_path):
    cmd = [sys.executable, "-m", "oc_cleanrl_amd.sac", "--backend", "Synthetic", "--obs-mode",
           "obj", "--total-timesteps", "64", "--learning-starts", "16", "--buffer-size", "64",
           "--log-dir", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    run = next(tmp_path.iterdir())
    lines = [json.loads(s) for s in (run / "metrics.jsonl").read_text().splitlines()]
    assert lines and lines[-1]["global_step"] == 64
    last = lines[-1]
    assert set(KEYS) <= set(last)
    assert all(np.isfinite(last[k]) for k in KEYS)
    assert last["losses/qf_loss"] == pytest.approx(
        (last["losses/qf1_loss"] + last["losses/qf2_loss"]) / 2)
    ck = torch.load(run / "sac_atari.cleanrl_model", weights_only=True)
    assert set(ck) == {"actor_weights", "qf1_weights", "qf2_weights", "args"}
    assert ck["args"]["learning_starts"] == 16
