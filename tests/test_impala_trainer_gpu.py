"""QDaggerTrainer with the script's IMPALA student on the fused units: one loss step against the
same networks run as plain modules under autograd (f32 on the device, f64 twin on the CPU), and a
short run of all three phases with hipGraphs on, twice, bitwise equal."""
from __future__ import annotations

import copy
import json

import pytest
import torch

import impala_util as U
import qdagger_util as qu
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CFG = dict(obs_mode="dqn", student_network="impala", env_id="ALE/Pong-v5", num_envs=2,
           buffer_size=64, batch_size=8, teacher_steps=8, offline_steps=8, total_timesteps=16,
           learning_starts=0, train_frequency=4, target_network_frequency=8, teacher_return=5.0)
OBS, A = (4, 84, 84), 6


@pytest.fixture(scope="module")
def teacher_file(tmp_path_factory):
    from oc_cleanrl_amd.dqn import QNetwork

    torch.manual_seed(3)
    path = tmp_path_factory.mktemp("teacher") / "pixel_teacher.pt"
    torch.save(QNetwork(OBS, A).state_dict(), path)
    return str(path)


def make(teacher_file, **kw):
    from oc_cleanrl_amd.qdagger import QDaggerArgs, QDaggerTrainer

    return QDaggerTrainer(QDaggerArgs(**{**CFG, "teacher_model_path": teacher_file, **kw}), DEV)


def test_loss_step_against_plain_modules(teacher_file):
    from oc_cleanrl_amd.qdagger import QNetworkImpala

    tr = make(teacher_file, cuda_graphs=False)
    assert isinstance(tr.q, QNetworkImpala) and isinstance(tr.target, QNetworkImpala)
    a, B = tr.args, CFG["batch_size"]
    gen = torch.Generator().manual_seed(7)
    d = {"observations": torch.randint(0, 256, (B,) + OBS, generator=gen).float(),
         "next_observations": torch.randint(0, 256, (B,) + OBS, generator=gen).float(),
         "actions": torch.randint(0, A, (B, 1), generator=gen),
         "rewards": torch.randn((B, 1), generator=gen),
         "dones": (torch.rand((B, 1), generator=gen) < 0.25).float()}
    want = {}
    for dtype, dev in ((torch.float32, DEV), (torch.float64, "cpu")):
        q, target, teacher = (copy.deepcopy(m).to(dev, dtype) for m in (tr.q, tr.target, tr.teacher))
        c = {k: v.to(dev, dtype) if v.is_floating_point() else v.to(dev) for k, v in d.items()}
        for p in q.parameters():
            p.requires_grad_(True)
            p.grad = None
        with torch.no_grad():
            q_next, q_t = target(c["next_observations"]), teacher(c["observations"])
        terms = qu.loss_terms(q(c["observations"]), q_next, q_t, c["actions"].reshape(-1),
                              c["rewards"].reshape(-1), c["dones"].reshape(-1), a.gamma,
                              a.temperature, 1.0)
        terms[0].backward()
        want[dtype] = (torch.stack(terms[:3]).detach(), [p.grad for p in q.parameters()])
    stats = torch.zeros(5, device=DEV)
    tr._loss_step({k: v.to(DEV) for k, v in d.items()}, None, stats)
    torch.cuda.synchronize()
    U.check("loss, q_loss, distill", stats[:3], want[torch.float32][0], want[torch.float64][0])
    for (n, p), g32, g64 in zip(tr.q.named_parameters(), want[torch.float32][1],
                                want[torch.float64][1]):
        U.check(n, p.grad, g32, g64)


def run_all(teacher_file):
    tr = make(teacher_file, cuda_graphs=True)
    before = tr.opt.params.clone()
    tr.run_teacher_fill()
    tr.run_offline()
    tr.steps(CFG["total_timesteps"])
    torch.cuda.synchronize()
    return tr, before


def test_three_phases_with_graphs_twice_bitwise(teacher_file):
    tr, before = run_all(teacher_file)
    assert tr.graphs and tr.train_steps == CFG["total_timesteps"] // CFG["train_frequency"]
    assert tr.offline_step == CFG["offline_steps"] and tr.phase == "online"
    assert bool(torch.isfinite(tr.opt.params).all()) and not torch.equal(tr.opt.params, before)
    assert bool(torch.isfinite(tr.td_stats).all()) and bool(torch.isfinite(tr.offline_stats).all())
    keys = json.loads((ROOT / "tests" / "golden" / "qdagger_state_keys.json").read_text())
    ck = tr.checkpoint()["model_weights"]
    assert {k: list(v.shape) for k, v in ck.items()} == keys
    again, _ = run_all(teacher_file)
    assert torch.equal(tr.opt.params, again.opt.params)
    assert torch.equal(tr.td_stats, again.td_stats)
    assert torch.equal(tr.offline_stats, again.offline_stats)
