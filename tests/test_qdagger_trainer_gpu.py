"""QDaggerTrainer on the GPU at one small configuration: the two teacher file forms, the teacher
fill's actions, the offline phase against a plain-torch restatement, the online phase's step
bookkeeping and ring, graph replay against the eager path, and the metric / checkpoint surface."""
import copy

import numpy as np
import pytest
import torch

import lstm_util as lu
import qdagger_util as qu

pytestmark = pytest.mark.gpu

DEV = "cuda"
CFG = dict(obs_mode="obj", env_id="ALE/Pong-v5", num_envs=1, num_features=12, buffer_window_size=4,
           encoder_dims=(32,), decoder_dims=(256,), buffer_size=64, batch_size=8,
           teacher_steps=16, offline_steps=8, total_timesteps=32, learning_starts=0,
           train_frequency=4, target_network_frequency=8, teacher_return=5.0)
OBS, A = (4, 12), 6


@pytest.fixture(scope="module")
def teacher_files(tmp_path_factory):
    from oc_cleanrl_amd.dqn import QNetworkObj

    d = tmp_path_factory.mktemp("teacher")
    torch.manual_seed(3)
    net = QNetworkObj(OBS, A, (32,), (256,))
    torch.save(net.state_dict(), d / "bare.pt")
    torch.save({"model_weights": net.state_dict(),
                "args": {"encoder_dims": (32,), "decoder_dims": (256,)}}, d / "dqn.cleanrl_model")
    torch.manual_seed(3)
    torch.save(QNetworkObj(OBS, 18, (32,), (256,)).state_dict(), d / "a18.pt")
    return d


def make(teacher_files, form="dqn.cleanrl_model", **kw):
    from oc_cleanrl_amd.qdagger import QDaggerArgs, QDaggerTrainer

    return QDaggerTrainer(QDaggerArgs(**{**CFG, "teacher_model_path": str(teacher_files / form),
                                         **kw}), DEV)


def run_all(teacher_files, graphs: bool):
    tr = make(teacher_files, cuda_graphs=graphs)
    tr.step_record = []
    tr.run_teacher_fill()
    tr.run_offline()
    tr.steps(CFG["total_timesteps"])
    torch.cuda.synchronize()
    return tr


@pytest.fixture(scope="module")
def eager(teacher_files):
    return run_all(teacher_files, False)


def test_teacher_file_forms(teacher_files):
    a, b = make(teacher_files, "dqn.cleanrl_model"), make(teacher_files, "bare.pt")
    assert a.teacher_flat.numel() > 0 and torch.equal(a.teacher_flat, b.teacher_flat)
    assert not a.teacher.training and not any(p.requires_grad for p in a.teacher.parameters())
    assert all(p.data_ptr() >= a.teacher_flat.data_ptr() for p in a.teacher.parameters())
    with pytest.raises(ValueError, match="18 actions"):
        make(teacher_files, "a18.pt")


def test_teacher_fill_records_the_teachers_actions(teacher_files):
    from oc_cleanrl_amd import ops

    tr = make(teacher_files)
    student = tr.opt.params.clone()
    tr.run_teacher_fill()
    rb, a = tr.teacher_rb, tr.args
    assert rb.state.tolist() == [16, 0] and tr.rb is None and tr.phase == "offline"
    assert torch.equal(tr.opt.params, student)  # nothing trained
    eps = []
    for i in range(16):
        obs = rb.obs[i].float()  # [E, W, F]
        with torch.no_grad():
            q = tr.teacher.q_values(obs)
        step = torch.tensor([i], dtype=torch.int64, device=DEV)
        e = torch.zeros(1, device=DEV)
        act = ops.epsilon_greedy(q, a.seed, step, a.start_e, a.end_e, float(a.teacher_steps),
                                 epsilon_out=e)
        assert act.tolist() == rb.actions[i].tolist(), i
        eps.append(float(e))
    from oc_cleanrl_amd.qdagger import linear_schedule

    want = [linear_schedule(a.start_e, a.end_e, a.teacher_steps, i) for i in range(16)]
    assert np.allclose(eps, want, rtol=1e-6)


def restate(models, batch, gamma, T, dtype):
    """One train step of the script in plain torch on `batch` (a dict of f32 tensors)."""
    q, target, teacher, opt = models
    c = lambda x: x.to(dtype) if x.is_floating_point() else x  # noqa: E731
    d = {k: c(v) for k, v in batch.items()}
    with torch.no_grad():
        q_next, q_t = target(d["next_observations"]), teacher(d["observations"])
    loss = qu.loss_terms(q(d["observations"]), q_next, q_t, d["actions"].reshape(-1),
                         d["rewards"].reshape(-1), d["dones"].reshape(-1), gamma, T, 1.0)[0]
    opt.zero_grad()
    loss.backward()
    opt.step()


def flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


def test_offline_phase_against_plain_torch(teacher_files):
    tr = make(teacher_files, cuda_graphs=False)
    tr.run_teacher_fill()
    a = tr.args
    twins = {}
    for dtype in (torch.float32, torch.float64):
        q = copy.deepcopy(tr.q).to(dtype)
        for p in q.parameters():
            p.requires_grad_(True)
        twins[dtype] = [q, copy.deepcopy(tr.target).to(dtype), copy.deepcopy(tr.teacher).to(dtype),
                        torch.optim.Adam(q.parameters(), lr=a.learning_rate)]
    changed = []
    for step in range(a.offline_steps):
        before = tr.t_flat.clone()
        tr.run_offline(1)
        changed.append(not torch.equal(before, tr.t_flat))
        if step >= 4:
            continue
        batch = {k: v.clone() for k, v in tr.batch.items()}
        for dtype, m in twins.items():
            restate(m, batch, a.gamma, a.temperature, dtype)
            if step % a.target_network_frequency == 0:
                m[1].load_state_dict(m[0].state_dict())
        lu.check(f"offline step {step}", flat(tr.q), flat(twins[torch.float32][0]),
                 flat(twins[torch.float64][0]))
    # step 0 is a multiple of target_network_frequency (the script updates there); steps 1-7 are
    # not, and step 8 would be the next
    assert changed == [True] + [False] * 7
    assert tr.offline_step == 8
    with pytest.raises(ValueError, match="0 offline steps remain"):
        tr.run_offline(1)
    m = tr.metrics()
    assert {"charts/offline/loss", "charts/offline/q_loss", "charts/offline/distill_loss",
            "charts/teacher/avg_episodic_return"} <= set(m)
    assert m["charts/offline/loss"] == pytest.approx(
        m["charts/offline/q_loss"] + m["charts/offline/distill_loss"], rel=1e-5)


def test_online_bookkeeping_and_ring(eager):
    a = eager.args
    # :367-446 with the offset, the step counted as DQNTrainer counts it (the count after the step)
    trains, updates, first = 0, 0, None
    for i in range(a.total_timesteps):
        gs = i + 1 + a.offline_steps
        if gs > a.learning_starts:
            if gs % a.train_frequency == 0:
                trains += 1
                first = first or i + 1
            if gs % a.target_network_frequency == 0:
                updates += 1
    assert (trains, updates, first) == (8, 4, 4)
    assert (eager.train_steps, eager.target_updates, eager.first_train_step) == (trains, updates,
                                                                                first)
    assert eager.global_step == 32 and eager.teacher_rb is None
    assert eager.rb.state.tolist() == [32, 0]
    assert int(eager.step_dev) == a.offline_steps + 32
    assert len(eager.step_record) == 32
    *_, (returns, run, coeff) = qu.episode_ring_ref(eager.step_record, 1, a.teacher_return)
    assert eager.ring.returns() == returns
    assert eager.ring.run_ret.cpu().numpy().tobytes() == run.tobytes()
    assert eager.ring.coeff.cpu().numpy().tobytes() == np.float32(coeff).tobytes()
    assert float(eager.td_stats[4]) == float(coeff)


def test_graph_replay_is_bitwise_the_eager_run(eager, teacher_files):
    g = run_all(teacher_files, True)
    assert g._graphable() and set(g.graphs) == {"train"}
    bits = lambda x: x.contiguous().view(torch.int32)  # noqa: E731
    for name in ("opt.params", "t_flat", "ring.ring", "ring.run_ret", "ring.coeff", "td_stats",
                 "offline_stats"):
        x, y = eager, g
        for part in name.split("."):
            x, y = getattr(x, part), getattr(y, part)
        assert torch.equal(bits(x), bits(y)), name
    assert torch.equal(eager.ring.state, g.ring.state)
    assert (g.train_steps, g.target_updates, g.first_train_step) == (8, 4, 4)


def test_metrics_and_checkpoint(eager):
    from oc_cleanrl_amd.dqn import DQNArgs, make_qnet

    m = eager.metrics()
    assert {"losses/loss", "losses/td_loss", "losses/distill_loss", "losses/q_values",
            "charts/distill_coeff", "charts/epsilon", "charts/teacher/avg_episodic_return",
            "charts/offline/loss", "charts/offline/q_loss", "charts/offline/distill_loss"} <= set(m)
    assert m["charts/teacher/avg_episodic_return"] == 5.0
    assert all(np.isfinite(v) for v in m.values())
    assert m["losses/loss"] == pytest.approx(
        m["losses/td_loss"] + m["charts/distill_coeff"] * m["losses/distill_loss"], rel=1e-5)
    ck = eager.checkpoint()
    net = make_qnet(DQNArgs(obs_mode="obj", encoder_dims=tuple(ck["args"]["encoder_dims"]),
                            decoder_dims=tuple(ck["args"]["decoder_dims"])), OBS, A)
    net.load_state_dict(ck["model_weights"])
    assert torch.equal(flat(net), flat(eager.q).cpu())
