"""QDagger, host side: the args surface and the IMPALA student's keys against fixtures taken from
the reference script, the trainer's refusals, the float64 twin against the script's own loss
lines (fixtures), the episodic-return ring's restatement on hand-written sequences, and the new
ABI functions' argument checks (no launch)."""
import ctypes
import dataclasses
import json

import numpy as np
import pytest
import torch

import lstm_util as lu
import qdagger_util as qu
from conftest import ROOT

GOLDEN = ROOT / "tests" / "golden"
ADDITIONS = {"obs_mode", "buffer_window_size", "backend", "num_features", "obs_storage",
             "encoder_dims", "decoder_dims", "cuda_graphs", "gemm_table", "vecnorm_reward",
             "log_dir", "log_every", "teacher_model_path", "teacher_return", "student_network"}


def test_args_match_the_scripts_fields():
    from oc_cleanrl_amd.qdagger import QDaggerArgs

    want = json.loads((GOLDEN / "qdagger_args_fields.json").read_text())
    a = QDaggerArgs()
    names = [f.name for f in dataclasses.fields(QDaggerArgs)]
    assert names[:len(want)] == list(want)  # the script's fields, in its order
    for k, v in want.items():
        assert getattr(a, k) == v, k
        assert v is None or type(getattr(a, k)) is type(v), k
    assert set(names) - set(want) == ADDITIONS
    assert (a.backend, a.teacher_model_path, a.teacher_return, a.student_network,
            a.vecnorm_reward) == ("Synthetic", "", None, "auto", False)


def test_cli_parses_the_scripts_flag_spellings():
    from oc_cleanrl_amd.args import parse_dataclass
    from oc_cleanrl_amd.qdagger import QDaggerArgs

    a = parse_dataclass(QDaggerArgs, ["--obs-mode", "obj", "--teacher-model-path", "t.pt",
                                      "--teacher-steps", "16", "--offline-steps", "8",
                                      "--temperature", "0.5", "--teacher-return", "5.0"])
    assert (a.obs_mode, a.teacher_model_path, a.teacher_steps, a.offline_steps, a.temperature,
            a.teacher_return) == ("obj", "t.pt", 16, 8, 0.5, 5.0)


def test_impala_student_keys_and_shapes():
    from oc_cleanrl_amd.qdagger import QNetworkImpala

    want = json.loads((GOLDEN / "qdagger_state_keys.json").read_text())
    net = QNetworkImpala((4, 84, 84), 6)
    got = {k: list(v.shape) for k, v in net.state_dict().items()}
    assert list(got) == list(want) and got == want
    assert net(torch.zeros(2, 4, 84, 84)).shape == (2, 6)
    # the script's default init, not PPG's normed one: biases are not zeroed
    assert float(net.network[0].conv.bias.detach().abs().max()) > 0


def _teacher_file(tmp_path, n_actions=6):
    from oc_cleanrl_amd.dqn import QNetworkObj

    torch.manual_seed(3)
    path = tmp_path / f"teacher_{n_actions}.pt"
    torch.save(QNetworkObj((4, 12), n_actions, (32,), (256,)).state_dict(), path)
    return str(path)


def _args(**kw):
    from oc_cleanrl_amd.qdagger import QDaggerArgs

    base = dict(obs_mode="obj", env_id="ALE/Pong-v5", encoder_dims=(32,), decoder_dims=(256,))
    return QDaggerArgs(**{**base, **kw})


def test_trainer_refusals_come_before_any_device_work(tmp_path):
    """None of these reaches DQNTrainer.__init__ (which would need a GPU)."""
    from oc_cleanrl_amd.qdagger import QDaggerTrainer

    with pytest.raises(NotImplementedError, match="3x3 pad-1 residual convolutions.*max-pool"):
        QDaggerTrainer(_args(student_network="impala"), "cuda")
    with pytest.raises(ValueError, match="teacher_model_path is empty"):
        QDaggerTrainer(_args(), "cuda")
    path = _teacher_file(tmp_path)
    for bad in (0.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="teacher mean return"):
            QDaggerTrainer(_args(teacher_model_path=path, teacher_return=bad), "cuda")
    with pytest.raises(ValueError, match="18 actions, the env ALE/Pong-v5 has 6"):
        QDaggerTrainer(_args(teacher_model_path=_teacher_file(tmp_path, 18), teacher_return=5.0),
                       "cuda")
    with pytest.raises(ValueError, match="does not fit observations"):
        QDaggerTrainer(_args(teacher_model_path=path, teacher_return=5.0, num_features=8), "cuda")


def test_teacher_file_forms_load_the_same_network(tmp_path):
    from oc_cleanrl_amd.dqn import QNetworkObj
    from oc_cleanrl_amd.qdagger import load_teacher

    torch.manual_seed(3)
    net = QNetworkObj((4, 12), 6, (32,), (256,))
    torch.save(net.state_dict(), tmp_path / "bare.pt")
    torch.save({"model_weights": net.state_dict(),
                "args": {"encoder_dims": (32,), "decoder_dims": (256,)}},
               tmp_path / "dqn.cleanrl_model")
    # the payload's recorded dims build the teacher, whatever the student's are
    a = _args(encoder_dims=(64, 64), decoder_dims=(512,))
    t1 = load_teacher(str(tmp_path / "dqn.cleanrl_model"), a)
    t2 = load_teacher(str(tmp_path / "bare.pt"), _args())
    for (k1, v1), (k2, v2) in zip(t1.state_dict().items(), t2.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2) and torch.equal(v1, net.state_dict()[k1])


@pytest.mark.parametrize("B,A_", [(7, 18), (32, 6)])
def test_twin_reproduces_the_scripts_loss_lines(B, A_):
    fx = np.load(GOLDEN / f"qdagger_loss_B{B}_A{A_}.npz")
    t = {k: torch.from_numpy(fx[k]) for k in ("q", "q_next", "q_teacher", "actions", "rewards",
                                              "dones")}
    for T in (1.0, 0.5):
        for coeff in (1.0, 0.37):
            pre = f"T{T}_c{coeff}_"
            st64, dq64 = qu.loss_twin(**t, gamma=0.99, temperature=T, coeff=coeff)
            st32, dq32 = qu.loss_twin(**t, gamma=0.99, temperature=T, coeff=coeff,
                                      dtype=torch.float32)
            for i, k in enumerate(("loss", "q_loss", "distill_loss", "q_values")):
                want = float(fx[pre + "f64_" + k])
                assert abs(float(st64[i]) - want) <= 1e-12 * max(abs(want), 1e-300), (pre, k)
                lu.check(pre + k, st32[i], fx[pre + "f32_" + k], fx[pre + "f64_" + k])
            want = torch.from_numpy(fx[pre + "f64_dq"])
            assert float((dq64 - want).abs().max()) <= 1e-12 * float(want.abs().max()), pre
            lu.check(pre + "dq", dq32, fx[pre + "f32_dq"], want)
            # the twin under autograd (the trainer test's restatement) gives the same gradient
            q = t["q"].double().requires_grad_(True)
            qu.loss_terms(q, t["q_next"].double(), t["q_teacher"].double(), t["actions"],
                          t["rewards"].double(), t["dones"].double(), 0.99, T, coeff)[0].backward()
            assert float((q.grad - want).abs().max()) <= 1e-12 * float(want.abs().max())


def _run(steps, E=1, teacher=5.0):
    return list(qu.episode_ring_ref(steps, E, teacher))


def test_episode_ring_ref_on_hand_written_sequences():
    one = lambda r, d: ([r], [d])  # noqa: E731
    # episodes of two steps, return 1 + 2 = 3: fewer than 10 episodes leave the coefficient at 1
    steps = [one(1.0, 0), one(2.0, 1)] * 9
    out = _run(steps)
    assert all(c == np.float32(1.0) for _, _, c in out)
    assert out[-1][0] == [3.0] * 9 and out[0][1][0] == 1.0 and out[1][1][0] == 0.0
    # exactly 10: mean 3 against a teacher of 5
    out = _run(steps + [one(1.0, 0), one(2.0, 1)])
    assert out[-2][2] == np.float32(1.0)
    assert out[-1][2] == np.float32(1 - 3.0 / 5.0) and len(out[-1][0]) == 10
    # wrap-around at 11 and 23: returns 1, 2, 3, ... one step each; the ring keeps the last ten
    for n in (11, 23):
        out = _run([one(float(i + 1), 1) for i in range(n)], teacher=100.0)
        last = [float(i) for i in range(n - 9, n + 1)]
        assert out[-1][0] == last
        assert out[-1][2] == np.float32(1 - (sum(last) / 10) / 100.0)
        ring, head, count = qu.ring_layout([float(i + 1) for i in range(n)])
        assert (head, count) == (n % 10, 10) and sorted(ring.tolist()) == last
    # returns above the teacher's: the coefficient stops at 0
    out = _run([one(7.0, 1)] * 10)
    assert out[-1][2] == np.float32(0.0) and out[-2][2] == np.float32(1.0)
    # several envs finishing at once enter in ascending env order
    out = _run([([1.0, 2.0, 3.0], [1, 0, 1]), ([1.0, 1.0, 1.0], [0, 1, 1])], E=3)
    assert out[0][0] == [1.0, 3.0] and out[1][0] == [1.0, 3.0, 3.0, 1.0]
    assert out[1][1].tolist() == [1.0, 0.0, 0.0]


def test_abi_refuses_bad_arguments_without_launch():
    from oc_cleanrl_amd import _lib

    L, d = _lib.LIB, ctypes.c_void_p(256)
    name = b"ocppo_qdagger_loss_fwd_bwd"
    loss = lambda B, A_, T=1.0, p=d, out=d: L.ocppo_qdagger_loss_fwd_bwd(  # noqa: E731
        None, p, d, d, d, d, d, B, A_, 0.99, T, None, out, out)
    for B, A_, T in ((8, 0, 1.0), (8, 1025, 1.0), (0, 6, 1.0), (-1, 6, 1.0), (8, 6, 0.0),
                     (8, 6, -1.0)):
        assert loss(B, A_, T) == _lib.OCPPO_E_INVALID
        assert name in L.ocppo_last_error() and b"bad sizes" in L.ocppo_last_error()
    for kw in (dict(p=None), dict(out=None)):
        assert loss(8, 6, **kw) == _lib.OCPPO_E_INVALID
        assert name in L.ocppo_last_error() and b"null pointer" in L.ocppo_last_error()
    for pos in range(1, 7):  # every required pointer on its own
        args = [None, d, d, d, d, d, d, 8, 6, 0.99, 1.0, None, d, d]
        args[pos] = None
        assert L.ocppo_qdagger_loss_fwd_bwd(*args) == _lib.OCPPO_E_INVALID
        assert b"null pointer" in L.ocppo_last_error()
    name = b"ocppo_qdagger_episode_push"
    push = lambda E, mean=5.0, p=d: L.ocppo_qdagger_episode_push(  # noqa: E731
        None, p, d, E, d, d, d, mean, d)
    assert push(0) == _lib.OCPPO_E_INVALID and b"bad sizes" in L.ocppo_last_error()
    assert name in L.ocppo_last_error()
    for mean in (0.0, float("nan"), float("inf")):
        assert push(4, mean) == _lib.OCPPO_E_INVALID and b"teacher_mean" in L.ocppo_last_error()
    assert push(4, p=None) == _lib.OCPPO_E_INVALID
    assert name in L.ocppo_last_error() and b"null pointer" in L.ocppo_last_error()


def test_ops_validate_before_any_launch():
    from oc_cleanrl_amd import ops

    z = torch.zeros(4, 6)
    with pytest.raises(ValueError, match="1 <= A <= 1024"):
        ops.qdagger_loss_fwd_bwd(torch.zeros(4, 0), z, z, z, z, z, 0.99, 1.0)
    with pytest.raises(ValueError, match="temperature"):
        ops.qdagger_loss_fwd_bwd(z, z, z, z, z, z, 0.99, 0.0)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.qdagger_loss_fwd_bwd(z, z, z, z, z, z, 0.99, 1.0)
