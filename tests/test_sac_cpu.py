"""Discrete SAC, host side: the args surface, the networks' keys / shapes / seeded construction
order, the hand-written policy gradient against autograd, the acting stream's restatement, and the
new ABI functions' argument checks (no launch)."""
import ctypes
import dataclasses
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import sac_util as su

OBS, A = (4, 84, 84), 6


def test_args_defaults_are_the_scripts():
    from oc_cleanrl_amd.sac import SACArgs

    a = SACArgs()
    want = dict(exp_name="sac_atari", env_id="BeamRiderNoFrameskip-v4", total_timesteps=5_000_000,
                buffer_size=1_000_000, gamma=0.99, tau=1.0, batch_size=64, learning_starts=20000,
                policy_lr=3e-4, q_lr=3e-4, update_frequency=4, target_network_frequency=8000,
                alpha=0.2, autotune=True, target_entropy_scale=0.89)
    for k, v in want.items():
        assert getattr(a, k) == v, k
        assert type(getattr(a, k)) is type(v), k
    names = {f.name for f in dataclasses.fields(SACArgs)}
    assert {"obs_mode", "backend", "buffer_window_size", "num_envs", "num_features",
            "obs_storage", "encoder_dims", "decoder_dims", "cuda_graphs", "gemm_table", "log_dir",
            "save_model", "log_every", "vecnorm_reward"} <= names
    assert a.vecnorm_reward is False
    # DQNTrainer's names for the same two flags follow them, and are not flags themselves
    b = SACArgs(update_frequency=8, q_lr=1e-3)
    assert (b.train_frequency, b.learning_rate) == (8, 1e-3)
    assert not {"train_frequency", "learning_rate", "exploration_fraction"} & names


def test_cli_parses_the_scripts_flag_spellings():
    from oc_cleanrl_amd.args import parse_dataclass
    from oc_cleanrl_amd.sac import SACArgs

    a = parse_dataclass(SACArgs, ["--backend", "Synthetic", "--obs-mode", "obj",
                                  "--total-timesteps", "64", "--learning-starts", "16",
                                  "--buffer-size", "64", "--no-autotune"])
    assert (a.obs_mode, a.total_timesteps, a.learning_starts, a.buffer_size, a.autotune) == \
        ("obj", 64, 16, 64, False)


def test_state_dict_keys_and_shapes():
    from oc_cleanrl_amd.sac import Actor, ActorObj, SoftQNetwork, SoftQNetworkObj

    conv = {"conv.0.weight": (32, 4, 8, 8), "conv.0.bias": (32,), "conv.2.weight": (64, 32, 4, 4),
            "conv.2.bias": (64,), "conv.4.weight": (64, 64, 3, 3), "conv.4.bias": (64,),
            "fc1.weight": (512, 3136), "fc1.bias": (512,)}
    for cls, head in ((Actor, "fc_logits"), (SoftQNetwork, "fc_q")):
        sd = cls(OBS, A).state_dict()
        want = dict(conv, **{f"{head}.weight": (A, 512), f"{head}.bias": (A,)})
        assert {k: tuple(v.shape) for k, v in sd.items()} == want
        assert list(sd) == list(want)  # the script's order too
        assert all(float(v.abs().max()) == 0 for k, v in sd.items() if k.endswith("bias"))
    for cls in (ActorObj, SoftQNetworkObj):
        sd = cls((4, 12), A, (32,), (16,)).state_dict()
        assert {k: tuple(v.shape) for k, v in sd.items()} == {
            "network.0.weight": (32, 12), "network.0.bias": (32,), "network.3.weight": (16, 128),
            "network.3.bias": (16,), "network.5.weight": (A, 16), "network.5.bias": (A,)}


def _script_layer_init(layer):
    nn.init.kaiming_normal_(layer.weight)
    nn.init.constant_(layer.bias, 0.0)
    return layer


def _script_net(head: str):
    """sac_atari.py:111-161's constructors restated: the module creation order draws the init."""
    m = nn.Module()
    m.conv = nn.Sequential(_script_layer_init(nn.Conv2d(OBS[0], 32, kernel_size=8, stride=4)),
                           nn.ReLU(),
                           _script_layer_init(nn.Conv2d(32, 64, kernel_size=4, stride=2)),
                           nn.ReLU(),
                           _script_layer_init(nn.Conv2d(64, 64, kernel_size=3, stride=1)),
                           nn.Flatten())
    with torch.inference_mode():
        d = m.conv(torch.zeros(1, *OBS)).shape[1]
    m.fc1 = _script_layer_init(nn.Linear(d, 512))
    setattr(m, head, _script_layer_init(nn.Linear(512, A)))
    return m


def test_construction_order_matches_the_script():
    from oc_cleanrl_amd.sac import SACArgs, make_networks

    torch.manual_seed(7)
    actor, q, target = make_networks(SACArgs(), OBS, A)
    after = torch.rand(1)
    torch.manual_seed(7)
    s_actor, s_qf1, s_qf2 = _script_net("fc_logits"), _script_net("fc_q"), _script_net("fc_q")
    s_t1, s_t2 = _script_net("fc_q"), _script_net("fc_q")  # consume the generator, then overwritten
    s_t1.load_state_dict(s_qf1.state_dict())
    s_t2.load_state_dict(s_qf2.state_dict())
    assert torch.equal(after, torch.rand(1))  # the same number of draws
    for got, want in ((actor, s_actor), (q.qf1, s_qf1), (q.qf2, s_qf2), (target.qf1, s_t1),
                      (target.qf2, s_t2)):
        gs, ws = got.state_dict(), want.state_dict()
        assert list(gs) == list(ws)
        for k in gs:
            assert torch.equal(gs[k], ws[k]), k
    assert not torch.equal(q.qf1.fc_q.weight, q.qf2.fc_q.weight)
    # the twin's parameter order is list(qf1.parameters()) + list(qf2.parameters())
    for p, w in zip(q.parameters(), list(s_qf1.parameters()) + list(s_qf2.parameters())):
        assert torch.equal(p, w)


def test_forward_is_the_scripts():
    from oc_cleanrl_amd.sac import Actor, SoftQNetwork

    torch.manual_seed(3)
    x = torch.randint(0, 256, (2,) + OBS).float()
    for cls, head, scale_in_forward in ((SoftQNetwork, "fc_q", True), (Actor, "fc_logits", False)):
        net = cls(OBS, A)
        h = x / 255.0 if scale_in_forward else x
        want = getattr(net, head)(F.relu(net.fc1(F.relu(net.conv(h)))))
        assert torch.equal(net(x), want)
    actor = Actor(OBS, A)
    _, logp, probs = actor.get_action(x)
    assert torch.equal(logp, F.log_softmax(actor(x / 255.0), dim=1))
    assert torch.allclose(probs.sum(1), torch.ones(2))


def test_target_entropy_is_the_f32_value():
    from oc_cleanrl_amd.sac import target_entropy

    te = target_entropy(0.89, 6)
    assert te == float(-0.89 * torch.log(1 / torch.tensor(6)))
    assert te == pytest.approx(0.89 * math.log(6), rel=1e-6) and te != 0.89 * math.log(6)


@pytest.mark.parametrize("A_,B", [(1, 3), (2, 5), (6, 8), (18, 4)])
def test_dlogits_formula_equals_autograd(A_, B):
    g = torch.Generator().manual_seed(11 * A_ + B)
    logits = (2 * torch.randn(B, A_, generator=g)).double()
    logits[0, 0] += 90.0 if A_ > 1 else 0.0
    q1, q2 = torch.randn(B, A_, generator=g).double(), torch.randn(B, A_, generator=g).double()
    for alpha in (1e-3, 0.2, 5.0):
        ref = su.actor_ref(logits, q1, q2, alpha, torch.zeros(1, dtype=torch.float64), 1.5)
        got = su.dlogits_formula(logits, q1, q2, alpha)
        assert torch.isfinite(got).all()
        scale = float(ref["dlogits"].abs().max()) or 1.0
        assert float((got - ref["dlogits"]).abs().max()) <= 1e-13 * max(scale, 1.0)
        # d alpha_loss / d log_alpha = alpha_loss itself (the loss is linear in exp(log_alpha))
        assert float(ref["dlog_alpha"]) == pytest.approx(float(ref["alpha_loss"]), rel=1e-12)


@pytest.mark.parametrize("A_", [2, 6, 18])
def test_act_stream_restatement_leaves_few_close_rows(A_):
    """The committed seed of tests/test_sac_kernels_gpu.py: at most 4 of the 4096 rows have their
    two largest p_j / e_j within 1e-4 relative; the random phase is uniform over [0, A)."""
    E = 4096
    logits = 2 * torch.randn(E, A_, generator=torch.Generator().manual_seed(1234 + A_))
    acts, gaps = su.act_ref(logits, seed=5, t=100, learning_starts=100)
    close = sum(g <= 1e-4 for g in gaps)
    print(f"A={A_}: {close} rows within 1e-4")
    assert close <= 4
    assert all(0 <= a < A_ for a in acts)
    # the draw follows the distribution: the empirical mean log-prob is near -entropy
    p = torch.softmax(logits.double(), 1)
    picked = p[torch.arange(E), torch.tensor(acts)].log().mean()
    expect = (p * p.log()).sum(1).mean()
    assert abs(float(picked - expect)) < 0.1
    rnd, _ = su.act_ref(logits, seed=5, t=99, learning_starts=100)
    counts = torch.bincount(torch.tensor(rnd), minlength=A_).double()
    # Pearson's statistic against the uniform law: mean A - 1, standard deviation sqrt(2 (A - 1));
    # six of them and 10 more is beyond the 1e-4 tail for 1, 5 and 17 degrees of freedom
    chi2 = float(((counts - E / A_) ** 2 / (E / A_)).sum())
    assert chi2 < (A_ - 1) + 6 * math.sqrt(2 * (A_ - 1)) + 10, (chi2, counts.tolist())
    assert rnd != acts


def test_abi_refuses_bad_arguments_without_launch():
    from oc_cleanrl_amd import _lib

    L, d = _lib.LIB, ctypes.c_void_p(256)
    critic = lambda B, A_, p=d: L.ocppo_sac_critic_loss_fwd_bwd(  # noqa: E731
        None, p, d, d, d, d, d, d, d, B, A_, 0.99, d, d, d, d, None)
    actor = lambda B, A_, p=d, tune=1, st=d: L.ocppo_sac_actor_alpha_fwd_bwd(  # noqa: E731
        None, p, d, d, B, A_, d, d, 1.5, st, st, st, 3e-4, 0.9, 0.999, 1e-4, tune, d, d)
    act = lambda E, A_, p=d: L.ocppo_sac_act(None, p, E, A_, 1, d, 0, 10, d)  # noqa: E731
    for fn, name in ((critic, b"ocppo_sac_critic_loss_fwd_bwd"),
                     (actor, b"ocppo_sac_actor_alpha_fwd_bwd"), (act, b"ocppo_sac_act")):
        for bad_a in (0, 19):
            assert fn(8, bad_a) == _lib.OCPPO_E_INVALID
            assert name in L.ocppo_last_error() and b"bad sizes" in L.ocppo_last_error()
        assert fn(-1, 6) == _lib.OCPPO_E_INVALID and b"bad sizes" in L.ocppo_last_error()
        assert fn(8, 6, None) == _lib.OCPPO_E_INVALID
        assert b"null pointer" in L.ocppo_last_error()
        assert fn(0, 6, None) == _lib.OCPPO_OK  # a zero size is a no-op
    exact = lambda P, p=d, ws=d, n=1 << 20: L.ocppo_clip_adam_step_exact(  # noqa: E731
        None, p, d, d, d, P, d, 0.9, 0.999, 1e-4, 1.0, 0.0, d, ws, n)
    assert exact(0) == _lib.OCPPO_E_INVALID and b"bad size" in L.ocppo_last_error()
    assert exact(8, None) == _lib.OCPPO_E_INVALID and b"null pointer" in L.ocppo_last_error()
    assert exact(8, ws=None) == _lib.OCPPO_E_WORKSPACE
    assert exact(8, n=16) == _lib.OCPPO_E_WORKSPACE
    # autotune needs the Adam state
    assert actor(8, 6, st=None) == _lib.OCPPO_E_INVALID and b"null pointer" in L.ocppo_last_error()


def test_ops_validate_shapes_before_any_launch():
    from oc_cleanrl_amd import ops

    with pytest.raises(ValueError, match="A <= 18"):
        ops.sac_act(torch.zeros(4, 19), 1, torch.zeros(1, dtype=torch.int64), 10)
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.sac_act(torch.zeros(4, 6), 1, torch.zeros(1, dtype=torch.int64), 10)
    with pytest.raises(ValueError, match="A <= 18"):
        ops.sac_critic_loss_fwd_bwd(*[torch.zeros(4, 0)] * 5, None, None, None, 0.99, None)
