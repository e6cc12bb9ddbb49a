"""The recurrent PQN learner without a GPU: the flag surface and network of
pqn_atari_envpool_lstm.py, the torch path against the plain-loop twin of tests/pqn_lstm_util.py,
the trainer's host-side index pieces and the new C-ABI entries' validation."""
from __future__ import annotations

import ctypes
import dataclasses
import json

import numpy as np
import pytest
import torch
import torch.nn as nn

import pqn_lstm_util as U
from conftest import GOLDEN

ARGS_FX = json.loads((GOLDEN / "pqn_lstm_args.json").read_text())
KEYS_FX = json.loads((GOLDEN / "pqn_lstm_state_keys.json").read_text())


@pytest.fixture(scope="module")
def pl():
    from oc_cleanrl_amd import pqn_lstm

    return pqn_lstm


def test_args_match_the_script(pl):
    fields = dataclasses.fields(pl.PQNLSTMArgs)
    assert [f.name for f in fields[:len(ARGS_FX)]] == [n for n, _ in ARGS_FX]
    a = pl.PQNLSTMArgs()
    for n, d in ARGS_FX:
        assert getattr(a, n) == d, n
    assert (a.num_envs, a.num_steps, a.num_minibatches, a.update_epochs) == (8, 128, 4, 4)
    assert (a.q_lambda, a.max_grad_norm, a.learning_rate, a.anneal_lr) == (0.65, 0.5, 2.5e-4, True)
    own = {f.name: f.default for f in fields[len(ARGS_FX):]}
    assert own["architecture"] == "PQN_LSTM_OBJ" and own["obs_mode"] == "obj"
    assert own["backend"] == "Synthetic" and own["vecnorm_reward"] is False
    assert own["lstm_hidden"] == 128
    assert pl.ARCHITECTURES == ("PQN_LSTM_OBJ", "PQN_LSTM")
    for n in ("rollout_frame_cache", "rollout_fusion", "update_frame_dedup", "dp_overlap"):
        assert n not in own and getattr(a, n) is False, n
    assert pl.FUSED_PQN_LSTM and pl.FUSED_PQN_LSTM_ACT and pl.FUSED_PQN_LSTM_LOSS


def test_finalize_sizes_and_refusals(pl):
    A = pl.PQNLSTMArgs
    a = pl.finalize(A(num_envs=6, num_steps=10, num_minibatches=3, total_timesteps=1000))
    assert (a.batch_size, a.minibatch_size, a.num_iterations) == (60, 20, 16)  # :175-177
    assert (a.local_num_envs, a.local_batch_size, a.local_minibatch_size) == (6, 60, 20)
    with pytest.raises(NotImplementedError, match="one GPU"):
        pl.finalize(A(), world_size=2)
    with pytest.raises(NotImplementedError, match="architecture"):
        pl.finalize(A(architecture="PQN_OBJ"))
    with pytest.raises(ValueError, match="obs_mode"):
        pl.finalize(A(architecture="PQN_LSTM"))
    with pytest.raises(ValueError, match="obs_mode"):
        pl.finalize(A(obs_mode="dqn"))
    with pytest.raises(ValueError, match="whole environments"):
        pl.finalize(A(num_envs=6, num_minibatches=4))  # :304
    with pytest.raises(ValueError, match="lstm_hidden"):
        pl.finalize(A(lstm_hidden=48))
    with pytest.raises(ValueError, match="duration"):
        pl.finalize(A(exploration_fraction=0.0))


def _kinds(net):
    return [type(m).__name__ for m in net.network]


def test_network_keys_shapes_and_init(pl):
    from oc_cleanrl_amd.agents import EnvSpec

    torch.manual_seed(5)
    net = pl.PQNLSTMNetwork(EnvSpec((1, 84, 84), 6), "PQN_LSTM")
    sd = net.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == KEYS_FX
    H = net.lstm.hidden_size
    assert H == 128 and net.lstm.num_layers == 1
    for k in ("lstm.bias_ih_l0", "lstm.bias_hh_l0", "q_func.bias"):
        assert not sd[k].any(), k
    # nn.init.orthogonal_(param, 1.0) on the whole [4H, I] matrix: orthonormal columns when it is
    # tall, orthonormal rows otherwise
    for k in ("lstm.weight_ih_l0", "lstm.weight_hh_l0"):
        w = sd[k].double()
        gram = w.t() @ w if w.shape[0] >= w.shape[1] else w @ w.t()
        assert torch.allclose(gram, torch.eye(gram.shape[0], dtype=torch.float64), atol=1e-5), k
    wq = sd["q_func.weight"].double()  # layer_init at the default gain sqrt(2), 6 x 128: rows
    assert torch.allclose(wq @ wq.t(), 2.0 * torch.eye(6, dtype=torch.float64), atol=1e-5)
    kinds = _kinds(net)
    assert kinds.count("ReLU") == 4
    for i, kind in enumerate(kinds):
        if kind == "ReLU":
            assert kinds[i - 1] == "LayerNorm", kinds
    # the same seed reproduces the script's construction order: trunk, then lstm, then q_func
    torch.manual_seed(5)
    from oc_cleanrl_amd import pqn
    from oc_cleanrl_amd.agents import layer_init
    from oc_cleanrl_amd.lstm import init_lstm

    layers, d = pqn.trunk_layers(EnvSpec((1, 84, 84), 6), True)
    lstm = init_lstm(nn.LSTM(d, 128))
    head = layer_init(nn.Linear(128, 6))
    assert torch.equal(lstm.weight_hh_l0, net.lstm.weight_hh_l0)
    assert torch.equal(head.weight, net.q_func.weight)


def test_object_network_reuses_pqn_trunk(pl):
    from oc_cleanrl_amd import pqn
    from oc_cleanrl_amd.agents import EnvSpec

    torch.manual_seed(3)
    net = pl.PQNLSTMNetwork(EnvSpec((4, 12), 6), "PQN_LSTM_OBJ", 32, None, (32, 16), (32,))
    torch.manual_seed(3)
    ref = pqn.PQNetwork(EnvSpec((4, 12), 6), "PQN_OBJ", None, (32, 16), (32,))
    assert _kinds(net) == [type(m).__name__ for m in ref.network][:-1]
    for a, b in zip(net.network.parameters(), ref.network.parameters()):
        assert torch.equal(a, b)
    assert list(net.state_dict())[-6:] == ["lstm.weight_ih_l0", "lstm.weight_hh_l0",
                                           "lstm.bias_ih_l0", "lstm.bias_hh_l0", "q_func.weight",
                                           "q_func.bias"]
    assert net.lstm.input_size == 32 and net.lstm.hidden_size == 32


@pytest.mark.parametrize("done_at", ["middle", "first", "last", "none"])
@pytest.mark.parametrize("arch", ["PQN_LSTM_OBJ", "PQN_LSTM"])
def test_torch_path_equals_the_plain_loop_twin(pl, arch, done_at):
    """forward on the torch path (CPU tensors) against pqn_lstm_util.forward_ref at T = 3, B = 2:
    q and the final state agree to f32 rounding (the rule of lstm_util.check against the f64
    twin; nn.LSTM's cell is not assumed to sum in the twin's order), and a done at the first step
    cuts the incoming state off exactly."""
    from oc_cleanrl_amd.agents import EnvSpec

    T, B, A = 3, 2, 6
    pixels = arch == "PQN_LSTM"
    torch.manual_seed(11)
    if pixels:
        net = pl.PQNLSTMNetwork(EnvSpec((1, 84, 84), A), arch)
        x = torch.randint(0, 256, (T * B, 1, 84, 84)).float()
    else:
        net = pl.PQNLSTMNetwork(EnvSpec((4, 12), A), arch, 32, None, (32, 16), (32,))
        x = torch.randn(T * B, 4, 12)
    H = net.lstm.hidden_size
    done = torch.zeros(T, B)
    if done_at != "none":
        done[{"middle": 1, "first": 0, "last": 2}[done_at], 1] = 1.0
    done = done.view(-1)
    h0, c0 = torch.randn(1, B, H), torch.randn(1, B, H)
    with torch.no_grad():
        q, (hT, cT) = net(x, (h0, c0), done)
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    q32, _, (h32, c32) = U.forward_ref(sd, x, (h0, c0), done, pixels)
    q64, _, (h64, c64) = U.forward_ref({k: v.double() for k, v in sd.items()}, x.double(),
                                       (h0.double(), c0.double()), done.double(), pixels)
    assert q.shape == (T * B, A) and hT.shape == cT.shape == (1, B, H)
    U.check("q", q, q32, q64)
    U.check("hT", hT, h32, h64)
    U.check("cT", cT, c32, c64)
    if done_at == "first":  # env 1 starts from a zero state: its outputs do not see h0 / c0
        with torch.no_grad():
            q2, _ = net(x, (h0 + 1.0, c0 - 1.0), done)
        assert torch.equal(q2.view(T, B, A)[:, 1], q.view(T, B, A)[:, 1])
        assert not torch.equal(q2.view(T, B, A)[:, 0], q.view(T, B, A)[:, 0])


def test_minibatch_indices_and_state_slices_are_the_scripts(pl):
    """The trainer's host-side pieces: the epoch's sample order is flatinds[:, mbenvinds].ravel()
    for the script's shuffle stream (:304-316, transcribed), and the first envs-per-minibatch
    entries of a minibatch are its environments, by which the trainer slices init_h / init_c and
    the dones (:318-322)."""
    from oc_cleanrl_amd import lstm

    assert pl.PQNLSTMTrainer._shuffle is lstm.LSTMTrainer._shuffle
    assert pl.PQNLSTMTrainer._minibatch_hidden is lstm.LSTMTrainer._minibatch_hidden
    assert pl.PQNLSTMTrainer._rollout_begin is lstm.LSTMTrainer._rollout_begin
    num_envs, num_steps, nmb, epochs = 8, 4, 4, 3
    rng = np.random.RandomState(7)
    envinds = np.arange(num_envs)
    got = [pl.epoch_indices(envinds, rng, num_steps, nmb) for _ in range(epochs)]
    np.random.seed(7)
    envsperbatch = num_envs // nmb
    ref_envinds = np.arange(num_envs)
    flatinds = np.arange(num_envs * num_steps).reshape(num_steps, num_envs)
    init_h = torch.arange(num_envs * 5.0).view(1, num_envs, 5)
    dones = torch.rand(num_steps, num_envs)
    for e in range(epochs):
        np.random.shuffle(ref_envinds)
        for k, start in enumerate(range(0, num_envs, envsperbatch)):
            mbenvinds = ref_envinds[start:start + envsperbatch]
            mb_inds = flatinds[:, mbenvinds].ravel()
            M = mb_inds.size
            mine = got[e][k * M:(k + 1) * M]
            assert np.array_equal(mine, mb_inds)
            envs = torch.from_numpy(mine[:envsperbatch])
            assert torch.equal(init_h[0].index_select(0, envs), init_h[:, mbenvinds][0])
            assert torch.equal(dones.view(-1).index_select(0, torch.from_numpy(mine)),
                               dones.view(-1)[mb_inds])


def test_abi_refuses_bad_arguments_without_a_launch():
    from oc_cleanrl_amd import _lib

    L, d = _lib.LIB, ctypes.c_void_p(256)
    bad = _lib.OCPPO_E_INVALID

    def act(N=4, I=8, H=64, A=6, h=d, commit=1, actions=d, wq=d):
        return L.ocppo_pqn_lstm_act(None, d, d, d, d, d, d, N, I, H, h, d, commit, wq, d, A, 0, d,
                                    0, 1.0, 0.1, 10.0, actions, d, None, None)

    assert act(H=48) == bad and b"not in {32, 64, 128}" in L.ocppo_last_error()
    for A in (0, 19):
        assert act(A=A) == bad and b"1 <= A <= 18" in L.ocppo_last_error()
    assert act(h=None) == bad and b"null pointer" in L.ocppo_last_error()
    assert act(actions=None) == bad and b"null pointer" in L.ocppo_last_error()
    assert act(N=-1) == bad and act(I=0) == bad
    assert act(wq=ctypes.c_void_p(260)) == bad and b"16-B aligned" in L.ocppo_last_error()
    assert act(N=0, h=None) == 0

    def loss(M=8, H=64, A=6, h=d, ws=d, nbytes=1 << 24):
        return L.ocppo_pqn_head_loss_fwd_bwd(None, h, d, d, d, d, M, H, A, d, d, d, d, ws, nbytes)

    for H in (0, 6, 1028):
        assert loss(H=H) == bad and L.ocppo_pqn_head_loss_workspace_bytes(8, H, 6) == 0
    for A in (0, 19):
        assert loss(A=A) == bad and b"1 <= A <= 18" in L.ocppo_last_error()
    assert loss(M=-1) == bad
    assert loss(h=None) == bad and b"null pointer" in L.ocppo_last_error()
    assert loss(nbytes=8) == _lib.OCPPO_E_WORKSPACE
    assert loss(ws=None) == _lib.OCPPO_E_WORKSPACE
    assert loss(M=0, h=None, ws=None, nbytes=0) == 0
    n = L.ocppo_pqn_head_loss_workspace_bytes(67, 128, 18)
    assert n % 16 == 0 and n >= 4 * (67 + 3 * (18 * 128 + 18 + 2))


def test_ops_refuse_cpu_tensors():
    from oc_cleanrl_amd import ops

    x, h, wq = torch.zeros(2, 8), torch.zeros(2, 32), torch.zeros(6, 32)
    assert not ops.pqn_lstm_act_ok(x, h, wq) and not ops.pqn_head_loss_ok(h, wq)
    with pytest.raises(ValueError, match="pqn_lstm_act_ok"):
        ops.pqn_lstm_act(x, None, None, None, None, None, h, h, wq, None, 0, None, 1.0, 0.1, 1.0)
    with pytest.raises(ValueError, match="pqn_head_loss_ok"):
        ops.pqn_head_loss_fwd_bwd(h, wq, None, None, None)
