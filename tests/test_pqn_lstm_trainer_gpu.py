"""pqn_lstm.PQNLSTMTrainer end to end on the Synthetic object env (4 envs x 4 steps, 2 minibatches,
2 epochs, 2 iterations = 8 optimizer steps, lstm_hidden = 32, a small PQN_LSTM_OBJ trunk) with an
episode end inside the first rollout, and one pixel iteration."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import pqn_lstm_util as U

pytestmark = pytest.mark.gpu

N, T, NMB, EPOCHS, ITERS = 4, 4, 2, 2, 2
M64 = (1 << 64) - 1


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _synth_done(seed: int, step: int, n: int) -> bool:
    """The Synthetic env's done of env n at step id `step` (csrc/ocppo_synth_env.h)."""
    key = _splitmix64((_splitmix64((_splitmix64(seed) + step) & M64) + n) & M64)
    ud = np.float32(_splitmix64(key ^ 0xB5297A4D) >> 40) * np.float32(1.0 / 16777216.0)
    return bool(ud < np.float32(1.0 / 3500.0))


def _seed_with_an_episode_end():
    """The first seed whose first rollout has a done with a step after it: env step t (step id
    1 + t; the reset took id 0) lands in dones[t + 1], and t + 1 <= T - 1."""
    from oc_cleanrl_amd.trainer import rank_seeds

    for seed in range(1, 200000):
        s = rank_seeds(seed, 0)[1]
        hits = [(t + 1, n) for t in range(T - 1) for n in range(N) if _synth_done(s, 1 + t, n)]
        if hits:
            return seed, hits
    raise AssertionError("no seed with an episode end")


SEED, DONE_AT = _seed_with_an_episode_end()


def _args(pl, **kw):
    base = dict(num_envs=N, num_steps=T, num_minibatches=NMB, update_epochs=EPOCHS,
                lstm_hidden=32, encoder_dims=(32, 16), decoder_dims=(32,), buffer_window_size=4,
                num_features=8, total_timesteps=N * T * ITERS, exploration_fraction=0.5,
                save_model=False, gemm_table=False, seed=SEED)
    base.update(kw)
    return pl.finalize(pl.PQNLSTMArgs(**base))


def _run(dev, own=(True, True, True), fused_pqn=True, fused_lstm=True, graphs=True):
    """ITERS iterations; per iteration the data the update consumed, and the end state. own:
    (FUSED_PQN_LSTM, FUSED_PQN_LSTM_ACT, FUSED_PQN_LSTM_LOSS)."""
    from oc_cleanrl_amd import lstm, pqn, pqn_lstm as pl

    old = (pl.FUSED_PQN_LSTM, pl.FUSED_PQN_LSTM_ACT, pl.FUSED_PQN_LSTM_LOSS, pqn.FUSED_PQN,
           lstm.FUSED_LSTM)
    pl.FUSED_PQN_LSTM, pl.FUSED_PQN_LSTM_ACT, pl.FUSED_PQN_LSTM_LOSS = own
    pqn.FUSED_PQN, lstm.FUSED_LSTM = fused_pqn, fused_lstm
    try:
        tr = pl.PQNLSTMTrainer(_args(pl, cuda_graphs=graphs), dev, log=False)
        c = lambda t: t.detach().cpu().clone()  # noqa: E731
        out = dict(sd0={k: c(v) for k, v in tr.agent.state_dict().items()}, its=[], tr=tr,
                   fused_act=tr.fused_act, fused_loss=tr.fused_loss)
        for _ in range(ITERS):
            m = tr.train_iteration()
            out["its"].append(dict(
                obs=c(tr.obs[:T]).float(), actions=c(tr.actions), returns=c(tr.returns),
                rewards=c(tr.rewards), values=c(tr.values[:T]), dones=c(tr.dones),
                next_q=c(tr.next_q), perm=c(tr.perm_dev), lr=float(tr.lr), metrics=m,
                init_h=c(tr.init_h), init_c=c(tr.init_c), lstm_h=c(tr.lstm_h),
                lstm_c=c(tr.lstm_c), eps=float(tr.epsilon)))
        torch.cuda.synchronize()
        out["sd"] = {k: c(v) for k, v in tr.agent.state_dict().items()}
        out["flat"] = c(tr.optimizer.params) if fused_pqn else None
        out["graphs_ready"] = tr.graphs_ready
        return out
    finally:
        (pl.FUSED_PQN_LSTM, pl.FUSED_PQN_LSTM_ACT, pl.FUSED_PQN_LSTM_LOSS, pqn.FUSED_PQN,
         lstm.FUSED_LSTM) = old


@pytest.fixture(scope="module")
def fused(dev):
    return _run(dev)


@pytest.fixture(scope="module")
def composed(dev):
    """All three of this module's switches off: the parents' existing kernels, composed."""
    return _run(dev, own=(False, False, False))


@pytest.fixture(scope="module")
def torch_path(dev):
    """The full torch path: this module's switches, pqn.FUSED_PQN and lstm.FUSED_LSTM off."""
    return _run(dev, own=(False, False, False), fused_pqn=False, fused_lstm=False, graphs=False)


def test_returns_are_bitwise_the_twin_and_an_episode_ends(fused):
    from oc_cleanrl_amd import ops, pqn_lstm as pl

    a = fused["tr"].args
    assert fused["fused_act"] and fused["fused_loss"] and fused["graphs_ready"]
    d0 = fused["its"][0]["dones"]
    for t, n in DONE_AT:  # the host restatement of the env's done found the seed
        assert d0[t, n] == 1.0
    assert 0 < float(d0[1:T].sum())
    for i, it in enumerate(fused["its"]):
        want = U.q_lambda_ref(it["rewards"], it["values"], it["dones"][:T], it["next_q"],
                              it["dones"][T], a.gamma, a.q_lambda)
        assert torch.equal(it["returns"], want)
        assert int(it["actions"].min()) >= 0 and int(it["actions"].max()) < fused["tr"].A
        m = it["metrics"]
        assert set(m) >= {"charts/learning_rate", "charts/epsilon", "losses/td_loss",
                          "losses/q_values"}
        assert np.isfinite(m["losses/td_loss"]) and np.isfinite(m["losses/q_values"])
        want_eps = pl.linear_schedule(a.start_e, a.end_e,
                                      a.exploration_fraction * a.total_timesteps,
                                      (i + 1) * T * N)
        assert abs(m["charts/epsilon"] - want_eps) <= 1e-6 and abs(it["eps"] - want_eps) <= 1e-6
    assert isinstance(fused["tr"].optimizer, ops.FlatRAdam)
    assert float(fused["tr"].optimizer.scalars[0]) == ITERS * EPOCHS * NMB


def _replay(sd, it, dtype):
    """forward step by step from init_h / init_c over the stored observations and dones:
    (greedy values [T, N], the state after the last step)."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    state = (it["init_h"].to(dtype).unsqueeze(0), it["init_c"].to(dtype).unsqueeze(0))
    vals = []
    for t in range(T):
        q, _, state = U.forward_ref(p, it["obs"][t].to(dtype), state, it["dones"][t].to(dtype))
        vals.append(q.max(1).values)
    return torch.stack(vals), state


@pytest.mark.parametrize("which", ["fused", "composed"])
def test_values_and_carried_state_follow_the_step_by_step_forward(which, request):
    """Iteration 1 ran on the initial parameters: values[t] is the greedy Q of forward(obs[t],
    state_t, dones[t]) from init_h / init_c = 0, the state after step T - 1 is lstm_h / lstm_c
    (the bootstrap did not move it), and an environment restarts from a zero state on the step
    after its done (the twin masks it; the done is inside the rollout)."""
    run = request.getfixturevalue(which)
    it = run["its"][0]
    assert not it["init_h"].any() and not it["init_c"].any()
    v32, (h32, c32) = _replay(run["sd0"], it, torch.float32)
    v64, (h64, c64) = _replay(run["sd0"], it, torch.float64)
    U.check("values", it["values"], v32, v64)
    U.check("lstm_h", it["lstm_h"], h32[0], h64[0])
    U.check("lstm_c", it["lstm_c"], c32[0], c64[0])
    t, n = DONE_AT[0]
    # env n at step t starts afresh: its value there is that of a zero state on obs[t] alone
    p = {k: v.double() for k, v in run["sd0"].items()}
    H = it["init_h"].shape[1]
    zero = (torch.zeros(1, N, H, dtype=torch.float64), torch.zeros(1, N, H, dtype=torch.float64))
    q, _, _ = U.forward_ref(p, it["obs"][t].double(), zero, torch.zeros(N, dtype=torch.float64))
    assert abs(float(q.max(1).values[n]) - float(it["values"][t, n])) <= 1e-5
    # the next iteration's snapshot is this iteration's final state
    nxt = run["its"][1]
    assert torch.equal(nxt["init_h"], it["lstm_h"]) and torch.equal(nxt["init_c"], it["lstm_c"])
    assert not torch.equal(nxt["lstm_h"], it["lstm_h"])


@pytest.mark.parametrize("own", [(True, True, True), (False, False, False)])
def test_bootstrap_leaves_the_carried_state_unchanged(dev, own):
    from oc_cleanrl_amd import pqn_lstm as pl

    old = pl.FUSED_PQN_LSTM, pl.FUSED_PQN_LSTM_ACT, pl.FUSED_PQN_LSTM_LOSS
    pl.FUSED_PQN_LSTM, pl.FUSED_PQN_LSTM_ACT, pl.FUSED_PQN_LSTM_LOSS = own
    try:
        tr = pl.PQNLSTMTrainer(_args(pl, cuda_graphs=False), dev, log=False)
    finally:
        pl.FUSED_PQN_LSTM, pl.FUSED_PQN_LSTM_ACT, pl.FUSED_PQN_LSTM_LOSS = old
    assert tr.fused_act == own[0]
    seen, end = [], tr._rollout_end

    def spy():
        seen.append((tr.lstm_h.clone(), tr.lstm_c.clone()))
        end()

    tr._rollout_end = spy
    tr._load_staged()
    tr._rollout()
    torch.cuda.synchronize()
    assert float(seen[0][0].abs().max()) > 0
    assert torch.equal(tr.lstm_h, seen[0][0]) and torch.equal(tr.lstm_c, seen[0][1])
    assert float(tr.next_q.abs().max()) > 0
    tr.close()


def _twin_update(run, dtype):
    """The update of pqn_atari_envpool_lstm.py:304-331 in `dtype` plain torch over the data each
    of `run`'s iterations consumed (observations, actions, returns, dones, initial state and
    permutation), from its initial parameters: the state dict after all iterations."""
    tr = run["tr"]
    p = {k: v.to(dtype).clone().requires_grad_() for k, v in run["sd0"].items()}
    ref = U.RAdamRef([v.detach() for v in p.values()], 0.0)
    M, B, epb = tr.M, tr.B, tr.envs_per_mb
    for it in run["its"]:
        ref.lr = it["lr"]
        obs = it["obs"].view((B,) + tr.obs_shape).to(dtype)
        acts, rets = it["actions"].view(-1), it["returns"].view(-1).to(dtype)
        dones = it["dones"][:T].reshape(-1).to(dtype)
        for j in range(EPOCHS * NMB):
            idx = it["perm"][j * M:(j + 1) * M]
            envs = idx[:epb]
            state = (it["init_h"][envs].to(dtype).unsqueeze(0),
                     it["init_c"][envs].to(dtype).unsqueeze(0))
            q, _, _ = U.forward_ref(p, obs[idx], state, dones[idx])
            old = q.gather(1, acts[idx].unsqueeze(-1)).squeeze(-1)
            loss = torch.nn.functional.mse_loss(rets[idx], old)
            grads = torch.autograd.grad(loss, list(p.values()))
            c, _ = U.clip_coef(grads, tr.args.max_grad_norm)
            ref.step([g * c for g in grads])
            for v, new in zip(p.values(), ref.params):
                v.data.copy_(new)
    return {k: v.detach() for k, v in p.items()}


def test_fused_equals_composed_in_the_rollout_and_agrees_in_the_update(fused, composed,
                                                                       torch_path):
    """All three switches on against all three off (the parents' kernels, composed): the rollout
    buffers and the returns are bitwise equal, the act kernel being bitwise. The parameters after
    8 optimizer steps are held to the tolerance tests/test_pqn_trainer_gpu.py uses for its own
    fused-versus-torch comparison (pqn_util.check = lstm_util.check, the rule of DESIGN.md 11):
    the error against the f64 twin of the update, relative to the twin's largest element, is at
    most max(3 x the torch path's own error, 4 * 2^-23). The fused run against the full torch path
    is held to the same rule."""
    assert not composed["fused_act"] and not composed["fused_loss"] and composed["graphs_ready"]
    a, b = fused["its"][0], composed["its"][0]
    for k in ("obs", "actions", "values", "dones", "rewards", "next_q", "returns", "lstm_h",
              "lstm_c", "perm"):
        assert torch.equal(a[k], b[k]), k
    for a, b in zip(fused["its"], torch_path["its"]):
        assert torch.equal(a["actions"], b["actions"]) and torch.equal(a["obs"], b["obs"])
    for a, b in zip(fused["its"], composed["its"]):
        assert torch.equal(a["actions"], b["actions"]) and torch.equal(a["obs"], b["obs"])
    twin = _twin_update(fused, torch.float64)
    for k in twin:
        U.check(f"params {k} (fused)", fused["sd"][k], torch_path["sd"][k], twin[k])
        U.check(f"params {k} (composed)", composed["sd"][k], torch_path["sd"][k], twin[k])


def test_graphs_off_and_a_second_run_are_bitwise_the_first(fused, dev):
    eager = _run(dev, graphs=False)
    again = _run(dev)
    assert not eager["graphs_ready"] and again["graphs_ready"]
    for other in (eager, again):
        assert torch.equal(other["flat"], fused["flat"])
        for a, b in zip(other["its"], fused["its"]):
            for k in ("returns", "actions", "values", "next_q", "lstm_h", "lstm_c", "init_h"):
                assert torch.equal(a[k], b[k]), k
            assert a["metrics"]["losses/td_loss"] == b["metrics"]["losses/td_loss"]


def test_pixel_architecture_runs_an_iteration(dev):
    from oc_cleanrl_amd import pqn_lstm as pl

    args = pl.finalize(pl.PQNLSTMArgs(
        architecture="PQN_LSTM", obs_mode="dqn", buffer_window_size=1, num_envs=2, num_steps=4,
        num_minibatches=2, update_epochs=1, total_timesteps=8, save_model=False))
    tr = pl.PQNLSTMTrainer(args, dev, log=False)
    m = tr.train_iteration()
    assert np.isfinite(m["losses/td_loss"]) and np.isfinite(m["losses/q_values"])
    keys = list(tr.agent.state_dict())
    assert keys[-2:] == ["q_func.weight", "q_func.bias"] and keys[0] == "network.0.weight"
    assert tr.agent.lstm.input_size == 512 and tr.agent.lstm.hidden_size == 128
    assert isinstance(tr.agent.network[1], torch.nn.LayerNorm)  # over [C, H, W]: torch's
    tr.close()
