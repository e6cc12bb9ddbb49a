"""trainer.ROLLOUT_FUSED_STEP: the policy head + env step of rollout step t-1 folded into step t's
store + encoder launch (ops.head_env_store_linear2) give bit for bit the rollout of the
five-launch chain, eager and captured, and the entry point alone is bitwise
ops.policy_head_env_step followed by ops.store_linear2.

Shapes: N = 24 envs (a partial 16-row tile, two owner workgroups), W = 4, F = 12, A = 6, T = 6
(the stack wraps) and T = 5 (odd and even counts of fused steps). The synthetic env ends an
episode with probability 1/3500 per step, so the env seeds below were searched on the host for
resets inside the window and on its last step; the tests assert that those resets occurred."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, W, F, A = 24, 4, 12, 6
# env seed -> a done at some step 0..T-2 AND one at step T-1 within two iterations of T steps
SEED_FOR_T = {5: 527, 6: 579}
# env 16 ends an episode at step ids 1 and 2 (the first two steps after the reset)
KERNEL_SEED = 38784

ROLLOUT_KEYS = ("obs", "actions", "logprobs", "values", "rewards", "dones", "advantages", "returns",
                "enc_cache", "net_obs", "ret_state", "rms_state")
ENV_KEYS = ("frame", "reward", "done", "ep_state", "step_base")


def _args(T, graphs):
    from oc_cleanrl_amd.args import Args, finalize

    return finalize(Args(env_id="ALE/Pong-v5", obs_mode="obj", architecture="PPO_OBJ", num_envs=N,
                         num_steps=T, num_minibatches=2, update_epochs=1, num_features=F,
                         total_timesteps=N * T * 10, encoder_dims=(32, 64, 48, 64),
                         decoder_dims=(256,), seed=SEED_FOR_T[T], cuda_graphs=graphs,
                         save_model=False), 1)


def _snapshot(tr):
    snap = {k: getattr(tr, k).clone() for k in ROLLOUT_KEYS}
    snap.update({"env." + k: getattr(tr.env, k).clone() for k in ENV_KEYS})
    snap["params"] = torch.cat([p.detach().reshape(-1) for p in tr.agent.parameters()]).clone()
    return snap


def _run(T, graphs, on, dev):
    """Two iterations with the switch set to `on`: (snapshot after each, fused launches seen)."""
    from oc_cleanrl_amd import ops, trainer
    from oc_cleanrl_amd.trainer import PPOTrainer

    old, real, calls = trainer.ROLLOUT_FUSED_STEP, ops.head_env_store_linear2, []

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    trainer.ROLLOUT_FUSED_STEP, ops.head_env_store_linear2 = on, spy
    try:
        tr = PPOTrainer(_args(T, graphs), dev)
        assert tr.fused_step_ok and tr.cache_ring
        snaps = []
        for _ in range(2):
            tr.train_iteration()
            torch.cuda.synchronize()
            snaps.append(_snapshot(tr))
        assert tr.graphs_ready == graphs
    finally:
        trainer.ROLLOUT_FUSED_STEP, ops.head_env_store_linear2 = old, real
    return snaps, len(calls)


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("T", [6, 5])
def test_fused_step_rollout_is_bitwise_the_five_launch_chain(dev, T, graphs):
    ref, n_ref = _run(T, graphs, False, dev)
    got, n_got = _run(T, graphs, True, dev)
    # eager: T-1 fused launches per rollout; captured: iteration 1 eager + one capture
    assert n_ref == 0 and n_got == 2 * (T - 1)
    for it in range(2):
        for k in ref[it]:
            assert torch.equal(ref[it][k], got[it][k]), (it, k)
    dones = torch.stack([s["dones"] for s in ref])  # [2, T+1, N]; row t+1 = the env's step t
    assert dones[:, 1:T].any(), "no reset inside the window"
    assert dones[:, T].any(), "no reset on the last step"


@pytest.mark.parametrize("H,dtype,vecnorm", [(256, torch.bfloat16, True), (512, torch.float32, False),
                                             (512, torch.bfloat16, True)])
def test_head_env_store_linear2_is_bitwise_the_two_launches(dev, H, dtype, vecnorm):
    from oc_cleanrl_amd import ops
    from oc_cleanrl_amd.envs import SyntheticAtariEnv

    g = torch.Generator(device="cpu").manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
    N1, N2 = 32, 64
    wa, ba, wc, bc = rnd(A, H) * 0.05, rnd(A) * 0.1, rnd(1, H) * 0.05, rnd(1) * 0.1
    w1, b1, w2, b2 = rnd(N1, F) * 0.01, rnd(N1) * 0.1, rnd(N2, N1) * 0.1, rnd(N2) * 0.1
    assert ops.head_env_store_linear2_ok(rnd(N, H), wa, wc, SyntheticAtariEnv(
        "ALE/Pong-v5", "obj", N, F, KERNEL_SEED, dev, W))
    obs0 = torch.randint(0, 200, (N, W, F), generator=g).to(dev).to(dtype)

    def state():
        env = SyntheticAtariEnv("ALE/Pong-v5", "obj", N, F, KERNEL_SEED, dev, W)
        env.reset()
        env.ep_state[:, :2] = torch.arange(2 * N, device=dev, dtype=torch.float32).view(N, 2)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731
        return dict(env=env, obs=[obs0.clone(), torch.zeros_like(obs0), torch.zeros_like(obs0)],
                    net=z(N, W, F), act=z(2, N, dt=torch.int64), lp=z(2, N), val=z(2, N),
                    rew=z(2, N), done=z(2, N), y=z(2, N, N2), ret=z(N, dt=torch.float64),
                    rms=torch.tensor([0.0, 1.0, 1e-4], dtype=torch.float64, device=dev))

    ref, got = state(), state()
    for t in range(2):  # two consecutive steps: the second starts from the first's outputs
        hidden, noise = rnd(N, H), torch.empty(N, A).exponential_(generator=g).to(dev)
        head = (hidden, wa, ba, wc.view(-1), bc, noise)
        s = ref
        vn = (s["ret"], s["rms"]) if vecnorm else None
        ops.policy_head_env_step(*head, s["act"][t], s["lp"][t], s["val"][t], s["env"], t)
        ops.store_linear2(s["env"].frame, s["env"].reward, s["env"].done, s["obs"][t],
                          s["obs"][t + 1], s["net"], s["done"][t], s["rew"][t], w1, b1, w2, b2,
                          s["y"][t], vecnorm_state=vn)
        s = got
        vn = (s["ret"], s["rms"]) if vecnorm else None
        ops.head_env_store_linear2(*head, s["act"][t], s["lp"][t], s["val"][t], s["env"], t,
                                   s["obs"][t], s["obs"][t + 1], s["net"], s["done"][t],
                                   s["rew"][t], w1, b1, w2, b2, s["y"][t], vecnorm_state=vn)
        torch.cuda.synchronize()
        for k in ("net", "act", "lp", "val", "rew", "done", "y", "ret", "rms"):
            assert torch.equal(ref[k], got[k]), (t, k)
        assert torch.equal(ref["obs"][t + 1], got["obs"][t + 1]), t
        for k in ENV_KEYS:
            assert torch.equal(getattr(ref["env"], k), getattr(got["env"], k)), (t, k)
        assert ref["done"][t].any(), "no reset at this step"
    assert ref["act"].unique().numel() > 1
