"""contppo.ContPPOTrainer on the GPU at N = 4, T = 16, 2 minibatches, 2 epochs: the fused kernels
against the plain-torch path, captured graphs against eager launches, Pendulum-v1 and a stub
device env with A = 3 action dimensions (the [T, N, A] strides through store, gather and loss),
RPO's noise, and the metric names."""
import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

N, T, NMB, EPOCHS, ITERS = 4, 16, 2, 2, 3
LR = 3e-4


class StubEnv:
    """A device env with D = 5 observations and A = 3 action dimensions in torch ops (all in
    place on preallocated tensors, so a captured rollout replays them): a contracting linear
    system driven by tanh(action), every env done on every 7th step."""

    pixels = False
    integer_obs = False

    def __init__(self, num_envs, device):
        self.num_envs, self.n_actions, self.window = num_envs, 3, 1
        self.frame_elems, self.single_obs_shape, self.frame_dtype = 5, (1, 5), torch.float32
        g = torch.Generator().manual_seed(5)
        self.init = torch.randn(num_envs, 5, generator=g).to(device)
        self.W = (0.5 * torch.randn(3, 5, generator=g)).to(device)
        self.s = torch.zeros((num_envs, 5), device=device)
        self.k = torch.zeros(1, dtype=torch.int64, device=device)
        self.frame = torch.zeros((num_envs, 5), device=device)
        self.reward = torch.zeros(num_envs, device=device)
        self.done = torch.zeros(num_envs, device=device)
        self.ep_state = torch.zeros((num_envs, 5), device=device)

    def reset(self):
        self.s.copy_(self.init)
        self.frame.copy_(torch.sin(self.s))
        return self.frame

    def step(self, actions, step_offset=0):
        assert actions.shape == (self.num_envs, 3) and actions.dtype == torch.float32
        self.s.mul_(0.9).add_(torch.tanh(actions) @ self.W)
        self.frame.copy_(torch.sin(self.s))
        self.reward.copy_(-0.1 * (self.s * self.s).sum(1))
        self.k.add_(1)
        self.done.copy_((self.k % 7 == 0).float().expand(self.num_envs))

    def advance(self, n):
        pass

    def pop_episode_stats(self):
        return [0.0, 0.0, 0.0]


def _args(contppo, **kw):
    base = dict(num_envs=N, num_steps=T, num_minibatches=NMB, update_epochs=EPOCHS,
                total_timesteps=N * T * ITERS, save_model=False, seed=3, ent_coef=0.01)
    base.update(kw)
    return contppo.finalize(contppo.ContPPOArgs(**base))


def _run(dev, fused=True, graphs=True, stub=False, iters=ITERS, start_from=None, **kw):
    """`iters` iterations; per iteration the rollout's buffers and the parameters after its
    update. start_from: another run; each iteration then starts from that run's parameters, so
    its rollout can be compared bitwise however the previous updates rounded."""
    from oc_cleanrl_amd import contppo

    old = contppo.FUSED_CONT
    contppo.FUSED_CONT = fused
    try:
        env = StubEnv(N, dev) if stub else None
        tr = contppo.ContPPOTrainer(_args(contppo, cuda_graphs=graphs, **kw), dev, log=False,
                                    device_env=env)
        c = lambda t: t.detach().cpu().clone()  # noqa: E731
        out = dict(its=[], tr=tr, sd0={k: c(v) for k, v in tr.agent.state_dict().items()})
        for i in range(iters):
            if start_from is not None and i > 0:
                tr.agent.load_state_dict(start_from["its"][i - 1]["sd"])
            m = tr.train_iteration()
            torch.cuda.synchronize()
            out["its"].append(dict(
                obs=c(tr.obs), actions=c(tr.cont_actions), z=c(tr.z), logprobs=c(tr.logprobs),
                values=c(tr.values), rewards=c(tr.rewards), dones=c(tr.dones),
                advantages=c(tr.advantages), returns=c(tr.returns), perm=c(tr.perm_dev),
                mb_actions=c(tr.mb_actions), stats=c(tr.stats), metrics=m,
                sd={k: c(v) for k, v in tr.agent.state_dict().items()}))
        out["graphs_ready"] = tr.graphs_ready
        return out
    finally:
        contppo.FUSED_CONT = old


ROLLOUT_KEYS = ("obs", "actions", "z", "logprobs", "values", "rewards", "dones", "advantages",
                "returns", "perm", "mb_actions")


_RUNS: dict = {}


def _runs(dev, stub: bool) -> dict:
    """The three runs of one env kind (made once): fused + graphs, fused eager, the torch path."""
    if stub not in _RUNS:
        base = _run(dev, stub=stub)
        _RUNS[stub] = dict(stub=stub, base=base, eager=_run(dev, graphs=False, stub=stub),
                           torch_path=_run(dev, fused=False, graphs=False, stub=stub, iters=2,
                                           start_from=base))
    return _RUNS[stub]


ENVS = pytest.mark.parametrize("stub", [False, True], ids=["pendulum", "stub_A3"])


@ENVS
def test_fused_against_the_torch_path(dev, stub):
    """Two iterations from the same seed and permutation: the rollouts (actions, log-probs,
    values, the env's outputs, GAE, the gathered action rows) are bitwise equal; the parameters
    after each iteration's four updates agree to 1 % of an Adam step (the bound of the config-2
    update fixture: sums in another order, carried through the steps)."""
    runs = _runs(dev, stub)
    base, tp = runs["base"], runs["torch_path"]
    A = base["tr"].A
    assert A == (3 if runs["stub"] else 1)
    assert base["its"][0]["actions"].shape == (T, N, A)
    for i in range(2):
        a, b = base["its"][i], tp["its"][i]
        for k in ROLLOUT_KEYS:
            assert torch.equal(a[k], b[k]), (i, k)
        assert float(a["actions"].abs().max()) > 0 and torch.isfinite(a["logprobs"]).all()
        # the gathered rows are the permutation's rows of the action buffer
        assert torch.equal(a["mb_actions"], a["actions"].view(T * N, A)[a["perm"]])
        worst = 0.0
        for k, v in a["sd"].items():
            torch.testing.assert_close(v, b["sd"][k], rtol=0, atol=0.01 * LR)
            worst = max(worst, float((v - b["sd"][k]).abs().max()))
        print(f"iteration {i}: max parameter difference {worst:.3g} (bound {0.01 * LR:.3g})")
    assert not torch.equal(base["its"][0]["sd"]["actor_logstd"], base["sd0"]["actor_logstd"])
    assert not torch.equal(base["its"][0]["sd"]["actor_mean.4.weight"],
                           base["sd0"]["actor_mean.4.weight"])


@ENVS
def test_torch_path_without_resync_after_two_iterations(dev, stub):
    """The torch path left alone for two iterations (no parameters carried over from the fused
    run): the drift of the first iteration's rounding through the second rollout and its four
    updates stays within 1 % of an Adam step."""
    base = _runs(dev, stub)["base"]
    tp = _run(dev, fused=False, graphs=False, stub=stub, iters=2)
    worst = 0.0
    for k, v in base["its"][1]["sd"].items():
        worst = max(worst, float((v - tp["its"][1]["sd"][k]).abs().max()))
    print(f"max parameter difference after two iterations {worst:.3g} (bound {0.01 * LR:.3g})")
    assert worst <= 0.01 * LR


def test_env_gets_the_args_gamma_and_trainers_do_not_share_a_stream(dev):
    from oc_cleanrl_amd import contppo, envs

    a = contppo.ContPPOTrainer(_args(contppo, gamma=0.9), dev, log=False)
    assert isinstance(a.env, envs.PendulumVecEnv) and a.env.gamma == 0.9
    assert envs.make_device_env("Pendulum-v1", "obj", 2, 0, 1, dev, 1, gamma=0.5).gamma == 0.5
    # a second trainer built in between neither reseeds nor consumes the first one's draws
    a.train_iteration()
    contppo.ContPPOTrainer(_args(contppo, seed=9), dev, log=False).train_iteration()
    a.train_iteration()
    b = contppo.ContPPOTrainer(_args(contppo, gamma=0.9), dev, log=False)
    b.train_iteration()
    b.train_iteration()
    assert torch.equal(a.z, b.z) and torch.equal(a.cont_actions, b.cont_actions)
    with pytest.raises(NotImplementedError, match="lagged"):
        a.train_iteration(lag=True)


@ENVS
def test_graphs_against_eager(dev, stub):
    runs = _runs(dev, stub)
    base, eager = runs["base"], runs["eager"]
    assert base["graphs_ready"] and not eager["graphs_ready"]
    for i in range(ITERS):
        a, b = base["its"][i], eager["its"][i]
        for k in ROLLOUT_KEYS + ("stats",):
            assert torch.equal(a[k], b[k]), (i, k)
        for k, v in a["sd"].items():
            assert torch.equal(v, b["sd"][k]), (i, k)


def test_torch_path_is_capturable(dev):
    """FUSED_CONT off under hipGraphs (what tools/contppo_rate.py times as the baseline): bitwise
    the eager torch path."""
    a, b = _run(dev, fused=False), _run(dev, fused=False, graphs=False)
    assert a["graphs_ready"]
    for i in range(ITERS):
        for k, v in a["its"][i]["sd"].items():
            assert torch.equal(v, b["its"][i]["sd"][k]), (i, k)


def test_metrics_carry_the_scripts_names(dev):
    m = _runs(dev, False)["base"]["its"][-1]["metrics"]
    for k in ("charts/learning_rate", "losses/value_loss", "losses/policy_loss", "losses/entropy",
              "losses/old_approx_kl", "losses/approx_kl", "losses/clipfrac",
              "losses/explained_variance"):
        assert k in m and np.isfinite(m[k]), k
    assert not any("Episodic" in k for k in m)


def test_rpo_changes_the_update_and_alpha_zero_is_contppo(dev):
    from oc_cleanrl_amd import rpo

    base = _runs(dev, False)["base"]
    d = dict(rpo.RPO_DEFAULTS, total_timesteps=N * T * ITERS)
    noisy = _run(dev, **d)
    zero = _run(dev, **dict(d, rpo_alpha=0.0))
    for i in range(ITERS):
        for k, v in base["its"][i]["sd"].items():
            assert torch.equal(v, zero["its"][i]["sd"][k]), (i, k)
    # the first rollout is the same; the update is not
    assert torch.equal(noisy["its"][0]["actions"], base["its"][0]["actions"])
    assert not torch.equal(noisy["its"][0]["sd"]["actor_mean.4.weight"],
                           base["its"][0]["sd"]["actor_mean.4.weight"])
    # the counter advanced once per iteration (the update graphs read it on the device)
    assert int(noisy["tr"].rpo_counter) == ITERS
    # the torch path adds exactly ops.rpo_noise's draws
    tp = _run(dev, fused=False, graphs=False, iters=1, **d)
    for k, v in noisy["its"][0]["sd"].items():
        torch.testing.assert_close(v, tp["its"][0]["sd"][k], rtol=0, atol=0.01 * LR)
