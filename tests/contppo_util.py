"""The steps of cleanrl/ppo_continuous_action.py / rpo_continuous_action.py the continuous-action
kernels restate, in plain torch / NumPy. Dtype-generic where it matters: run on float64 copies of
f32 inputs they are the float64 twin; run in float32 they are "torch's own computation", whose
error sets the bound (lstm_util.check).

  * loss_ref: the update lines :265-300 from the network outputs on, by autograd;
  * loss_case: seeded minibatches whose ratios, value differences and advantages sit where the
    clip branches need them (asserted here, on the CPU);
  * NormChainRef: the wrapper chain of :96-100 per env, the spec of ops.env_normalize (gymnasium
    0.28.1's semantics as recalled: gymnasium is not installed);
  * pendulum_*_ref: Pendulum-v1's step and the reset stream, the spec of ops.pendulum_step;
  * rpo_noise_ref: the RPO noise stream (Philox4x32-10) in Python integers.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch
from torch.distributions.normal import Normal

from lstm_util import check, rel_err  # noqa: F401  (re-exported for the tests)
from rnd_util import MASK64, splitmix64, unit53

STAT_NAMES = ("loss", "pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac",
              "adv_mean", "adv_std")
CLIP = 0.2
# a row's log-ratio / value-difference targets: both sides of both clip bounds, in any four rows
LOGRATIO_CYCLE = (-0.5, -0.1, 0.1, 0.5)   # ratios 0.61, 0.90, 1.11, 1.65 against 0.8 / 1.2
VDIFF_CYCLE = (-0.5, -0.05, 0.05, 0.5)    # against -0.2 / 0.2
NEAR = 1e-4


def cfg(norm_adv=True, clip_vloss=True, ent_coef=0.0, vf_coef=0.5, clip_coef=CLIP):
    return SimpleNamespace(norm_adv=norm_adv, clip_vloss=clip_vloss, ent_coef=ent_coef,
                           vf_coef=vf_coef, clip_coef=clip_coef)


# ---- the update lines ------------------------------------------------------------------------------
def loss_ref(t: dict, a, dtype, noise=None) -> dict:
    """:265-300 on the tensors t (mean [M, A], logstd [A], newvalue [M], actions [M, A],
    logprobs, advantages, returns, values [M]) cast to `dtype`, with loss.backward(): stats [9] in
    STAT_NAMES' layout, dmean, dvalue, dlogstd. noise [M, A]: RPO's, added to the mean."""
    c = lambda v: torch.as_tensor(v).detach().cpu().to(dtype)  # noqa: E731
    mean, value = c(t["mean"]).requires_grad_(), c(t["newvalue"]).requires_grad_()
    logstd = c(t["logstd"]).view(1, -1).requires_grad_()
    mu = mean if noise is None else mean + c(noise)
    probs = Normal(mu, torch.exp(logstd.expand_as(mean)))
    newlogprob = probs.log_prob(c(t["actions"])).sum(1)
    entropy = probs.entropy().sum(1)
    logratio = newlogprob - c(t["logprobs"])
    ratio = logratio.exp()
    old_approx_kl = (-logratio).mean()
    approx_kl = ((ratio - 1) - logratio).mean()
    clipfrac = ((ratio - 1.0).abs() > a.clip_coef).to(dtype).mean()
    adv = c(t["advantages"])
    adv_mean = adv_std = torch.zeros((), dtype=dtype)
    if a.norm_adv:
        adv_mean, adv_std = adv.mean(), adv.std()
        adv = (adv - adv_mean) / (adv_std + 1e-8)
    pg_loss = torch.max(-adv * ratio,
                        -adv * torch.clamp(ratio, 1 - a.clip_coef, 1 + a.clip_coef)).mean()
    ret, val = c(t["returns"]), c(t["values"])
    if a.clip_vloss:
        v_clipped = val + torch.clamp(value - val, -a.clip_coef, a.clip_coef)
        v_loss = 0.5 * torch.max((value - ret) ** 2, (v_clipped - ret) ** 2).mean()
    else:
        v_loss = 0.5 * ((value - ret) ** 2).mean()
    entropy_loss = entropy.mean()
    loss = pg_loss - a.ent_coef * entropy_loss + v_loss * a.vf_coef
    loss.backward()
    stats = torch.stack([loss, pg_loss, v_loss, entropy_loss, old_approx_kl, approx_kl, clipfrac,
                         adv_mean, adv_std]).detach()
    return dict(stats=stats, dmean=mean.grad, dvalue=value.grad, dlogstd=logstd.grad.view(-1),
                ratio=ratio.detach(), vdiff=(value - val).detach())


def new_logprob64(t: dict, noise=None):
    mean = torch.as_tensor(t["mean"]).double()
    if noise is not None:
        mean = mean + torch.as_tensor(noise).double()
    std = torch.exp(torch.as_tensor(t["logstd"]).double().view(1, -1).expand_as(mean))
    return Normal(mean, std).log_prob(torch.as_tensor(t["actions"]).double()).sum(1)


def shape_rows(t: dict, seed: int, noise=None) -> dict:
    """Set a case's old log-probs, old values and one zero advantage so that row m's ratio and
    value difference follow the two cycles (with a seeded jitter that keeps them off the
    bounds)."""
    M = t["mean"].shape[0]
    g = torch.Generator().manual_seed(seed + 77)
    m = torch.arange(M)
    lr = torch.tensor(LOGRATIO_CYCLE, dtype=torch.float64)[m % 4] + \
        0.03 * (2 * torch.rand(M, generator=g, dtype=torch.float64) - 1)
    vd = torch.tensor(VDIFF_CYCLE, dtype=torch.float64)[(3 * m + 1) % 4] + \
        0.02 * (2 * torch.rand(M, generator=g, dtype=torch.float64) - 1)
    t["logprobs"] = (new_logprob64(t, noise) - lr).float()
    t["values"] = (t["newvalue"].double() - vd).float()
    if M > 2:
        t["advantages"][2] = 0.0
    return t


def assert_branches(t: dict, a, noise=None, full: bool = True):
    """The conditions a loss case must meet, on the f32 torch reference: no ratio or value
    difference within NEAR (relative) of a clip bound; with `full` (M >= 4), ratios on both sides
    of both bounds, value differences on both sides of +-clip, and a zero-advantage row."""
    r = loss_ref(t, a, torch.float32, noise)
    ratio, vd, c = r["ratio"].double(), r["vdiff"].double(), a.clip_coef
    for b in (1 - c, 1 + c):
        assert float(((ratio - b).abs() / b).min()) > NEAR, "a ratio sits on a clip bound"
    for b in (-c, c):
        assert float(((vd - b).abs() / c).min()) > NEAR, "a value difference sits on a clip bound"
    if not full:
        return
    assert (ratio < 1 - c).any() and ((ratio > 1 - c) & (ratio < 1 + c)).any() and \
        (ratio > 1 + c).any()
    assert (vd < -c).any() and ((vd > -c) & (vd < c)).any() and (vd > c).any()
    assert (torch.as_tensor(t["advantages"]) == 0).any()


def loss_case(M: int, A: int, seed: int, noise=None) -> dict:
    """A seeded minibatch of f32 CPU tensors for the Gaussian loss."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = {"mean": 0.5 * rn(M, A), "logstd": -1.0 + 1.5 * torch.rand(A, generator=g),
         "newvalue": rn(M), "advantages": rn(M), "returns": rn(M)}
    t["actions"] = t["mean"] + torch.exp(t["logstd"]) * rn(M, A) + 0.1 * rn(M, A)
    return shape_rows(t, seed, noise)


# ---- the update fixtures (tests/golden/gen_golden_contppo.py) --------------------------------------
TERMS = ("loss", "pg_loss", "v_loss", "entropy_loss", "old_approx_kl", "approx_kl", "clipfrac")


def stub_parameters(agent, seed: int):
    """Overwrite the agent's parameters in state-dict order with a seeded CPU generator's draws
    (the same bits on any machine): randn * 0.3 / sqrt(fan-in), actor_logstd in [-1, 0.5)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in agent.state_dict().items():
            if k == "actor_logstd":
                p.copy_(-1.0 + 1.5 * torch.rand(p.shape, generator=g))
            else:
                p.copy_(0.3 * torch.randn(p.shape, generator=g) / max(p.shape[-1], 1) ** 0.5)
    return agent


def flat_grads(grads):
    """Gradients (in parameter order) as one flat vector."""
    return np.concatenate([np.asarray(g).reshape(-1) for g in grads])


def split_grads(flat, agent) -> dict:
    """A fixture's flat gradient vector as {parameter name: array} for `agent`."""
    out, pos = {}, 0
    for k, p in agent.named_parameters():
        out[k] = flat[pos:pos + p.numel()].reshape(tuple(p.shape))
        pos += p.numel()
    assert pos == flat.size
    return out


def load_update(fx: dict):
    """A fixture's arrays as (t, a, out): the minibatch tensors (with the f32 network outputs as
    mean / newvalue and the stub parameters' logstd), the hyper-parameters, and per dtype the
    terms and the heads' gradients."""
    M, A = fx["actions"].shape
    tt = torch.from_numpy
    t = {"obs": tt(fx["obs"]), "actions": tt(fx["actions"])}
    t.update({k: tt(fx["batch"][i]) for i, k in enumerate(("logprobs", "advantages", "returns",
                                                           "values"))})
    h = fx["hyper"]
    a = cfg(bool(h[3]), bool(h[4]), float(h[1]), float(h[2]), float(h[0]))
    out = {}
    for tag in ("f32", "f64"):
        v = fx[tag + "_heads"]
        out[tag] = dict(zip(TERMS, fx[tag + "_terms"]), mean=v[:M * A].reshape(M, A),
                        newvalue=v[M * A:M * A + M], dmean=v[M * A + M:2 * M * A + M].reshape(M, A),
                        dvalue=v[2 * M * A + M:])
    t["mean"], t["newvalue"] = tt(out["f32"]["mean"]), tt(out["f32"]["newvalue"])
    return t, a, out


def fixture_agent(fx: dict):
    """ContAgent with the fixture's stub parameters (the generator's seed 1000 M + A)."""
    from oc_cleanrl_amd import contppo

    M, A = fx["actions"].shape
    return stub_parameters(contppo.ContAgent(contppo.cont_spec((fx["obs"].shape[1],), A)),
                           1000 * M + A)


# ---- the RPO noise stream ------------------------------------------------------------------------------
RPO_KEY = 0x3C6EF372FE94F82B
M32 = 0xFFFFFFFF


def philox4x32_10(c, k):
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def rpo_noise_ref(seed: int, counter: int, mb: int, M: int, A: int, alpha: float):
    """ops.rpo_noise's draws [M, A] f32: word 0 of the Philox block with key seed ^ RPO_KEY and
    counter (m * 64 + a, counter << 32 | mb); its top 24 bits as u in [-1, 1), times alpha."""
    key = (seed & MASK64) ^ RPO_KEY
    sub = ((counter << 32) | (mb & M32)) & MASK64
    out = np.empty((M, A), np.float32)
    al = np.float32(alpha)
    for m in range(M):
        for a in range(A):
            blk = m * 64 + a
            w = philox4x32_10([blk & M32, blk >> 32, sub & M32, sub >> 32],
                              [key & M32, key >> 32])[0]
            u = np.float32(np.float32(w >> 8) * np.float32(2.0 ** -23) - np.float32(1.0))
            out[m, a] = u * al
    return torch.from_numpy(out)


# ---- the wrapper chain (:96-100), per env -----------------------------------------------------------
class RunningMeanStd:
    """gym's RunningMeanStd in NumPy f64."""

    def __init__(self, shape=()):
        self.mean, self.var, self.count = np.zeros(shape), np.ones(shape), 1e-4

    def update(self, x):
        x = np.asarray(x, np.float64)
        bm, bv, bc = x.mean(0), x.var(0), x.shape[0]
        delta = bm - self.mean
        tot = self.count + bc
        new_mean = self.mean + delta * bc / tot
        m2 = self.var * self.count + bv * bc + np.square(delta) * self.count * bc / tot
        self.mean, self.var, self.count = new_mean, m2 / tot, tot


class NormChainRef:
    """N sub-envs' NormalizeObservation -> clip(+-10) -> NormalizeReward(gamma) -> clip(+-10), each
    with its own statistics (as each wrapped sub-env of the script's SyncVectorEnv has). A done
    step normalises the terminal observation first (the sub-env's step), then the reset
    observation (its reset): two statistics updates. The return accumulator is multiplied by
    (1 - terminated) only: a truncation leaves it (gymnasium 0.28.1)."""

    def __init__(self, N: int, D: int, gamma: float = 0.99, norm_obs=True, norm_reward=True,
                 eps: float = 1e-8):
        self.N, self.D, self.gamma, self.eps = N, D, gamma, eps
        self.norm_obs, self.norm_reward = norm_obs, norm_reward
        self.obs_rms = [RunningMeanStd((D,)) for _ in range(N)]
        self.ret_rms = [RunningMeanStd(()) for _ in range(N)]
        self.returns = np.zeros(N)

    def _obs(self, n, x):
        if not self.norm_obs:
            return np.asarray(x, np.float64)
        self.obs_rms[n].update(np.asarray(x, np.float64)[None])
        r = self.obs_rms[n]
        return np.clip((x - r.mean) / np.sqrt(r.var + self.eps), -10, 10)

    def reset(self, obs):
        return np.stack([self._obs(n, np.asarray(obs[n], np.float64)) for n in range(self.N)])

    def step(self, obs, final_obs, reward, terminated, truncated):
        """Raw f32 outputs of one vector step -> (obs [N, D], reward [N]) in f64."""
        o, r = np.zeros((self.N, self.D)), np.zeros(self.N)
        for n in range(self.N):
            if terminated[n] or truncated[n]:
                self._obs(n, np.asarray(final_obs[n], np.float64))
            rew = float(reward[n])
            if self.norm_reward:
                self.returns[n] = self.returns[n] * self.gamma * (1 - float(bool(terminated[n]))) + rew
                self.ret_rms[n].update(np.array([self.returns[n]]))
                rew = float(np.clip(rew / np.sqrt(self.ret_rms[n].var + self.eps), -10, 10))
            r[n] = rew
            o[n] = self._obs(n, np.asarray(obs[n], np.float64))
        return o, r

    def state(self):
        """ops.cont_norm_state's layout [N, 2D + 5]."""
        return np.stack([np.concatenate([
            self.obs_rms[n].mean, self.obs_rms[n].var, [self.obs_rms[n].count, self.returns[n],
                                                        self.ret_rms[n].mean, self.ret_rms[n].var,
                                                        self.ret_rms[n].count]])
            for n in range(self.N)])


# ---- Pendulum-v1 -----------------------------------------------------------------------------------------
def pendulum_step_ref(th: float, thdot: float, action: float):
    """pendulum.py step() behind ClipAction in Python floats: (th', thdot', reward)."""
    u = min(max(float(np.float32(action)), -2.0), 2.0)
    g, m, l, dt = 10.0, 1.0, 1.0, 0.05
    an = ((th + math.pi) % (2 * math.pi)) - math.pi
    costs = an ** 2 + 0.1 * thdot ** 2 + 0.001 * (u ** 2)
    newthdot = thdot + (3 * g / (2 * l) * math.sin(th) + 3.0 / (m * l ** 2) * u) * dt
    newthdot = min(max(newthdot, -8.0), 8.0)
    return th + newthdot * dt, newthdot, -costs


def pendulum_obs_ref(th, thdot):
    return np.array([math.cos(th), math.sin(th), thdot], np.float32)


def pendulum_reset_ref(seed: int, n: int, episode: int):
    """The reset draw of env n's episode: (theta in [-pi, pi), theta_dot in [-1, 1))."""
    key = splitmix64((splitmix64(seed & MASK64) + n * 0x100000001B3) & MASK64) ^ \
        splitmix64((episode + 0x632BE59BD9B4E019) & MASK64)
    u = [unit53(splitmix64((key + i) & MASK64)) for i in range(2)]
    return -math.pi + (math.pi - -math.pi) * u[0], -1.0 + (1.0 - -1.0) * u[1]
