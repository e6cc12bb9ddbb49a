"""Continuous SAC without a GPU: the Args and state-dict surface against the script's fixtures, the
plain-torch update of the package's modules against the f64 fixtures (DESIGN 11's rule), the NumPy
twins of the streams, torch.min's tie rule, every refusal and the step-counting schedule."""
import dataclasses
import json
import math

import numpy as np
import pytest
import torch

import sac_continuous_util as U
from conftest import ROOT
from oc_cleanrl_amd import sac_continuous as sc

GOLD = ROOT / "tests" / "golden"
OWN = ("backend", "cuda_graphs", "log_dir", "log_every")


def _json(name):
    return json.loads((GOLD / name).read_text())


# ---- surface ---------------------------------------------------------------------------------------------
def test_args_fields_and_defaults_match_the_script():
    ref = _json("sac_continuous_args_fields.json")
    fields = {f.name: f.default for f in dataclasses.fields(sc.ContSACArgs)}
    names = list(fields)
    assert names[:len(ref)] == list(ref), "the script's fields first, in its order"
    for k, v in ref.items():
        if k == "env_id":  # declared: Hopper-v4 needs MuJoCo
            assert (v, fields[k]) == ("Hopper-v4", "Pendulum-v1")
        else:
            assert fields[k] == v and type(fields[k]) is type(v), k
    assert isinstance(fields["learning_starts"], float) and fields["learning_starts"] == 5e3
    for k in OWN:
        assert k in fields
    assert sc.ContSACArgs().train_frequency == 2
    assert sc.ContSACArgs(policy_frequency=3, target_network_frequency=2).train_frequency == 6
    assert (sc.LOG_STD_MIN, sc.LOG_STD_MAX) == (-5, 2)


def test_state_keys_shapes_and_construction_order():
    ref = _json("sac_continuous_state_keys.json")
    spec = sc.box_spec(3, [-2.0], [2.0])
    for name, cls in (("Actor", sc.Actor), ("SoftQNetwork", sc.QNetwork)):
        sd = cls(spec).state_dict()
        assert list(sd) == list(ref[name])
        assert {k: list(v.shape) for k, v in sd.items()} == ref[name]
    spec = sc.box_spec(5, *U.BOUNDS[6])
    lo, hi = (np.asarray(v, np.float32) for v in U.BOUNDS[6])
    ac = sc.Actor(spec)
    assert np.array_equal(ac.action_scale.numpy(), (hi - lo) / 2.0)
    assert np.array_equal(ac.action_bias.numpy(), (hi + lo) / 2.0)
    # the script's order (:199-205): actor, qf1, qf2, then the two targets, which consume the
    # generator before being overwritten; no target actor
    torch.manual_seed(3)
    actor, q, q_target = sc.make_networks(spec)
    after = torch.rand(4)
    torch.manual_seed(3)
    want = [sc.Actor(spec), sc.QNetwork(spec), sc.QNetwork(spec)]
    sc.QNetwork(spec), sc.QNetwork(spec)
    assert torch.equal(after, torch.rand(4))
    for g, w in zip([actor, q.qf1, q.qf2], want):
        assert [tuple(v.shape) for v in g.state_dict().values()] == \
            [tuple(v.shape) for v in w.state_dict().values()]
        for (k, a), (_, b) in zip(g.state_dict().items(), w.state_dict().items()):
            assert torch.equal(a, b), k
    for a, b in zip(q_target.state_dict().values(), q.state_dict().values()):
        assert torch.equal(a, b)
    assert [k for k, _ in q.named_parameters()][:2] == ["qf1.fc1.weight", "qf1.fc1.bias"]


def test_actor_forward_and_get_action_are_the_scripts():
    spec = sc.box_spec(5, *U.BOUNDS[6])
    torch.manual_seed(0)
    ac = sc.Actor(spec)
    x = torch.randn(7, 5)
    mean, log_std = ac(x)
    m2, r = ac.heads(x)
    assert torch.equal(mean, m2) and torch.equal(log_std, -5 + 3.5 * (torch.tanh(r) + 1))
    assert float(log_std.detach().min()) >= -5 and float(log_std.detach().max()) <= 2
    torch.manual_seed(1)
    action, logp, mean_action = ac.get_action(x)
    torch.manual_seed(1)
    z = torch.randn(7, 6)  # Normal.rsample's eps
    a2, lp2 = sc.squash(m2, r, z, ac.action_scale, ac.action_bias)
    assert logp.shape == (7, 1) and torch.allclose(action, a2, atol=1e-6)
    assert torch.allclose(logp, lp2, atol=1e-4)
    assert torch.equal(mean_action, torch.tanh(mean) * ac.action_scale + ac.action_bias)


# ---- the update against the fixtures -----------------------------------------------------------------------
@pytest.mark.parametrize("case", U.CASES, ids=lambda c: "B%d_A%d_D%d" % c)
def test_plain_torch_update_against_the_f64_fixture(case):
    B, A, D = case
    fx = np.load(GOLD / U.fixture_name(B, A))
    nets, t = U.package_case(B, A, D)
    U.assert_branches(t, nets)
    got = U.update_ref(nets, t, torch.float32)
    assert set(got) == set(U.FIXTURE_KEYS)
    for k in U.FIXTURE_KEYS:
        U.check(k, got[k], fx["f32_" + k], fx["f64_" + k])
    # the f64 restatement (log_prob from z, 1 - y^2 from exp(-2 |x|)) is the script's f64 run far
    # below f32 rounding (the script's own 1 - y^2 cancels to ~1e-9 of its gradient past |x| = 12)
    got64 = U.update_ref(nets, t, torch.float64)
    for k in U.FIXTURE_KEYS:
        assert U.rel_err(got64[k], fx["f64_" + k]) < 1e-8, k


def test_fixture_sizes():
    for B, A, _ in U.CASES:
        assert (GOLD / U.fixture_name(B, A)).stat().st_size < 1_000_000


def test_min_backward_tie_rule():
    """What ocppo_csac_actor_loss_fwd_bwd restates: the smaller input takes the gradient, equal
    inputs take half each."""
    a = torch.tensor([1.0, 2.0, 3.0, -1.0], requires_grad=True)
    b = torch.tensor([2.0, 1.0, 3.0, -1.0], requires_grad=True)
    (-torch.min(a, b)).mean().backward()
    assert a.grad.tolist() == [-0.25, 0.0, -0.125, -0.125]
    assert b.grad.tolist() == [0.0, -0.25, -0.125, -0.125]


# ---- the streams' twins ----------------------------------------------------------------------------------
def test_stream_twins_moments_and_distinct_draws():
    n = 2 ** 16
    E, A = n // 64, 64
    w = U.act_words(3, 17, E, A)
    z = U.box_muller(w, np.float64).reshape(-1)
    u = U.unit24(w[..., 0], np.float64).reshape(-1)
    assert abs(z.mean()) < 5 / n ** 0.5 and abs(z.var() - 1) < 5 * (2 / n) ** 0.5
    assert abs(u.mean() - 0.5) < 5 * (1 / 12 / n) ** 0.5 and u.min() >= 0 and u.max() < 1
    B, A = n // 8, 8
    draws = [U.box_muller(U.update_words(3, 17, d, B, A), np.float64).reshape(-1)
             for d in (U.TARGET_DRAW, 1, 2)]
    for zd in draws:
        assert np.isfinite(zd).all()
        assert abs(zd.mean()) < 5 / n ** 0.5 and abs(zd.var() - 1) < 5 * (2 / n) ** 0.5
    # no two draws of a step coincide, nor the acting stream, nor the next counter
    assert not np.array_equal(draws[0], draws[1]) and not np.array_equal(draws[1], draws[2])
    w0 = U.update_words(3, 17, 1, 4, 3)
    assert not np.array_equal(w0, U.update_words(3, 18, 1, 4, 3))
    assert not np.array_equal(w0, U.act_words(3, 17, 4, 3))
    assert not np.array_equal(w0, U.update_words(4, 17, 1, 4, 3))
    # the counter's word: its low 32 bits
    assert np.array_equal(w0, U.update_words(3, 17 + 2 ** 32, 1, 4, 3))


# ---- refusals ------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_device_work():
    class Wide:
        n_actions = 65

    dev = "cpu"  # nothing may touch the device: a CPU "device" would fail later, not here
    T, Args = sc.ContSACTrainer, sc.ContSACArgs
    with pytest.raises(NotImplementedError, match="Synthetic"):
        T(Args(backend="MuJoCo"), dev)
    with pytest.raises(NotImplementedError, match="Pendulum-v1"):
        T(Args(env_id="Hopper-v4"), dev)
    with pytest.raises(ValueError, match="at most 64"):
        T(Args(), dev, device_env=Wide())
    with pytest.raises(ValueError, match="policy_frequency"):
        T(Args(policy_frequency=0), dev)
    with pytest.raises(ValueError, match="batch_size"):
        T(Args(batch_size=0), dev)
    with pytest.raises(ValueError, match="target_network_frequency"):
        T(Args(target_network_frequency=0), dev)


# ---- the schedule ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tnf", [1, 2])
@pytest.mark.parametrize("pf", [1, 2, 3])
@pytest.mark.parametrize("ls", [0, 3, 4])
def test_schedule_is_the_scripts_four_conditions(ls, pf, tnf):
    """Which steps act at random, train, run the actor / temperature block (policy_frequency
    iterations) and soft-update, eagerly and chunked, against a direct transcription of :233,
    :262, :282, :307 (the trainer's loop with its device work recorded instead of run)."""
    N = 24
    want = []
    for global_step in range(N):
        trains = global_step > ls
        want.append((global_step < ls, trains, pf if trains and global_step % pf == 0 else 0,
                     trains and global_step % tnf == 0))
        assert sc.train_schedule(global_step, ls, pf, tnf) == \
            (want[-1][0], trains, want[-1][2] > 0, want[-1][3])
    chunk = math.lcm(pf, tnf)
    assert sc.chunk_length(pf, tnf) == chunk

    class Env:
        def advance(self, n):
            pass

    class Step:
        def add_(self, n):
            pass

    class Replay:
        def sample(self, n, out=None):
            return {}

    for graphs in (False, True):
        tr = object.__new__(sc.ContSACTrainer)
        tr.args = sc.ContSACArgs(learning_starts=float(ls), policy_frequency=pf,
                                 target_network_frequency=tnf, cuda_graphs=graphs)
        tr.learning_starts, tr.global_step, tr.env, tr.step_dev = ls, 0, Env(), Step()
        tr.rb, tr.batch = Replay(), None
        assert tr.chunk_len == chunk
        log, kinds = [], []
        tr._env_step = lambda k: log.append([len(log) < ls, False, 0, False])
        tr.update_critics = lambda d: log[-1].__setitem__(1, True)
        tr.update_policy = lambda d, i: (log[-1].__setitem__(2, log[-1][2] + 1),
                                         pytest.fail("order") if i != log[-1][2] - 1 else None)
        tr._target_update = lambda: log[-1].__setitem__(3, True)
        if graphs:  # the chunk kinds, without capturing
            def run_chunk(base, tr=tr):
                kinds.append("fill" if base + chunk - 1 <= ls else "train" if base > ls
                             else "eager")
                tr._chunk(base)
            tr._run_chunk = run_chunk
        n = N - N % chunk
        tr.steps(n)
        assert [tuple(r) for r in log] == want[:n] and tr.global_step == n
        if graphs:
            if chunk > 1:
                with pytest.raises(ValueError, match="multiple"):
                    tr.steps(chunk + 1)
            # at most one chunk is neither all-fill nor all-train, and it holds learning_starts;
            # every train chunk has the same schedule (one graph serves them all)
            assert kinds.count("eager") <= 1
            train_rows = set()
            for i, kind in enumerate(kinds):
                rows = want[i * chunk:(i + 1) * chunk]
                assert kind != "fill" or not any(r[1] for r in rows)
                assert kind != "eager" or i * chunk <= ls < (i + 1) * chunk
                if kind == "train":
                    assert all(r[1] for r in rows)
                    train_rows.add(tuple(rows))
            assert len(train_rows) == 1
