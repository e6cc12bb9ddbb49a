"""TD3 / DDPG without a GPU: the Args and state-dict surface against the scripts' fixtures, the
plain-torch update of the package's modules against the f64 fixtures (DESIGN 11's rule), the
NumPy twins of the streams, every refusal and the step-counting schedule."""
import dataclasses
import json

import numpy as np
import pytest
import torch

import td3_util as U
from conftest import ROOT
from oc_cleanrl_amd import ddpg, td3

GOLD = ROOT / "tests" / "golden"
OWN = ("backend", "cuda_graphs", "log_dir", "log_every", "save_model")


def _json(name):
    return json.loads((GOLD / name).read_text())


# ---- surface ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,fixture", [(td3.TD3Args, "td3_args_fields.json"),
                                         (ddpg.DDPGArgs, "ddpg_args_fields.json")])
def test_args_fields_and_defaults_match_the_script(cls, fixture):
    ref = _json(fixture)
    fields = {f.name: f.default for f in dataclasses.fields(cls)}
    names = [f.name for f in dataclasses.fields(cls)]
    assert names[:len(ref)] == list(ref), "the script's fields first, in its order"
    for k, v in ref.items():
        if k == "env_id":  # declared: Hopper-v4 needs MuJoCo
            assert (v, fields[k]) == ("Hopper-v4", "Pendulum-v1")
        else:
            assert fields[k] == v and type(fields[k]) is type(v), k
    assert isinstance(fields["learning_starts"], float)  # the script's 25e3, kept
    for k in OWN:
        assert k in fields
    assert cls().train_frequency == cls().policy_frequency == 2
    assert (td3.TD3Args.twin, ddpg.DDPGArgs.twin, ddpg.DDPGArgs.policy_noise) == (True, False, 0.0)
    assert "policy_noise" not in {f.name for f in dataclasses.fields(ddpg.DDPGArgs)}


def test_state_keys_shapes_and_construction_order():
    ref = _json("td3_state_keys.json")
    spec = td3.box_spec(3, [-2.0], [2.0])
    for name, cls in (("Actor", td3.Actor), ("QNetwork", td3.QNetwork)):
        sd = cls(spec).state_dict()
        assert list(sd) == list(ref[name])
        assert {k: list(v.shape) for k, v in sd.items()} == ref[name]
    spec = td3.box_spec(5, *U.BOUNDS[6])
    ac = td3.Actor(spec)
    lo, hi = (np.asarray(v, np.float32) for v in U.BOUNDS[6])
    assert np.array_equal(ac.action_scale.numpy(), (hi - lo) / 2.0)
    assert np.array_equal(ac.action_bias.numpy(), (hi + lo) / 2.0)
    # the script's order (:178-186): actor, qf1, qf2, then the three targets, which consume the
    # generator before being overwritten
    for twin in (True, False):
        torch.manual_seed(3)
        actor, q, target_actor, q_target = td3.make_networks(spec, twin)
        torch.manual_seed(3)
        want = [td3.Actor(spec), td3.QNetwork(spec)] + ([td3.QNetwork(spec)] if twin else [])
        got = [actor, q.qf1] + ([q.qf2] if twin else [])
        for g, w in zip(got, want):
            for (k, a), (_, b) in zip(g.state_dict().items(), w.state_dict().items()):
                assert torch.equal(a, b), k
        for t, o in ((target_actor, actor), (q_target, q)):
            for a, b in zip(t.state_dict().values(), o.state_dict().values()):
                assert torch.equal(a, b)
        assert [k for k, _ in q.named_parameters()][:2] == ["qf1.fc1.weight", "qf1.fc1.bias"]
        assert hasattr(q, "qf2") is twin


def test_generator_position_after_construction():
    """make_networks leaves the generator where the script's six (four) constructions do."""
    spec = td3.box_spec(3, [-2.0], [2.0])
    for twin in (True, False):
        torch.manual_seed(11)
        td3.make_networks(spec, twin)
        got = torch.rand(4)
        torch.manual_seed(11)
        td3.Actor(spec)
        for _ in range(4 if twin else 2):
            td3.QNetwork(spec)
        td3.Actor(spec)
        assert torch.equal(got, torch.rand(4))


# ---- the update against the fixtures -----------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["td3", "ddpg"])
@pytest.mark.parametrize("case", U.CASES, ids=lambda c: "B%d_A%d_D%d" % c)
def test_plain_torch_update_against_the_f64_fixture(algo, case):
    B, A, D = case
    twin = algo == "td3"
    fx = np.load(GOLD / U.fixture_name(algo, B, A))
    nets, t = U.package_networks(B, A, D, twin), U.stub_batch(B, A, D)
    U.assert_branches(t, nets, twin)
    got = U.update_ref(nets, t, torch.float32, twin)
    got64 = U.update_ref(nets, t, torch.float64, twin)
    for k in U.FIXTURE_KEYS:
        if k == "dq2" and not twin:
            assert "f64_dq2" not in fx.files
            continue
        U.check(f"{algo} {k}", got[k], fx["f32_" + k], fx["f64_" + k])
        # the f64 restatement is the fixture's f64 run to f64 rounding
        assert U.rel_err(got64[k], fx["f64_" + k]) < 1e-12, k


def test_fixture_sizes():
    for algo in ("td3", "ddpg"):
        for B, A, _ in U.CASES:
            assert (GOLD / U.fixture_name(algo, B, A)).stat().st_size < 1_500_000


# ---- the streams' twins ----------------------------------------------------------------------------------
def test_replay_index_twin_law():
    idx = U.replay_indices_ref(7, 3, 4096, pos=5, full=False, size=16, E=3)
    assert idx[:, 0].min() == 0 and idx[:, 0].max() == 4 and set(idx[:, 1]) == {0, 1, 2}
    full = U.replay_indices_ref(7, 3, 4096, pos=5, full=True, size=16, E=3)
    assert full[:, 0].min() == 0 and full[:, 0].max() == 15
    assert (U.replay_indices_ref(7, 0, 8, 0, False, 16, 2)[:, 0] == 0).all()
    assert not np.array_equal(idx, U.replay_indices_ref(7, 4, 4096, 5, False, 16, 3))
    assert abs(np.bincount(full[:, 0], minlength=16) / 4096 - 1 / 16).max() < 5 * (1 / 16 / 4096) ** 0.5


def test_philox_known_answer_and_box_muller():
    # Random123's known-answer vectors for philox4x32-10
    assert U.philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert U.philox4x32_10([M := 0xFFFFFFFF, M, M, M], [M, M]) == \
        [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    kat = np.array([[[0x6627E8D5, 0xE169C58D]], [[0x408F276D, 0x41C83B0E]]], np.uint64)
    z32, z64 = U.box_muller(kat, np.float32), U.box_muller(kat, np.float64)
    for w, z in zip(kat[:, 0], z64[:, 0]):
        u1, u2 = ((int(w[0]) >> 8) + 1) * 2.0 ** -24, (int(w[1]) >> 8) * 2.0 ** -24
        assert z == np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)
    assert z32.dtype == np.float32 and U.rel_err(z32, z64) <= U.bound(0.0)
    # the extreme words: u1 = 1 gives 0, u1 = 2^-24 the largest draw, all finite
    ext = np.array([[[0xFFFFFFFF, 0]], [[0, 0]], [[0, 0x80000000]]], np.uint64)
    z = U.box_muller(ext, np.float32)[:, 0]
    assert z[0] == 0 and np.isfinite(z).all() and abs(z[1] - np.sqrt(2 * 24 * np.log(2))) < 1e-5
    assert abs(z[2] + z[1]) < 1e-5
    w = U.act_words(1, 9, 2, 3)
    assert w.shape == (2, 3, 2) and not np.array_equal(w, U.act_words(1, 10, 2, 3))
    assert not np.array_equal(w, U.target_words(1, 9, 2, 3))


# ---- refusals ------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_device_work():
    class Wide:
        n_actions = 65

    dev = "cpu"  # nothing may touch the device: a CPU "device" would fail later, not here
    with pytest.raises(NotImplementedError, match="Synthetic"):
        td3.TD3Trainer(td3.TD3Args(backend="MuJoCo"), dev)
    with pytest.raises(NotImplementedError, match="Pendulum-v1"):
        td3.TD3Trainer(td3.TD3Args(env_id="Hopper-v4"), dev)
    with pytest.raises(NotImplementedError, match="Pendulum-v1"):
        td3.TD3Trainer(ddpg.DDPGArgs(env_id="Hopper-v4"), dev)
    with pytest.raises(ValueError, match="at most 64"):
        td3.TD3Trainer(td3.TD3Args(), dev, device_env=Wide())
    with pytest.raises(ValueError, match="policy_frequency"):
        td3.TD3Trainer(td3.TD3Args(policy_frequency=0), dev)
    with pytest.raises(ValueError, match="batch_size"):
        td3.TD3Trainer(td3.TD3Args(batch_size=0), dev)
    with pytest.raises(ValueError, match="bounds"):
        td3.box_spec(3, [1.0], [1.0])
    with pytest.raises(ValueError, match="multiple of 64"):
        td3.act_mu(torch.zeros(1, 100), torch.zeros(1, 100), torch.zeros(1))


# ---- the schedule ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ls", [0, 3, 4])
@pytest.mark.parametrize("pf", [1, 2, 3])
def test_schedule_is_the_scripts_three_conditions(ls, pf, monkeypatch):
    """Which steps act at random, train and update the policy, eagerly and chunked, against a
    direct transcription of :205, :236, :262 (the trainer's loop with its device work recorded
    instead of run)."""
    want = []
    for global_step in range(12):
        want.append((global_step < ls, global_step > ls,
                     global_step > ls and global_step % pf == 0))
        assert td3.train_schedule(global_step, ls, pf) == want[-1]

    class Env:
        def advance(self, n):
            pass

    class Step:
        def add_(self, n):
            pass

    for graphs in (False, True):
        tr = object.__new__(td3.TD3Trainer)
        tr.args = td3.TD3Args(learning_starts=float(ls), policy_frequency=pf, cuda_graphs=graphs)
        tr.learning_starts, tr.global_step, tr.env, tr.step_dev = ls, 0, Env(), Step()
        log, kinds = [], []
        tr._env_step = lambda k: log.append([len(log) < ls, False, False])
        tr._train_step = lambda policy: log[-1].__setitem__(slice(1, 3), [True, policy])
        if graphs:  # the chunk kinds, without capturing
            def run_chunk(base, tr=tr):
                kinds.append("fill" if base + pf - 1 <= ls else "train" if base > ls else "eager")
                tr._chunk(base)
            tr._run_chunk = run_chunk
        n = 12 - 12 % pf
        tr.steps(n)
        assert [tuple(r) for r in log] == want[:n] and tr.global_step == n
        if graphs:
            if pf > 1:
                with pytest.raises(ValueError, match="multiple"):
                    tr.steps(pf + 1)
            # at most one chunk is neither all-fill nor all-train, and it holds learning_starts
            assert kinds.count("eager") <= 1
            for i, kind in enumerate(kinds):
                rows = want[i * pf:(i + 1) * pf]
                assert kind != "fill" or not any(r[1] for r in rows)
                assert kind != "train" or (all(r[1] for r in rows) and rows[0][2]
                                           and not any(r[2] for r in rows[1:]))
                assert kind != "eager" or i * pf <= ls < (i + 1) * pf
