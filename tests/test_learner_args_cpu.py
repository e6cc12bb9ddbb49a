"""The argument surface of the seven learners on trainer.PPOTrainer (lstm, transformer, pqn,
pqn_lstm, rnd, ppg, contppo) against tests/golden/onpolicy_args_surface.json: class name and doc,
the fields with their types and defaults in order, the class attributes that stand in for the
args.Args fields left off the command line, and what each module's finalize derives. Then the
shared entry points on a trainer without a device: how many iterations trainer.run drives (PPG:
whole phases) and what trainer.learner_main does around a run."""
from __future__ import annotations

import importlib.util
import json

import pytest

from conftest import GOLDEN


def _recorder():
    spec = importlib.util.spec_from_file_location("gen_onpolicy_args_surface",
                                                  GOLDEN / "gen_onpolicy_args_surface.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def got():
    return json.loads(json.dumps(_recorder().surface()))  # as the fixture went through JSON


@pytest.fixture(scope="module")
def want():
    return json.loads((GOLDEN / "onpolicy_args_surface.json").read_text())


def test_the_seven_learners_are_recorded(got, want):
    assert list(got) == list(want) == ["lstm", "transformer", "pqn", "pqn_lstm", "rnd", "ppg",
                                       "contppo"]


@pytest.mark.parametrize("learner", ["lstm", "transformer", "pqn", "pqn_lstm", "rnd", "ppg",
                                     "contppo"])
def test_surface_is_the_recorded_one(got, want, learner):
    g, w = got[learner], want[learner]
    assert list(g) == list(w)
    assert (g["name"], g["doc"]) == (w["name"], w["doc"])
    assert g["fields"] == w["fields"]  # names, types and defaults, in order
    assert g["class_attrs"] == w["class_attrs"]
    for key in list(w)[4:]:  # finalized_default, finalized_small (contppo: finalized_rpo)
        assert list(g[key].items()) == list(w[key].items()), key


class _Trainer:
    """What trainer.run and trainer.learner_main touch of a trainer, without a device."""

    def __init__(self, args, device, rank=0, world_size=1):
        self.args, self.device = args, device
        self.collected, self.global_step, self.closed = [], 0, False
        self.last_metrics = {"losses/value_loss": 0.123456789}

    def train_iteration(self, collect_metrics=True):
        self.collected.append(collect_metrics)
        return {}

    def close(self):
        self.closed = True


def test_run_drives_ppg_for_whole_phases_and_collects_on_the_last(tmp_path):
    from oc_cleanrl_amd import ppg
    from oc_cleanrl_amd.trainer import PPOTrainer, run

    class PPG(_Trainer):
        run_iterations = ppg.PPGTrainer.run_iterations

    class PPO(_Trainer):
        run_iterations = PPOTrainer.run_iterations

    args = ppg.finalize(ppg.PPGArgs(num_envs=6, num_steps=4, num_minibatches=3, n_iteration=2,
                                    num_aux_rollouts=3, total_timesteps=6 * 4 * 5,
                                    metrics_every=100, save_model=False, log_dir=str(tmp_path)))
    assert (args.num_iterations, args.num_phases) == (5, 2)
    assert run(args, "cpu", trainer_cls=PPG).collected == [False, False, False, True]
    assert run(args, "cpu", trainer_cls=PPO).collected == [False, False, False, False, True]


def test_learner_main_parses_finalizes_runs_prints_and_closes(monkeypatch, capsys):
    import torch

    from oc_cleanrl_amd import contppo, rpo
    from oc_cleanrl_amd.trainer import learner_main

    monkeypatch.setenv("LOCAL_RANK", "3")
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    tr = learner_main(contppo.ContPPOArgs, contppo.finalize, _Trainer, "rpo",
                      ["--num-envs", "4"], rpo.RPO_DEFAULTS)
    assert tr.device == torch.device("cuda:3") and tr.closed
    assert (tr.args.num_envs, tr.args.rpo_alpha, tr.args.batch_size) == (4, 0.5, 4 * 2048)
    assert capsys.readouterr().out.strip() == "{'losses/value_loss': 0.12346}"

    def fails(args, device):
        raise RuntimeError("no trainer")

    with pytest.raises(RuntimeError, match="no trainer"):
        learner_main(contppo.ContPPOArgs, contppo.finalize, fails, "rpo", [])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError, match="one GPU"):
        learner_main(contppo.ContPPOArgs, contppo.finalize, _Trainer, "rpo", [])
