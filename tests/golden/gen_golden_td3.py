"""Generate the TD3 / DDPG fixtures from the reference scripts (data only, no reference text):

    python tests/golden/gen_golden_td3.py /path/to/reference

  td3_args_fields.json / ddpg_args_fields.json   names and defaults of the scripts' Args, by AST
  td3_state_keys.json       keys and shapes of td3_continuous_action.py's Actor and QNetwork for a
                            (3,) observation and a (1,) action (the classes are executed from the
                            file)
  {td3,ddpg}_update_B*_A*.npz  the script's classes and update lines (td3 :238-274, ddpg
                            :215-238) executed from the file on td3_util.stub_batch and
                            td3_util.stub_networks (seeded, so neither is stored), in f32 and with
                            the same inputs and parameters cast up in f64. The optimizers are
                            stand-ins that record the gradients at their step() and change
                            nothing, so the actor loss sees the stub qf1. torch.randn_like is the
                            recorded draw z (td3_util.stub_batch seeds torch before it) in both
                            dtypes. Arrays per dtype tag: td3_util.FIXTURE_KEYS (next_actions,
                            next_q_value, losses = qf1_loss, [qf2_loss,] actor_loss, dq1, dq2, dmu
                            = the gradient at fc_mu's output, polyak = the new target fc_mu.bias
                            and qf1_target fc3.weight, grads = every parameter gradient but the
                            fc2.weight ones, td3_util.grad_names' order).
Before a fixture is written, td3_util.assert_branches checks the rows it needs and the f32 run is
checked against every tolerance of tests/test_td3_cpu.py (it is its own reference: the check is
that the package's plain-torch restatement, run here, stays inside them too).
"""
import ast
import copy
import json
import sys
import textwrap
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
sys.path.insert(0, str(HERE.parent.parent))
import td3_util as U  # noqa: E402  (tests/td3_util.py)


def args_fields(tree, path: Path) -> dict:
    """Names and defaults of the script's Args: literals, exp_name from the file's name, and
    `int(<literal>)` (buffer_size) evaluated."""
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Args")
    out = {}
    for n in cls.body:
        if not isinstance(n, ast.AnnAssign):
            continue
        v = n.value
        if n.target.id == "exp_name":
            out["exp_name"] = path.stem
        elif isinstance(v, ast.Call) and isinstance(v.func, ast.Name) and v.func.id == "int":
            out[n.target.id] = int(ast.literal_eval(v.args[0]))
        else:
            out[n.target.id] = ast.literal_eval(v)
    return out


SCRIPTS = {"td3": ("cleanrl/td3_continuous_action.py", (238, 274)),
           "ddpg": ("cleanrl/ddpg_continuous_action.py", (215, 238))}


def definitions(tree, path, names) -> dict:
    import torch.nn as nn
    import torch.nn.functional as F

    ns = {"torch": torch, "nn": nn, "np": np, "F": F}
    for n in tree.body:
        if isinstance(n, ast.ClassDef) and n.name in names:
            exec(compile(ast.Module([n], []), str(path), "exec"), ns)
    return ns


def envs_for(D: int, low, high):
    sp = types.SimpleNamespace
    act = sp(shape=(len(low),), low=np.asarray(low, np.float32), high=np.asarray(high, np.float32))
    return sp(single_observation_space=sp(shape=(D,)), single_action_space=act, action_space=act)


class _TorchProxy:
    """torch with randn_like returning the recorded draw."""

    def __init__(self, z):
        self._z = z

    def __getattr__(self, name):
        return getattr(torch, name)

    def randn_like(self, t, **_):
        return self._z.to(t.dtype)


class _Recorder:
    """An optimizer stand-in: step() records its parameters' gradients."""

    def __init__(self, named):
        self.named, self.grads = named, None

    def zero_grad(self):
        for _, p in self.named:
            p.grad = None

    def step(self):
        self.grads = {k: p.grad.clone() for k, p in self.named}


def run_update(code, nets, t, dtype, twin: bool) -> dict:
    import torch.nn.functional as F

    n = {k: copy.deepcopy(v).to(dtype) for k, v in nets.items()}
    c = {k: v.to(dtype) for k, v in t.items()}
    kept = {"q": [], "mu": []}
    hooks = [n["qf1"].register_forward_hook(lambda m, i, o: (o.retain_grad(), kept["q"].append(o))[0]),
             n["actor"].fc_mu.register_forward_hook(
                 lambda m, i, o: (o.retain_grad(), kept["mu"].append(o))[0])]
    if twin:
        kept["q2"] = []
        hooks.append(n["qf2"].register_forward_hook(
            lambda m, i, o: (o.retain_grad(), kept["q2"].append(o))[0]))
    qnamed = [(("qf1", k), p) for k, p in n["qf1"].named_parameters()]
    if twin:
        qnamed += [(("qf2", k), p) for k, p in n["qf2"].named_parameters()]
    q_opt = _Recorder(qnamed)
    a_opt = _Recorder([(("actor", k), p) for k, p in n["actor"].named_parameters()])
    before = {"mu_b": n["target_actor"].fc_mu.bias.detach().clone(),
              "w3": n["qf1_target"].fc3.weight.detach().clone()}
    data = types.SimpleNamespace(observations=c["obs"], next_observations=c["next_obs"],
                                 actions=c["actions"], rewards=c["rewards"].view(-1, 1),
                                 dones=c["dones"].view(-1, 1))
    ns = {"torch": _TorchProxy(t["z"]), "F": F, "data": data, "device": "cpu",
          "args": types.SimpleNamespace(policy_frequency=2, **U.HYPER), "global_step": 0,
          "envs": envs_for(c["obs"].shape[1], t["low"].tolist(), t["high"].tolist()),
          "q_optimizer": q_opt, "actor_optimizer": a_opt, **n}
    exec(code, ns)
    for h in hooks:
        h.remove()
    out = {"next_actions": ns["next_state_actions"], "next_q_value": ns["next_q_value"],
           "dq1": kept["q"][0].grad.view(-1), "dmu": kept["mu"][0].grad}
    losses = [ns["qf1_loss"]]
    if twin:
        out["dq2"] = kept["q2"][0].grad.view(-1)
        losses.append(ns["qf2_loss"])
    out["losses"] = torch.stack(losses + [ns["actor_loss"]])
    grads = {**q_opt.grads, **a_opt.grads}
    out["grads"] = torch.cat([grads[k].reshape(-1) for k in U.grad_names(nets)])
    # the script's own soft update of the two recorded tensors (:269-274), and a check that it
    # started from the stub values
    assert not torch.equal(before["mu_b"], n["target_actor"].fc_mu.bias)
    out["polyak"] = torch.cat([n["target_actor"].fc_mu.bias.reshape(-1),
                               n["qf1_target"].fc3.weight.reshape(-1)])
    return {k: v.detach().numpy() for k, v in out.items()}


def main(reference: str):
    defs = None
    for algo, (script, lines) in SCRIPTS.items():
        path = Path(reference) / script
        src = path.read_text()
        tree = ast.parse(src)
        (HERE / f"{algo}_args_fields.json").write_text(json.dumps(args_fields(tree, path)))
        code = textwrap.dedent("".join(src.splitlines(keepends=True)[lines[0] - 1:lines[1]]))
        defs = definitions(tree, path, ("QNetwork", "Actor"))
        twin = algo == "td3"
        if twin:
            torch.manual_seed(0)
            e = envs_for(3, [-2.0], [2.0])
            (HERE / "td3_state_keys.json").write_text(json.dumps(
                {name: {k: list(v.shape) for k, v in defs[name](e).state_dict().items()}
                 for name in ("Actor", "QNetwork")}))
        for B, A, D in U.CASES:
            low, high = U.BOUNDS[A]
            e = envs_for(D, low, high)
            # ddpg's Actor reads env.action_space (:105-110)
            nets = U.stub_networks(lambda k: defs["Actor"](e) if k == "actor" else
                                   defs["QNetwork"](e), B, A, twin)
            t = U.stub_batch(B, A, D)
            U.assert_branches(t, nets, twin)
            out = {}
            runs = {}
            for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
                runs[tag] = run_update(code, nets, t, dtype, twin)
                for k, v in runs[tag].items():
                    out[f"{tag}_{k}"] = v
            # the package's plain-torch restatement against the same tolerances, here on the CPU
            pk = U.update_ref(U.package_networks(B, A, D, twin), t, torch.float32, twin)
            for k in runs["f64"]:
                U.check(f"{algo} B{B} A{A} {k}", pk[k], runs["f32"][k], runs["f64"][k])
            np.savez(HERE / U.fixture_name(algo, B, A), **out)


if __name__ == "__main__":
    main(sys.argv[1])
