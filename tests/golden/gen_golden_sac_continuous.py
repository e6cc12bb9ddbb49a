"""Generate the continuous-SAC fixtures from the reference script (data only, no reference text):

    python tests/golden/gen_golden_sac_continuous.py /path/to/reference

  sac_continuous_args_fields.json  names and defaults of the script's Args, by AST
  sac_continuous_state_keys.json   keys and shapes of sac_continuous_action.py's Actor and
                            SoftQNetwork for a (3,) observation and a (1,) action (the classes are
                            executed from the file)
  sac_continuous_update_B*_A*.npz  the script's classes and update lines (:263-311) executed from
                            the file on sac_continuous_util.stub_batch and stub_networks (seeded,
                            so neither is stored), in f32 and with the same inputs and parameters
                            cast up in f64, at policy_frequency = target_network_frequency = 1 and
                            log_alpha = HYPER's. The q and actor optimizers are stand-ins that
                            record the gradients at their step() and change nothing, so the actor
                            loss sees the stub critics; a_optimizer is torch.optim.Adam itself.
                            torch.distributions.Normal.rsample returns mean + std * z for the
                            recorded draws z_target, z_pi, z_alpha (in the script's call order) in
                            both dtypes. Arrays per dtype tag: sac_continuous_util.FIXTURE_KEYS
                            (next_actions, next_log_pi, next_q_value, losses = qf1, qf2, actor,
                            alpha, dq1, dq2, dmean / dr = the gradients at fc_mean's and
                            fc_logstd's outputs, polyak = the new qf1_target fc3.weight, temp =
                            log_alpha and alpha after the step, grads = every parameter gradient
                            but the fc2.weight ones, grad_names' order).
Before a fixture is written, sac_continuous_util.assert_branches checks the rows it needs (with a
margin of 0.25 on the excluded band of |x|) and the package's plain-torch restatement, run here,
is checked against every tolerance of tests/test_sac_continuous_cpu.py.
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
import sac_continuous_util as U  # noqa: E402  (tests/sac_continuous_util.py)
from gen_golden_td3 import _Recorder, args_fields, envs_for  # noqa: E402

SCRIPT, LINES = "cleanrl/sac_continuous_action.py", (263, 311)
MARGIN = 0.25


def definitions(tree, path, names, torch_mod) -> dict:
    import torch.nn as nn
    import torch.nn.functional as F

    ns = {"torch": torch_mod, "nn": nn, "np": np, "F": F}
    for n in tree.body:
        if isinstance(n, ast.ClassDef) and n.name in names:
            exec(compile(ast.Module([n], []), str(path), "exec"), ns)
        elif isinstance(n, ast.Assign) and isinstance(n.targets[0], ast.Name) and \
                n.targets[0].id.startswith("LOG_STD_"):
            ns[n.targets[0].id] = ast.literal_eval(n.value)
    return ns


class _TorchProxy:
    """torch with distributions.Normal.rsample returning mean + std * (the next recorded draw)."""

    def __init__(self):
        self.queue = []
        proxy = self

        class Normal(torch.distributions.Normal):
            def rsample(self, sample_shape=torch.Size()):
                return self.loc + proxy.queue.pop(0).to(self.loc.dtype) * self.scale

        self.distributions = types.SimpleNamespace(Normal=Normal)

    def __getattr__(self, name):
        return getattr(torch, name)


def run_update(code, proxy, nets, t, dtype) -> dict:
    import torch.nn.functional as F

    h = U.HYPER
    n = {k: copy.deepcopy(v).to(dtype) for k, v in nets.items()}
    c = {k: v.to(dtype) for k, v in t.items()}
    kept = {k: [] for k in ("q1", "q2", "mean", "r")}

    def keep(key):
        def hook(m, i, o):
            if o.requires_grad:
                o.retain_grad()
            kept[key].append(o)
        return hook

    ac = n["actor"]
    hooks = [n["qf1"].register_forward_hook(keep("q1")), n["qf2"].register_forward_hook(keep("q2")),
             ac.fc_mean.register_forward_hook(keep("mean")),
             ac.fc_logstd.register_forward_hook(keep("r"))]
    q_opt = _Recorder([((m, k), p) for m in ("qf1", "qf2") for k, p in n[m].named_parameters()])
    a_opt = _Recorder([(("actor", k), p) for k, p in ac.named_parameters()])
    log_alpha = torch.tensor([h["log_alpha"]], dtype=dtype, requires_grad=True)
    w3 = n["qf1_target"].fc3.weight.detach().clone()
    data = types.SimpleNamespace(observations=c["obs"], next_observations=c["next_obs"],
                                 actions=c["actions"], rewards=c["rewards"].view(-1, 1),
                                 dones=c["dones"].view(-1, 1))
    A = c["actions"].shape[1]
    proxy.queue[:] = [t[k] for k in U.DRAWS]
    ns = {"torch": proxy, "F": F, "data": data, "device": "cpu", "global_step": 0,
          "args": types.SimpleNamespace(policy_frequency=1, target_network_frequency=1,
                                        autotune=True, gamma=h["gamma"], tau=h["tau"],
                                        batch_size=c["obs"].shape[0]),
          "q_optimizer": q_opt, "actor_optimizer": a_opt, "log_alpha": log_alpha,
          "alpha": log_alpha.exp().item(), "target_entropy": -float(A),
          "a_optimizer": torch.optim.Adam([log_alpha], lr=h["q_lr"]),
          "rb": types.SimpleNamespace(sample=lambda batch_size: data), **n}
    exec(code, ns)
    for hk in hooks:
        hk.remove()
    assert not proxy.queue and not torch.equal(w3, n["qf1_target"].fc3.weight)
    # forward order: q1(s, a), q1(s, pi); mean / r: next_obs (no grad), obs (the actor loss), obs
    out = {"next_actions": ns["next_state_actions"], "next_log_pi": ns["next_state_log_pi"].view(-1),
           "next_q_value": ns["next_q_value"], "dq1": kept["q1"][0].grad.view(-1),
           "dq2": kept["q2"][0].grad.view(-1), "dmean": kept["mean"][1].grad,
           "dr": kept["r"][1].grad,
           "losses": torch.stack([ns["qf1_loss"], ns["qf2_loss"], ns["actor_loss"],
                                  ns["alpha_loss"]]),
           "temp": torch.cat([log_alpha.detach(), torch.tensor([ns["alpha"]], dtype=dtype)]),
           "polyak": n["qf1_target"].fc3.weight.reshape(-1)}
    grads = {**q_opt.grads, **a_opt.grads}
    out["grads"] = torch.cat([grads[k].reshape(-1) for k in U.grad_names(nets)])
    return {k: v.detach().numpy() for k, v in out.items()}


def main(reference: str):
    path = Path(reference) / SCRIPT
    src = path.read_text()
    tree = ast.parse(src)
    (HERE / "sac_continuous_args_fields.json").write_text(json.dumps(args_fields(tree, path)))
    code = textwrap.dedent("".join(src.splitlines(keepends=True)[LINES[0] - 1:LINES[1]]))
    proxy = _TorchProxy()
    defs = definitions(tree, path, ("SoftQNetwork", "Actor"), proxy)
    torch.manual_seed(0)
    e = envs_for(3, [-2.0], [2.0])
    (HERE / "sac_continuous_state_keys.json").write_text(json.dumps(
        {name: {k: list(v.shape) for k, v in defs[name](e).state_dict().items()}
         for name in ("Actor", "SoftQNetwork")}))
    for B, A, D in U.CASES:
        e = envs_for(D, *U.BOUNDS[A])
        nets = U.stub_networks(lambda k: defs["Actor"](e) if k == "actor" else
                               defs["SoftQNetwork"](e), B, A)
        t = U.stub_batch(B, A, D, nets["actor"])
        U.assert_branches(t, nets, MARGIN)
        out, runs = {}, {}
        for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            runs[tag] = run_update(code, proxy, nets, t, dtype)
            for k, v in runs[tag].items():
                out[f"{tag}_{k}"] = v
        # the package's plain-torch restatement against the same tolerances, here on the CPU
        pk = U.update_ref(U.package_networks(B, A, D), t, torch.float32)
        assert set(pk) == set(runs["f64"]) == set(U.FIXTURE_KEYS)
        for k in U.FIXTURE_KEYS:
            U.check(f"B{B} A{A} {k}", pk[k], runs["f32"][k], runs["f64"][k])
        np.savez(HERE / U.fixture_name(B, A), **out)


if __name__ == "__main__":
    main(sys.argv[1])
