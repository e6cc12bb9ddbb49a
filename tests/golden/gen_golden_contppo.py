"""Generate the continuous-action PPO / RPO fixtures from the reference scripts (data only, no
reference text):

    python tests/golden/gen_golden_contppo.py /path/to/reference

  contppo_args_fields.json / rpo_args_fields.json   names and defaults of the scripts' Args, by AST
  contppo_state_keys.json   keys and shapes of ppo_continuous_action.py's Agent for a (3,)
                            observation and a (1,) action (its class is executed from the file)
  contppo_update_M*_A*.npz  the script's Agent (:112-141) and update lines (:265-300) executed
                            from the file on seeded stub data and stub parameters
                            (contppo_util.stub_parameters: a seeded CPU randn, the same bits on
                            any machine, so the parameters are not stored), with loss.backward().
                            Arrays (contppo_util.load_update reads them): obs, actions, batch
                            [4, M] = old log-probs, advantages, returns, old values, hyper [5];
                            in f32 and (the same inputs and parameters cast up) in f64: terms [7]
                            = the loss terms, heads = mean, newvalue, dmean, dvalue flattened;
                            grads = every parameter gradient in named_parameters() order,
                            flattened (contppo_util.split_grads)
"""
import ast
import json
import sys
import textwrap
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
from contppo_util import TERMS, flat_grads, stub_parameters  # noqa: E402  (tests/contppo_util.py)
SCRIPT = "cleanrl/ppo_continuous_action.py"
RPO_SCRIPT = "cleanrl/rpo_continuous_action.py"
UPDATE_LINES = (265, 300)
CASES = [(64, 1, 3), (33, 6, 5)]  # (M, A, D)
HYPER = dict(clip_coef=0.2, norm_adv=True, clip_vloss=True, ent_coef=0.01, vf_coef=0.5)
# row m's log-ratio / value difference (tests/contppo_util.py's cycles)
LOGRATIO_CYCLE = (-0.5, -0.1, 0.1, 0.5)
VDIFF_CYCLE = (-0.5, -0.05, 0.05, 0.5)


def args_fields(tree, path: Path) -> dict:
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Args")
    out = {}
    for n in cls.body:
        if isinstance(n, ast.AnnAssign):
            try:
                out[n.target.id] = ast.literal_eval(n.value)
            except ValueError:
                assert n.target.id == "exp_name"  # derived from the file's name
                out[n.target.id] = path.stem
    return out


def definitions(tree, names) -> dict:
    """Execute the named top-level classes / functions of the script in a fresh namespace."""
    import torch.nn as nn
    from torch.distributions.normal import Normal

    ns = {"torch": torch, "nn": nn, "np": np, "Normal": Normal}
    for n in tree.body:
        if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names:
            exec(compile(ast.Module([n], []), SCRIPT, "exec"), ns)
    return ns


def make_agent(defs, D: int, A: int):
    space = types.SimpleNamespace
    envs = space(single_observation_space=space(shape=(D,)), single_action_space=space(shape=(A,)))
    return defs["Agent"](envs)


def run_update(code, defs, agent, t: dict, dtype) -> dict:
    """The script's update lines on agent and the batch t, both cast to `dtype`."""
    import copy

    ag = copy.deepcopy(agent).to(dtype)
    c = {k: v.to(dtype) for k, v in t.items()}
    kept = {}
    hooks = [ag.actor_mean.register_forward_hook(lambda m, i, o: (o.retain_grad(), kept.update(mean=o))[0]),
             ag.critic.register_forward_hook(lambda m, i, o: (o.retain_grad(), kept.update(value=o))[0])]
    M = c["obs"].shape[0]
    ns = {"torch": torch, "agent": ag, "args": types.SimpleNamespace(**HYPER), "clipfracs": [],
          "b_obs": c["obs"], "b_actions": c["actions"], "b_logprobs": c["logprobs"],
          "b_advantages": c["advantages"], "b_returns": c["returns"], "b_values": c["values"],
          "mb_inds": np.arange(M)}
    exec(code, ns)
    ns["loss"].backward()
    for h in hooks:
        h.remove()
    out = {k: ns[k].detach().numpy() for k in ("loss", "pg_loss", "v_loss", "entropy_loss",
                                                "old_approx_kl", "approx_kl")}
    out["clipfrac"] = np.asarray(ns["clipfracs"][-1], np.float64)
    out["mean"], out["newvalue"] = kept["mean"].detach().numpy(), kept["value"].detach().numpy()
    out["dmean"], out["dvalue"] = kept["mean"].grad.numpy(), kept["value"].grad.numpy()
    for k, p in ag.named_parameters():
        out["grad." + k] = p.grad.numpy()
    return out


def main(reference: str):
    for script, name in ((SCRIPT, "contppo"), (RPO_SCRIPT, "rpo")):
        path = Path(reference) / script
        (HERE / f"{name}_args_fields.json").write_text(
            json.dumps(args_fields(ast.parse(path.read_text()), path)))
    path = Path(reference) / SCRIPT
    src = path.read_text()
    tree = ast.parse(src)
    code = textwrap.dedent("".join(src.splitlines(keepends=True)[UPDATE_LINES[0] - 1:UPDATE_LINES[1]]))
    defs = definitions(tree, ("layer_init", "Agent"))
    torch.manual_seed(0)
    (HERE / "contppo_state_keys.json").write_text(json.dumps(
        {k: list(v.shape) for k, v in make_agent(defs, 3, 1).state_dict().items()}))
    for M, A, D in CASES:
        agent = stub_parameters(make_agent(defs, D, A), 1000 * M + A)
        g = torch.Generator().manual_seed(M + 7 * A)
        t = {"obs": torch.randn(M, D, generator=g), "advantages": torch.randn(M, generator=g),
             "returns": torch.randn(M, generator=g)}
        with torch.no_grad():
            mean = agent.actor_mean(t["obs"])
            t["actions"] = mean + torch.exp(agent.actor_logstd) * torch.randn(M, A, generator=g)
            a64 = __import__("copy").deepcopy(agent).double()
            _, lp, _, v = a64.get_action_and_value(t["obs"].double(), t["actions"].double())
        m = torch.arange(M)
        jit = lambda s: s * (2 * torch.rand(M, generator=g, dtype=torch.float64) - 1)  # noqa: E731
        t["logprobs"] = (lp - torch.tensor(LOGRATIO_CYCLE, dtype=torch.float64)[m % 4]
                         - jit(0.03)).float()
        t["values"] = (v.view(-1) - torch.tensor(VDIFF_CYCLE, dtype=torch.float64)[(3 * m + 1) % 4]
                       - jit(0.02)).float()
        t["advantages"][2] = 0.0
        out = {"obs": t["obs"].numpy(), "actions": t["actions"].numpy(),
               "batch": torch.stack([t[k] for k in ("logprobs", "advantages", "returns",
                                                    "values")]).numpy(),
               "hyper": np.array([HYPER[k] for k in ("clip_coef", "ent_coef", "vf_coef",
                                                     "norm_adv", "clip_vloss")], np.float64)}
        for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            r = run_update(code, defs, agent, t, dtype)
            out[tag + "_terms"] = np.array([r[k] for k in TERMS])
            out[tag + "_heads"] = np.concatenate([r[k].reshape(-1) for k in (
                "mean", "newvalue", "dmean", "dvalue")])
            out[tag + "_grads"] = flat_grads([r["grad." + k] for k, _ in agent.named_parameters()])
        np.savez(HERE / f"contppo_update_M{M}_A{A}.npz", **out)


if __name__ == "__main__":
    main(sys.argv[1])
