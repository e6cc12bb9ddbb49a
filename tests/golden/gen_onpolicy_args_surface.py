"""Writes tests/golden/onpolicy_args_surface.json: the argument surface of the seven learners that
run on trainer.PPOTrainer (lstm, transformer, pqn, pqn_lstm, rnd, ppg, contppo), read from this
package alone. tests/test_learner_args_cpu.py rebuilds the same structure (surface()) and compares.

    python tests/golden/gen_onpolicy_args_surface.py

Per class: its __name__ and __doc__; [name, str(type), default] of dataclasses.fields, in order;
the class attribute of every args.Args field that is not a dataclass field of the class; the
instance __dict__ after the module's finalize on the default instance and on a small one
(num_envs 6, num_steps 4, num_minibatches 3; ppg also n_iteration 2, num_aux_rollouts 3); for
contppo also on rpo's defaults. A value JSON cannot hold as it is (a tuple) is recorded as its repr.
"""
from __future__ import annotations

import dataclasses
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

# module name, class name, extra keywords of the small instance
LEARNERS = (("lstm", "LSTMArgs", {}), ("transformer", "TransformerArgs", {}),
            ("pqn", "PQNArgs", {}), ("pqn_lstm", "PQNLSTMArgs", {}), ("rnd", "RNDArgs", {}),
            ("ppg", "PPGArgs", {"n_iteration": 2, "num_aux_rollouts": 3}),
            ("contppo", "ContPPOArgs", {}))
SMALL = {"num_envs": 6, "num_steps": 4, "num_minibatches": 3}


def _enc(v):
    return v if v is None or isinstance(v, (bool, int, float, str)) else repr(v)


def _finalized(mod, cls, **kw) -> dict:
    return {k: _enc(v) for k, v in vars(mod.finalize(cls(**kw))).items()}


def surface() -> dict:
    import importlib

    from oc_cleanrl_amd.args import Args
    from oc_cleanrl_amd.rpo import RPO_DEFAULTS

    out = {}
    for modname, clsname, extra in LEARNERS:
        mod = importlib.import_module(f"oc_cleanrl_amd.{modname}")
        cls = getattr(mod, clsname)
        own = {f.name for f in dataclasses.fields(cls)}
        rec = {
            "name": cls.__name__, "doc": cls.__doc__,
            "fields": [[f.name, str(f.type), _enc(f.default)] for f in dataclasses.fields(cls)],
            "class_attrs": {f.name: _enc(getattr(cls, f.name)) for f in dataclasses.fields(Args)
                            if f.name not in own},
            "finalized_default": _finalized(mod, cls),
            "finalized_small": _finalized(mod, cls, **SMALL, **extra),
        }
        if modname == "contppo":
            rec["finalized_rpo"] = _finalized(mod, cls, **RPO_DEFAULTS)
        out[modname] = rec
    return out


if __name__ == "__main__":
    dst = Path(__file__).resolve().parent / "onpolicy_args_surface.json"
    dst.write_text(json.dumps(surface(), indent=1) + "\n")
    print(dst)
