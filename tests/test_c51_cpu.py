"""C51 surface without a GPU: the Args dataclass and QNetworkC51 against fixtures made from the
reference (tests/golden/gen_golden_c51.py), the loss fixtures read back through a torch
restatement, and the new ABI entry points' argument validation."""
import ctypes
import dataclasses
import json

import numpy as np
import pytest
import torch

from c51_util import CHECKED, F32_FLOOR, FIXTURES, fixture, rel_err, restated
from conftest import GOLDEN, golden


def test_args_fields_and_defaults_match_reference():
    from oc_cleanrl_amd.c51 import C51Args

    ref = json.loads((GOLDEN / "c51_args_fields.json").read_text())
    mine = {f.name: f.default for f in dataclasses.fields(C51Args)}
    assert [n for n, _ in ref] == list(mine)[:len(ref)]  # same names, same order, ours after
    for name, default in ref:
        if name == "backend":  # ALE / OCAtari are not available: declared difference
            assert mine[name] == "Synthetic" and default == "OCAtari"
            continue
        assert mine[name] == default, name
    assert "tau" not in mine and "masked_wrapper" not in mine
    a = C51Args()
    assert (a.n_atoms, a.v_min, a.v_max, a.target_network_frequency) == (51, -10, 10, 10000)
    assert a.learning_rate == 2.5e-4 and a.total_timesteps == 20_000_000


def _seeded_net():
    from oc_cleanrl_amd.c51 import QNetworkC51

    z = golden("c51_init_a6.npz")
    torch.manual_seed(int(z["seed"]))
    net = QNetworkC51((4, 84, 84), int(z["n_actions"]), n_atoms=int(z["n_atoms"]), v_min=-10,
                      v_max=10)
    return net, z


def test_qnetwork_c51_layout_and_seeded_init():
    net, z = _seeded_net()
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in z["keys"]]  # same keys, same order (atoms first)
    assert torch.equal(sd["atoms"], torch.from_numpy(z["atoms"]))  # bitwise
    for (k, v), shape, (s, sa) in zip(sd.items(), z["shapes"], z["sums"]):
        assert list(v.shape) == json.loads(str(shape)), k
        np.testing.assert_allclose(float(v.double().sum()), s, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(float(v.double().abs().sum()), sa, rtol=1e-6)


def test_qnetwork_c51_get_action_matches_reference():
    net, z = _seeded_net()
    x = torch.from_numpy(z["x"]).float()
    with torch.no_grad():
        action, pmfs = net.get_action(x)
        given, pmfs_given = net.get_action(x, torch.from_numpy(z["given"]))
        a2, qv, _, _ = net.get_action_and_value(x)
    assert np.array_equal(action.numpy(), z["action"])
    np.testing.assert_allclose(pmfs.numpy(), z["pmfs"], rtol=1e-4, atol=1e-6)
    assert np.array_equal(given.numpy(), z["given"])
    np.testing.assert_allclose(pmfs_given.numpy(), z["pmfs_given"], rtol=1e-4, atol=1e-6)
    assert np.array_equal(a2.numpy(), z["action"]) and tuple(qv.shape) == (2, 2)
    assert np.array_equal(net.predict(z["x"])[0], z["action"])


def test_class_defaults_are_the_reference_ones():
    from oc_cleanrl_amd.c51 import QNetworkC51Obj

    net = QNetworkC51Obj((4, 6), 3, encoder_dims=(8,), decoder_dims=(8,))
    assert net.n_atoms == 101 and float(net.atoms[0]) == -100 and float(net.atoms[-1]) == 100
    assert list(net.state_dict())[0] == "atoms" and net.network[-1].out_features == 3 * 101
    with torch.no_grad():
        action, pmf = net.get_action(torch.zeros(2, 4, 6))
    assert tuple(pmf.shape) == (2, 101) and tuple(action.shape) == (2,)


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_fixture(name):
    """The fixtures are read correctly: the restated loss gives the reference's f32 outputs (to
    f32 rounding: CPUs vectorise the sums differently) and its f64 twin's."""
    z = fixture(name)
    r32, r64 = restated(z, torch.float32), restated(z, torch.float64)
    assert np.array_equal(r32["next_action"], z["next_action"])
    assert np.array_equal(r64["next_action"], z["next_action"])
    for k in CHECKED + ("old_pmfs",):
        assert rel_err(r32[k], z[k]) <= F32_FLOOR, k
        assert rel_err(r64[k], z[k + "64"]) <= 1e-12, k
        assert r32[k].dtype == np.float32 and z[k + "64"].dtype == np.float64
    assert np.array_equal(r32["dlogits"] == 0, z["dlogits"] == 0)


def test_fixture_conditions():
    """What each fixture is for holds in the stored data."""
    z = fixture("b32_a6_n51")
    assert float(z["atoms"][1] - z["atoms"][0]) == float(np.float32(0.39999962))  # not 0.4
    p = fixture("peaked")["old_pmfs"].astype(np.float64)
    assert np.abs(p / 1e-5 - 1).min() > 1e-3 and np.abs(p - (1 - 1e-5)).min() > 1e-6
    assert (p < 1e-5).any() and (p > 1e-5).any() and (p > 1 - 1e-5).any() and (p < 1 - 1e-5).any()
    t = fixture("ties")
    assert np.abs(t["target_pmfs"].sum(1) - 1).max() <= 2.0 ** -22
    z = fixture("b7_a18_n101")
    assert z["logits"].shape == (7, 18 * 101) and z["atoms"].size == 101


def test_abi_rejects_bad_sizes_and_null_pointers():
    from oc_cleanrl_amd import _lib

    L = _lib.LIB
    d = ctypes.c_void_p(256)

    def loss(B=4, A=6, N=51, ptrs=(d,) * 8):
        lg, ln, at, ac, rw, dn, dl, st = ptrs
        return L.ocppo_c51_loss_fwd_bwd(None, lg, ln, at, ac, rw, dn, B, A, N, 0.99, -10.0, 10.0,
                                        dl, st, None, None)

    def act(E=4, A=6, N=51, ptrs=(d,) * 4, duration=100.0):
        lg, at, st, ac = ptrs
        return L.ocppo_c51_epsilon_greedy(None, lg, at, E, A, N, 1, st, 0, 1.0, 0.01, duration,
                                          ac, None, None)

    for fn in (loss, act):
        for kw in (dict(N=1), dict(N=129), dict(A=19), dict(A=0)):
            assert fn(**kw) == _lib.OCPPO_E_INVALID, (fn.__name__, kw)
            assert b"bad sizes" in L.ocppo_last_error()
    assert loss(B=0) == _lib.OCPPO_E_INVALID and act(E=0) == _lib.OCPPO_E_INVALID
    assert act(duration=0.0) == _lib.OCPPO_E_INVALID
    for i in range(8):
        ptrs = tuple(None if j == i else d for j in range(8))
        assert loss(ptrs=ptrs) == _lib.OCPPO_E_INVALID, i
        assert b"null pointer" in L.ocppo_last_error()
    for i in range(4):
        ptrs = tuple(None if j == i else d for j in range(4))
        assert act(ptrs=ptrs) == _lib.OCPPO_E_INVALID, i
        assert b"null pointer" in L.ocppo_last_error()


def test_ops_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from oc_cleanrl_amd import ops

    atoms = torch.linspace(-10, 10, 51)
    step = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="GPU"):
        ops.c51_epsilon_greedy(torch.zeros(2, 6 * 51), atoms, 1, step, 1.0, 0.01, 10.0)
    with pytest.raises(ValueError, match="A \\* 51"):
        ops.c51_epsilon_greedy(torch.zeros(2, 100), atoms, 1, step, 1.0, 0.01, 10.0)
    with pytest.raises(ValueError, match="N=1"):
        ops.c51_loss_fwd_bwd(torch.zeros(2, 6), torch.zeros(2, 6), torch.zeros(1),
                             torch.zeros(2, dtype=torch.int64), torch.zeros(2), torch.zeros(2),
                             0.99, -10, 10)
