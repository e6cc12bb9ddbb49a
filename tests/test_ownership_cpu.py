"""Who owns process-lived state ("Who owns derived state"): ops._persistent, the one
per-shape workspace cache, and agents.rollout_inference, the one per-thread rollout scope."""
import threading

import torch

from oc_cleanrl_amd import agents, ops


def test_persistent_allocates_each_key_once():
    calls = []

    def make():
        calls.append(1)
        return torch.zeros(4)

    key = ("test_persistent_allocates_each_key_once", 3, 5)
    a = ops._persistent("tag_a", "cpu", key, make)
    assert ops._persistent("tag_a", "cpu", key, make) is a
    assert ops._persistent("tag_a", torch.device("cpu"), key, make) is a  # one device, one form
    assert ops._persistent("tag_a", torch.device("cpu", 0), key, make) is a
    assert len(calls) == 1
    b = ops._persistent("tag_b", "cpu", key, make)  # another owner, the same key tuple
    assert b is not a and b.data_ptr() != a.data_ptr() and len(calls) == 2
    assert ops._persistent("tag_a", "cpu", key + (1,), make) is not a and len(calls) == 3
    # a zeroed-once workspace keeps what its launches leave in it
    a[2] = 7.0
    again = ops._persistent("tag_a", "cpu", key, make)
    assert again.tolist() == [0.0, 0.0, 7.0, 0.0] and b.tolist() == [0.0] * 4
    assert len(calls) == 3


def test_rollout_scope_nests_and_counts_outermost_entries():
    assert not agents._in_rollout()
    with agents.rollout_inference():
        g1 = agents._ROLLOUT.gen
        assert agents._in_rollout()
        with agents.rollout_inference():
            assert agents._in_rollout() and agents._ROLLOUT.gen == g1  # inner entry: same rollout
        assert agents._in_rollout()  # the inner exit leaves the outer scope open
        assert agents._ROLLOUT.gen == g1
    assert not agents._in_rollout()
    with agents.rollout_inference():
        g2 = agents._ROLLOUT.gen
    assert g2 > g1
    with agents.rollout_inference():
        assert agents._ROLLOUT.gen > g2
    assert not agents._in_rollout()


def test_rollout_scope_is_per_thread():
    seen = {}

    def other():
        seen["inside"] = agents._in_rollout()
        with agents.rollout_inference():
            seen["own"] = agents._in_rollout()
            seen["gen"] = agents._ROLLOUT.gen
        seen["after"] = agents._in_rollout()

    with agents.rollout_inference():
        mine = agents._ROLLOUT.gen
        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert agents._in_rollout() and agents._ROLLOUT.gen == mine  # untouched by the thread
    assert seen["inside"] is False and seen["own"] is True and seen["after"] is False
    assert seen["gen"] != mine  # a form stamped by one thread's rollout is stale in another's


def test_rollout_form_is_made_once_and_refilled_once_per_rollout():
    w = torch.nn.Parameter(torch.arange(6.0).view(2, 3))
    made, filled = [], []

    def make():
        made.append(1)
        return torch.empty(2, 3)

    def fill(t):
        filled.append(1)
        t.copy_(w)

    def form():
        return agents._rollout_form(w, "test", make, fill)

    with agents.rollout_inference():
        a = form()
        with agents.rollout_inference():
            assert form() is a
        assert form() is a and len(filled) == 1 and torch.equal(a, w)
    with torch.no_grad():
        w.mul_(2.0)
    with agents.rollout_inference():
        assert form() is a and form() is a
    assert len(made) == 1 and len(filled) == 2 and torch.equal(a, w)
    assert w._ocppo_rollout["test"][0] is a
