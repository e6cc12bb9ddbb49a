"""The two QDagger launches (csrc/ocppo_qdagger.hip): the loss against the float64 twin of
tests/qdagger_util.py by the error rule (lstm_util.check) over every action count, every batch
size around the wave and the 256-thread workgroup, every temperature and coefficient; its exact
properties (the TD half's bits, a zero distillation term, run-to-run equality); and the
episodic-return ring against its Python restatement, bit for bit after every call."""
import numpy as np
import pytest
import torch

import lstm_util as lu
import qdagger_util as qu

pytestmark = pytest.mark.gpu

ACTIONS = [1, 2, 6, 18]
BATCHES = [1, 2, 63, 64, 65, 255, 256, 257]
TEMPERATURES = [0.5, 1.0, 4.0]
COEFFS = [0.0, 0.37, 1.0, None]  # None: the null pointer (1.0, the offline phase)
GAMMA = float(np.float32(0.99))  # the kernel rounds gamma to f32 once: the twin's input is that
DEV = "cuda"


def make_inputs(B: int, A: int, all_done: bool = False):
    """f32 CPU inputs: seeded randn Q values, dones alternating 0 / 1 (or all 1); with more than
    one row, row 0's top teacher logit leads by 90 (the other entries' softmax underflows,
    log_softmax stays finite); q_next's row maximum is tied between two actions where A > 1."""
    g = torch.Generator().manual_seed(1000 * A + B)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    z = dict(q=r(B, A), q_next=r(B, A), q_teacher=2 * r(B, A),
             actions=torch.randint(0, A, (B,), generator=g), rewards=r(B),
             dones=torch.ones(B) if all_done else (torch.arange(B) % 2).float())
    if B > 1:
        z["q_teacher"][0, A // 2] = z["q_teacher"][0].max() + 90.0
    if A > 1:
        top = z["q_next"].max(dim=1).values
        z["q_next"][torch.arange(B), torch.arange(B) % A] = top
        z["q_next"][torch.arange(B), (torch.arange(B) + 1) % A] = top
    return z


def launch(z, T, coeff):
    from oc_cleanrl_amd import ops

    d = {k: v.to(DEV) for k, v in z.items()}
    c = None if coeff is None else torch.tensor([coeff], dtype=torch.float32, device=DEV)
    stats, dq = ops.qdagger_loss_fwd_bwd(d["q"], d["q_next"], d["q_teacher"], d["actions"],
                                         d["rewards"], d["dones"], GAMMA, T, c)
    return stats.cpu(), dq.cpu()


def td_launch(z):
    from oc_cleanrl_amd import ops

    d = {k: v.to(DEV) for k, v in z.items()}
    stats, dq = ops.td_loss_fwd_bwd(d["q"], d["q_next"], d["actions"], d["rewards"], d["dones"],
                                    GAMMA)
    return stats.cpu(), dq.cpu()


def bits(x):
    return x.contiguous().view(torch.int32)


def check_case(z, T, coeff, tag):
    stats, dq = launch(z, T, coeff)
    st64, dq64 = qu.loss_twin(**z, gamma=GAMMA, temperature=T, coeff=coeff)
    st32, dq32 = qu.loss_twin(**z, gamma=GAMMA, temperature=T, coeff=coeff, dtype=torch.float32)
    lu.check(tag + " dq", dq, dq32, dq64)
    for i, name in enumerate(("loss", "q_loss", "distill", "q_mean")):
        if float(st64[i]) == 0.0:  # A = 1: no distillation term at all
            assert float(stats[i]) == 0.0, (tag, name)
        else:
            lu.check(f"{tag} {name}", stats[i], st32[i], st64[i])
    assert float(stats[4]) == float(np.float32(1.0 if coeff is None else coeff))
    return stats, dq


@pytest.mark.parametrize("A", ACTIONS)
@pytest.mark.parametrize("B", BATCHES)
def test_loss_against_the_f64_twin(B, A):
    z = make_inputs(B, A)
    td_stats, td_dq = td_launch(z)
    for T in TEMPERATURES:
        for coeff in COEFFS:
            stats, dq = check_case(z, T, coeff, f"B{B} A{A} T{T} c{coeff}")
            # the TD half is td_loss_kernel's device code
            assert torch.equal(bits(stats[[1, 3]]), bits(td_stats))
            if coeff == 0.0:
                assert torch.equal(bits(dq), bits(td_dq))
            if A == 1:  # one action: softmax is 1, the distillation term and its gradient vanish
                assert float(stats[2]) == 0.0 and torch.equal(bits(dq), bits(td_dq))
                assert torch.equal(bits(stats[0:1]), bits(stats[1:2]))


@pytest.mark.parametrize("A", ACTIONS)
def test_all_dones_one(A):
    z = make_inputs(65, A, all_done=True)
    stats, _ = check_case(z, 1.0, 0.37, f"all-done A{A}")
    # the target is the reward alone
    old = z["q"].gather(1, z["actions"].reshape(-1, 1)).squeeze(1)
    want = ((z["rewards"].double() - old.double()) ** 2).mean()
    assert abs(float(stats[1]) - float(want)) <= 1e-5 * float(want)


@pytest.mark.parametrize("A", [2, 6, 18])
@pytest.mark.parametrize("B", [1, 65, 257])
def test_teacher_equal_to_student_gives_the_td_gradient(B, A):
    from oc_cleanrl_amd import ops

    z = make_inputs(B, A)
    d = {k: v.to(DEV) for k, v in z.items()}
    for T in TEMPERATURES:
        stats, dq = ops.qdagger_loss_fwd_bwd(d["q"], d["q_next"], d["q"], d["actions"],
                                             d["rewards"], d["dones"], GAMMA, T, None)
        _, td_dq = td_launch(z)
        assert float(stats[2]) == 0.0
        assert torch.equal(bits(dq.cpu()), bits(td_dq))


def test_two_launches_are_bitwise_equal():
    z = make_inputs(257, 18)
    a, b = launch(z, 0.5, 0.37), launch(z, 0.5, 0.37)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


def scripted_steps(E: int, episodes: int, steps: int = 40):
    """`steps` steps of integer-valued rewards whose done pattern finishes exactly `episodes`
    episodes; where E > 1 and enough episodes remain, a step ends several envs at once."""
    rng = np.random.RandomState(100 * E + episodes)
    out, left = [], episodes
    for t in range(steps):
        reward = rng.randint(-3, 8, size=E).astype(np.float32)
        done = np.zeros(E, dtype=np.float32)
        if left and t % 2 == 1:
            n = min(left, E, 1 + (t // 2) % 3)  # 1, 2 or 3 envs finish together
            done[rng.permutation(E)[:n]] = 1.0
            left -= n
        out.append((reward, done))
    if left:  # the last step finishes what remains (E = 1 and 23 episodes in 40 steps)
        raise AssertionError("pattern too short")
    return out


@pytest.mark.parametrize("E", [1, 3, 64])
@pytest.mark.parametrize("episodes", [0, 9, 10, 11, 23])
def test_episode_push_is_bitwise_the_restatement(E, episodes):
    from oc_cleanrl_amd import ops

    if E == 1:  # one env finishes at most one episode per step: every step but the first 17
        steps = scripted_steps(1, 0)
        for t in range(40 - episodes, 40):
            steps[t][1][0] = 1.0
    else:
        steps = scripted_steps(E, episodes)
    teacher = 7.5
    ring = ops.EpisodeRing(E, DEV)
    pushed, prev_run = [], np.zeros(E, dtype=np.float32)
    ref = qu.episode_ring_ref(steps, E, teacher)
    for (reward, done), (returns, run, coeff) in zip(steps, ref):
        ops.qdagger_episode_push(torch.from_numpy(reward).to(DEV), torch.from_numpy(done).to(DEV),
                                 ring, teacher)
        pushed += [np.float32(prev_run[e] + reward[e]) for e in range(E) if done[e]]
        prev_run = run
        want_ring, head, count = qu.ring_layout(pushed)
        assert ring.state.tolist() == [head, count]
        assert ring.ring.cpu().numpy().tobytes() == want_ring.tobytes()
        assert ring.run_ret.cpu().numpy().tobytes() == run.tobytes()
        assert ring.coeff.cpu().numpy().tobytes() == np.float32(coeff).tobytes()
        assert ring.returns() == returns
    assert len(pushed) == episodes
