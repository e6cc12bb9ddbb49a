"""The dropout mask function without a GPU: the numpy restatement of Philox4x32-10
(tests/dropout_util.py) against the Random123 known answers, the keep rate of the elementwise
layout, the two layouts' indexing, and the fused_dropout switch of the transformer agent."""
import math

import numpy as np
import pytest

import dropout_util as du

# Random123 kat_vectors, philox4x32 10 rounds: counter, key -> output
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,out", KNOWN)
def test_philox_known_answers(counter, key, out):
    got = du.philox4x32_10(counter, key)
    assert got.dtype == np.uint32 and tuple(int(v) for v in got) == out


def test_philox_blocks_is_the_counter_and_key_layout():
    """counter = (lo32 blk, hi32 blk, lo32 sub, hi32 sub), key = (lo32 seed, hi32 seed),
    sub = offset * 256 + site."""
    seed, offset, site = 0x299f31d0a4093822, 0x0370734413198a, 0x2e
    blk = np.array([0x85a308d3243f6a88], dtype=np.uint64)
    assert offset * 256 + site == 0x0370734413198a2e
    got = du.philox_blocks(seed, offset, site, blk)[0]
    assert tuple(int(v) for v in got) == KNOWN[2][2]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("site", [0, 1, 11])
@pytest.mark.parametrize("offset", [0, 1])
def test_keep_rate_of_the_elementwise_layout(offset, site, p):
    n = 2 ** 20
    keep = du.keep_elementwise(1234, offset, site, n, p)
    rate = float(keep.mean())
    sd = math.sqrt(p * (1 - p) / n)
    print(f"offset {offset} site {site} p {p}: keep {rate:.6f}, {(rate - (1 - p)) / sd:+.2f} sd")
    assert abs(rate - (1 - p)) <= 4 * sd


def test_threshold_and_scale():
    assert du.threshold(0.0) == 0 and du.threshold(0.5) == 2 ** 31
    assert du.threshold(0.1) == int(0.1 * 2 ** 32) == 429496729
    assert du.threshold(1.0 - 2.0 ** -40) == 2 ** 32 - 1
    assert du.scale_f32(0.5) == np.float32(2.0)


def test_layouts_index_the_same_blocks():
    """Element e of the elementwise layout is component e & 3 of block e >> 2; the attention
    layout's row (b, h, i) is the 16 blocks from ((b * H + h) * 64 + i) * 16, whatever S is."""
    seed, offset, site = 99, 3, 5
    w = du.words_elementwise(seed, offset, site, 2 * 3 * 64 * 16 * 4)  # every block of B * H = 6
    assert np.array_equal(du.words_elementwise(seed, offset, site, 7), w[:7])
    B, H = 2, 3
    for S in (1, 4, 5, 17, 64):
        a = du.words_attention(seed, offset, site, B, H, S)
        assert a.shape == (B, H, S, S)
        for b, h, i in ((0, 0, 0), (1, 2, S - 1), (0, 1, S // 2)):
            blk0 = ((b * H + h) * 64 + i) * 16
            assert np.array_equal(a[b, h, i], w[4 * blk0:4 * blk0 + S])
    # sites and offsets are separate subsequences
    assert not np.array_equal(du.words_elementwise(seed, offset, site + 1, 64), w[:64])
    assert not np.array_equal(du.words_elementwise(seed, offset + 1, site, 64), w[:64])


def test_fused_dropout_is_off_by_default_and_opens_the_fused_path():
    from oc_cleanrl_amd import transformer as T

    assert T.TransformerArgs().fused_dropout is False
    assert T.attn_shape_ok(6, 128, 8, 0.1, fused_dropout=True)
    assert not T.attn_shape_ok(6, 128, 8, 0.1)
    assert T.attn_shape_ok(6, 128, 8, 0.0) and T.attn_shape_ok(6, 128, 8, 0.0, fused_dropout=True)
    assert not T.attn_shape_ok(65, 128, 8, 0.1, fused_dropout=True)
    assert not T.attn_shape_ok(6, 128, 8, 1.0, fused_dropout=True)


def test_fused_dropout_flag_and_agent_state_dict():
    """--fused-dropout parses; the generator state is no buffer, so the state-dict keys stay the
    reference's."""
    from oc_cleanrl_amd import transformer as T
    from oc_cleanrl_amd.agents import EnvSpec
    from oc_cleanrl_amd.args import parse_dataclass

    a = parse_dataclass(T.TransformerArgs, ["--fused-dropout"], None, "t")
    assert a.fused_dropout is True and a.dropout == 0.1
    mk = lambda fd: T.OCTransformerAgent(EnvSpec((6, 8), 4), 32, 4, 2, True, 3, None,  # noqa: E731
                                         dropout=0.1, fused_dropout=fd, seed=7)
    on, off = mk(True), mk(False)
    assert on.fused_dropout and not off.fused_dropout and on.rng is None
    assert list(on.state_dict()) == list(off.state_dict())
    assert not list(on.buffers())


def test_dropout_argument_validation_needs_no_gpu():
    from oc_cleanrl_amd import ops

    assert ops.dropout_consts(0.1) == (du.threshold(0.1), 1.0 / 0.9)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="not in"):
            ops.dropout_consts(bad)
    assert ops.mha_dropout_shape_ok(6, 128, 8) and not ops.mha_dropout_shape_ok(65, 128, 8)
