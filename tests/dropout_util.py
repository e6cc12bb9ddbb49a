"""The dropout mask of the fused transformer path restated in numpy: Philox4x32-10
(Salmon et al. 2011, the Random123 constants) and the two element -> (block, component) layouts.

A launch has a generator state (seed, offset), a site in [0, 256) and a threshold
thr = min(int(p * 2^32), 2^32 - 1). The word of an element is a component of the Philox block with
counter (lo32 blk, hi32 blk, lo32 sub, hi32 sub), key (lo32 seed, hi32 seed), sub = offset * 256 +
site; the element is kept iff word >= thr. No float takes part in the decision.
"""
from __future__ import annotations

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
ATTN_MAX_S = 64


def philox4x32_10(counter, key) -> np.ndarray:
    """counter: four arrays (or ints) of 32-bit words, broadcast together; key: two ints.
    Returns uint32 [..., 4]."""
    c = [np.asarray(x, dtype=np.uint64) & MASK32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def philox_blocks(seed: int, offset: int, site: int, blk) -> np.ndarray:
    """The blocks `blk` (uint64 array) of the launch (seed, offset, site): uint32 [..., 4]."""
    assert 0 <= site < 256
    sub = (int(offset) * 256 + int(site)) & 0xFFFFFFFFFFFFFFFF
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    blk = np.asarray(blk, dtype=np.uint64)
    return philox4x32_10((blk & MASK32, blk >> np.uint64(32), sub & 0xFFFFFFFF, sub >> 32),
                         (seed & 0xFFFFFFFF, seed >> 32))


def threshold(p: float) -> int:
    return min(int(p * 2 ** 32), 2 ** 32 - 1)


def scale_f32(p: float) -> np.float32:
    """1 / (1 - p) in double, rounded to f32 once (what the kernels multiply by)."""
    return np.float32(1.0 / (1.0 - p))


def words_elementwise(seed: int, offset: int, site: int, n: int) -> np.ndarray:
    """uint32 [n]: flat index e -> block e >> 2, component e & 3."""
    nblk = (n + 3) // 4
    return philox_blocks(seed, offset, site, np.arange(nblk, dtype=np.uint64)).reshape(-1)[:n]


def words_attention(seed: int, offset: int, site: int, B: int, H: int, S: int) -> np.ndarray:
    """uint32 [B, H, S, S] (query i, key j): block ((b * H + h) * 64 + i) * 16 + (j >> 2),
    component j & 3 -- independent of S."""
    assert 1 <= S <= ATTN_MAX_S
    bh = np.arange(B * H, dtype=np.uint64).reshape(B, H, 1, 1)
    i = np.arange(S, dtype=np.uint64).reshape(1, 1, S, 1)
    jb = np.arange((S + 3) // 4, dtype=np.uint64).reshape(1, 1, 1, -1)
    blk = (bh * np.uint64(ATTN_MAX_S) + i) * np.uint64(ATTN_MAX_S // 4) + jb
    w = philox_blocks(seed, offset, site, blk)  # [B, H, S, ceil(S / 4), 4]
    return w.reshape(B, H, S, -1)[..., :S]


def keep_elementwise(seed, offset, site, n, p) -> np.ndarray:
    """bool [n]"""
    return words_elementwise(seed, offset, site, n) >= np.uint32(threshold(p))


def keep_attention(seed, offset, site, B, H, S, p) -> np.ndarray:
    """bool [B, H, S, S]"""
    return words_attention(seed, offset, site, B, H, S) >= np.uint32(threshold(p))
