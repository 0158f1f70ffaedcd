"""numpy restatement of the training step's dropout generator (csrc/eec_drop.h, csrc/eec_train.h).

TEST INFRASTRUCTURE -- see oracle/__init__.py for who may import this.

The generator is counter-based: element ``i`` of the tensor a site masks is kept when

    lowbias32(lo(i) * C1 + hi(i) * C2 + key(seed, site)) >= thr(p)

with ``key`` a splitmix64-style mix of the 64-bit seed and the 32-bit site number folded to 32 bits, ``thr(p) = floor(p * 2^32)``
for the fp32 value of ``p`` (saturated at 2^32 - 1), and kept values scaled by ``1 / (1 - p)`` in fp32.  ``i`` is the flat
row-major index of the site's natural tensor ([B, T', D], [B, T', F], [B H, T', T'], [n_tok, D]).  Only the per-element form is
stated here: the device's four-at-a-time shortcuts have to equal it, which is what the tests check.
"""
from __future__ import annotations

import numpy as np

_M64 = (1 << 64) - 1
_C1, _C2 = np.uint32(0x9E3779B1), np.uint32(0x85EBCA77)


def drop_key(seed: int, site: int) -> int:
    """32-bit key of (seed, site): two xor-shift-multiply rounds over seed * golden ratio + (site, site), halves xor-ed."""
    seed, site = int(seed) & _M64, int(site) & 0xFFFFFFFF
    x = (seed * 0x9E3779B97F4A7C15 + ((site << 32) | site)) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return ((x >> 32) ^ x) & 0xFFFFFFFF


def drop_thr(p: float) -> int:
    """Keep threshold of probability ``p`` (taken as fp32, as the C ABI passes it): floor(p * 2^32), at most 2^32 - 1."""
    t = float(np.float32(p)) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def inv_keep(p: float) -> np.float32:
    """The multiplier of a kept element: 1 / (1 - p) rounded as the device computes it, in fp32."""
    p32 = np.float32(p)
    return np.float32(1.0) / (np.float32(1.0) - p32) if p32 > 0 else np.float32(1.0)


def drop_hash(key: int, index: np.ndarray) -> np.ndarray:
    """lowbias32 of the keyed element index (uint64 array) -> uint32 array."""
    i = np.asarray(index, dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = (i & np.uint64(0xFFFFFFFF)).astype(np.uint32) * _C1 + (i >> np.uint64(32)).astype(np.uint32) * _C2 + np.uint32(key)
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x7FEB352D)
        h ^= h >> np.uint32(15)
        h *= np.uint32(0x846CA68B)
        h ^= h >> np.uint32(16)
    return h


def keep_mask(seed: int, site: int, p: float, n: int, start: int = 0) -> np.ndarray:
    """bool[n]: which of the elements start .. start + n - 1 of site ``site`` survive dropout of probability ``p`` under ``seed``."""
    if np.float32(p) <= 0:
        return np.ones(n, dtype=bool)
    index = np.arange(n, dtype=np.uint64) + np.uint64(start)
    return drop_hash(drop_key(seed, site), index) >= np.uint32(drop_thr(p))
