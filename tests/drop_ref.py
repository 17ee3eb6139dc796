"""TEST INFRASTRUCTURE ONLY - host statement of the stateless dropout stream, written from its definition in toad_amd/csrc/common.h
(drop_hash, make_drop, drop_keep) and toad_amd/functional.py (drop_seeds). numpy, with uint32 / uint64 wrap-around; it does not import the
product package, so a change to the hash, the threshold or the seed handling there moves the device and not this file.

    keep(element) = hash(seed, flat element index) >= p * 2^32 ;  kept values carry 1 / (1 - p), dropped ones 0.
"""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15             # the stream step: site i of a forward draws from seed + (i + 1) * GOLDEN
M64 = 0xFFFFFFFFFFFFFFFF


def drop_hash(idx, seed: int) -> np.ndarray:
    """uint32 hash of the 64-bit flat element index ``idx`` (array) under the 64-bit ``seed``: both halves of each enter it."""
    idx = np.asarray(idx, dtype=np.uint64)
    seed = int(seed) & M64
    u32 = np.uint32
    x = (idx & np.uint64(0xFFFFFFFF)).astype(u32) ^ u32(seed & 0xFFFFFFFF)
    y = (idx >> np.uint64(32)).astype(u32) ^ u32(seed >> 32)
    with np.errstate(over="ignore"):
        x = x * u32(0x9E3779B1); x = x ^ (x >> u32(15)); x = x + y * u32(0x85EBCA77)
        x = x * u32(0xC2B2AE3D); x = x ^ (x >> u32(13)); x = x * u32(0x27D4EB2F); x = x ^ (x >> u32(16))
    return x


def threshold(p: float) -> int:
    """p * 2^32 as make_drop forms it: p arrives as a float (0.1 is rounded to fp32 first), is widened to double, scaled and truncated."""
    return int(np.uint32(np.float64(np.float32(p)) * 4294967296.0))


def keep(n: int, p: float, seed: int) -> np.ndarray:
    """The first n multipliers of the stream (float32): 0 where dropped, float32(1 / (1 - float32(p))) where kept; p == 0 means dropout is off."""
    if not np.float32(p) > 0:
        return np.ones(n, dtype=np.float32)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    kept = drop_hash(np.arange(n, dtype=np.uint64), seed) >= np.uint32(threshold(p))
    return np.where(kept, scale, np.float32(0.0)).astype(np.float32)


def drop_seeds(seed: int):
    """The four streams of one forward: trunk layer 1, trunk layer 2, tanh branch, sigmoid branch. Slide b of a batch draws its two
    branch masks from the branch seeds + 2 b GOLDEN."""
    return tuple((int(seed) + (i + 1) * GOLDEN) & M64 for i in range(4))
