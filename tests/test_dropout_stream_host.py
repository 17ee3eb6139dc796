"""CPU: statistics of the dropout stream, on its host statement (tests/drop_ref.py; tests/test_gpu_dropout_stream.py requires the device's
masks to equal it exactly). A hash that is biased in some column or row, or whose four sites or whose slides are correlated, would change
training silently: no comparison of a kernel with masks exported by the same hash can notice."""
import numpy as np
from scipy.stats import binom

from tests import drop_ref

P_KEEP = 0.75
ROWS = 4096
WIDTHS = (("h1", 512), ("h", 512), ("a", 384), ("b", 384))


def _two_sided(k, n, p):
    """Exact two-sided binomial p-value of each count k of n trials: twice the smaller exact tail, capped at 1."""
    k = np.asarray(k, dtype=np.int64)
    return np.minimum(1.0, 2.0 * np.minimum(binom.cdf(k, n, p), binom.sf(k - 1, n, p)))


def _stats_of_seed(seed):
    s = dict(zip(("h1", "h", "a", "b"), drop_ref.drop_seeds(seed)))
    kept = {k: drop_ref.keep(ROWS * w, 0.25, s[k]).reshape(ROWS, w) != 0 for k, w in WIDTHS}
    a_slide1 = drop_ref.keep(ROWS * 384, 0.25, (s["a"] + 2 * drop_ref.GOLDEN) & drop_ref.M64).reshape(ROWS, 384) != 0
    pv = []
    for k, w in WIDTHS:
        m = kept[k]
        pv.append(_two_sided([m.sum()], m.size, P_KEEP))                        # the whole mask
        pv.append(_two_sided(m.sum(0), ROWS, P_KEEP))                           # every column
        pv.append(_two_sided(m.sum(1), w, P_KEEP))                              # every row
        # neighbours, as DISJOINT pairs (columns 2j, 2j + 1; rows 2i, 2i + 1): the both-kept indicators of overlapping pairs would share
        # elements and their count would not be binomial
        pv.append(_two_sided([(m[:, 0::2] & m[:, 1::2]).sum()], m.size // 2, P_KEEP ** 2))
        pv.append(_two_sided([(m[0::2] & m[1::2]).sum()], m.size // 2, P_KEEP ** 2))
    for u, v in ((kept["h1"], kept["h"]), (kept["a"], kept["b"]), (kept["h1"][:, :384], kept["a"]), (kept["a"], a_slide1)):
        pv.append(_two_sided([(u & v).sum()], u.size, P_KEEP ** 2))             # two streams at equal positions
    return np.concatenate(pv)


def test_stream_shows_no_bias_and_no_correlation():
    """Eight seeds (the first eight of default_rng(0).integers(0, 2**62)), 4096 rows, the four sites' streams at their widths 512, 512, 384,
    384. Exact two-sided binomial p-values of: the kept count of each mask, of each of its columns and each of its rows against 0.75; the
    both-kept count of horizontally and of vertically adjacent elements (disjoint pairs) against 0.5625; the both-kept count at equal
    positions of (h1, h), (a, b), (h1[:, :384], a) and (a of slide 0, a of slide 1: seeds 2 GOLDEN apart) against 0.5625. 18,192 statistics
    per seed, 145,536 in all; the condition is Bonferroni's: min p x count >= 1e-3. Under the hypothesis that the stream is fair, min p x
    count is below 1e-3 once in a thousand; a stream with any structure at these scales misses it by many orders (a column kept 80 % of the
    time has p ~ 1e-13). Deterministic; this stream gives min p x count = 0.0578 (computed here on the CPU), a factor of 58 inside the bound."""
    seeds = [int(s) for s in np.random.default_rng(0).integers(0, 2 ** 62, size=8)]
    pv = np.concatenate([_stats_of_seed(s) for s in seeds])
    assert pv.size == 145536
    worst = float(pv.min()) * pv.size
    print(f"min p x count = {worst:.4g} over {pv.size} statistics")
    assert worst >= 1e-3, worst


def test_the_statistics_notice_structure():
    """The same p-values on broken streams: a hash that ignores the high half of the seed makes two sites' masks equal, one that drops the
    low index bit makes horizontal neighbours equal, a threshold of 0.26 x 2^32 shifts every count."""
    n = ROWS * 512
    m = (drop_ref.keep(n, 0.25, 7) != 0).reshape(ROWS, 512)
    assert _two_sided([(m & m).sum()], n, P_KEEP ** 2)[0] < 1e-100                                  # two equal streams
    pair = (drop_ref.drop_hash(np.arange(n, dtype=np.uint64) >> np.uint64(1), 7) >= drop_ref.threshold(0.25)).reshape(ROWS, 512)
    assert _two_sided([(pair[:, 0::2] & pair[:, 1::2]).sum()], n // 2, P_KEEP ** 2)[0] < 1e-100
    off = drop_ref.keep(n, 0.26, 7) != 0
    assert _two_sided([off.sum()], n, P_KEEP)[0] < 1e-100


def test_twin_follows_the_definition():
    """What drop_ref states, checked on a few values worked out by hand from toad_amd/csrc/common.h: thresholds (p rounded to fp32 first),
    the scale in fp32, p == 0 meaning off, 64-bit seeds and indices entering through both halves, and the seed arithmetic modulo 2^64."""
    assert drop_ref.threshold(0.25) == 1 << 30 and drop_ref.threshold(0.5) == 1 << 31
    assert drop_ref.threshold(0.1) == int(float(np.float32(0.1)) * 2 ** 32) == 429496736          # fp32(0.1) = 0.100000001490116...
    assert drop_ref.threshold(0.1) != int(0.1 * 2 ** 32)
    assert set(np.unique(drop_ref.keep(4096, 0.25, 3))) == {np.float32(0.0), np.float32(1.0) / np.float32(0.75)}
    assert set(np.unique(drop_ref.keep(4096, 0.1, 3))) == {np.float32(0.0), np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))}
    assert np.array_equal(drop_ref.keep(100, 0.0, 3), np.ones(100, np.float32))

    def by_hand(idx, seed):                                    # python integers, masked to 32 bits after every step
        m = 0xFFFFFFFF
        x = (idx & m) ^ (seed & m); y = (idx >> 32) ^ (seed >> 32)
        x = x * 0x9E3779B1 & m; x ^= x >> 15; x = (x + y * 0x85EBCA77) & m
        x = x * 0xC2B2AE3D & m; x ^= x >> 13; x = x * 0x27D4EB2F & m; x ^= x >> 16
        return x
    for idx in (0, 1, 63, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 33 + 5):
        for seed in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 62 - 1, 2 ** 64 - 1):
            assert int(drop_ref.drop_hash(np.array([idx], dtype=np.uint64), seed)[0]) == by_hand(idx, seed), (idx, seed)
    # the high halves matter: same low words, different streams
    assert not np.array_equal(drop_ref.drop_hash(np.arange(64, dtype=np.uint64), 5), drop_ref.drop_hash(np.arange(64, dtype=np.uint64), 5 + 2 ** 32))
    s = drop_ref.drop_seeds(2 ** 64 - 1)
    assert s == tuple(((2 ** 64 - 1) + (i + 1) * 0x9E3779B97F4A7C15) % 2 ** 64 for i in range(4)) and len(set(s)) == 4
