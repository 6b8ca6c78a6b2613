"""The planted cases shared by tests/test_tmalign_cpu.py and tests/test_tmalign.py, with the yardstick's results computed once.

A case is (Lx, Ly, core fraction, mirrored, seed).  The seed of a case is the first of its three CANDIDATES (1000 k + 0, 1, 2 for case
number k) at which the yardstick returns the same mapping with its DP score matrices rounded to float32 as in float64 (otherwise a
near-tie of the discrete DP decides the result and fp32 may fall on either side).  KEPT records which candidate that is; the CPU test
recomputes the rule for every kept case and holds the dropped candidates to at most 1 in 10."""
import functools

import numpy as np

import align_ref as AR
import tmalign_ref as TR

SHAPES = [(5, 5), (5, 40), (40, 5), (63, 64), (64, 65), (65, 63), (130, 97), (257, 255), (320, 300)]
FRACTIONS = [1.0, 0.6, 0.35]
# candidate index kept per case, in the order of CASES (0: the first candidate passed the float32 rule)
KEPT = [0, 0, 0, 0, 0, 0, 0, 0, 0]
CASES = [(Lx, Ly, FRACTIONS[k % 3], k % 4 == 3, 1000 * k + KEPT[k]) for k, (Lx, Ly) in enumerate(SHAPES)]
# a diagonal longer than the workgroup's 512 rows on either side of 512 and of 1024 rows (the DP gives a thread 1, 2 and 3 rows);
# candidates 20000 + 1000 k + 0, 1, 2, kept by the same float32 rule
LONG_SHAPES = [(500, 530), (530, 500), (1010, 1040), (1040, 1010)]
LONG_KEPT = [0, 0, 0, 0]
LONG_CASES = [(Lx, Ly, 1.0, k == 3, 20000 + 1000 * k + LONG_KEPT[k]) for k, (Lx, Ly) in enumerate(LONG_SHAPES)]


@functools.lru_cache(maxsize=None)
def planted_case(Lx, Ly, frac, mirrored, seed):
    """float32-rounded compacted inputs as float64, the planted transform and mapping"""
    rng = np.random.default_rng(seed)
    x, y, R0, t0, amap = TR.planted(rng, Lx, Ly, frac, mirrored=mirrored)
    x, y = x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    return dict(x=x, y=y, R0=R0, t0=t0, mapping=amap, planted_tm=TR.score_of(x, y, amap, R0, t0)[0])


@functools.lru_cache(maxsize=None)
def yardstick(Lx, Ly, frac, mirrored, seed, f32_scores=False):
    c = planted_case(Lx, Ly, frac, mirrored, seed)
    return TR.align(c["x"], c["y"], mirror=True, f32_scores=f32_scores)
