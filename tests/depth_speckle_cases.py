"""Inputs the CPU and the GPU tests of dmi_filter_depth_speckles share: the pairs of neighbouring depths that sit
exactly on the definition's tolerance, and small random images."""
import numpy as np

# (Da, Db, abs_tolerance, rel_tolerance, linked).  The first four are dyadic numbers: every operation is exact.
#   4.0 | 4.5      |Da - Db| = 0.5 against abs 0.5: <= holds at equality; not at the next f64 below 0.5
#   4.0 | 4.5      rel 0.125 of fmin = 4.0 is 0.5: linked
#   4.0 | 4.53125  rel 0.125 of fmin = 4.0 is 0.5 < 0.53125: not linked; of the LARGER depth it would be 0.56640625 and link
# The last pair was found by a search in exact rational arithmetic: abs + rel * min rounded as a product and then a sum is
# 0x1.1525cc388d4a0p+1, the difference itself; a contracted multiply-add rounds once, to 0x1.1525cc388d49fp+1, and would not link.
FMA_PAIR = (float.fromhex("0x1.7f80000000000p+3"), float.fromhex("0x1.c4c9730e23528p+3"), float.fromhex("0x1.7300000000000p-1"),
            float.fromhex("0x1.ec5e400179430p-4"), True)
TIE_PAIRS = (
    (4.0, 4.5, 0.5, 0.0, True),
    (4.0, 4.5, float(np.nextafter(0.5, 0.0)), 0.0, False),
    (4.0, 4.5, 0.0, 0.125, True),
    (4.0, 4.53125, 0.0, 0.125, False),
    FMA_PAIR,
)


def random_levels(rng, n, H, W, valid_share=0.8):
    """[n, H, W]: two depth levels (2.0 and 3.0) in random blocks of 1 to 4 pixels, with random holes of -1."""
    out = np.empty((n, H, W))
    for m in range(n):
        step = int(rng.integers(1, 5))
        coarse = rng.random((H // step + 1, W // step + 1)) < 0.5
        level = np.repeat(np.repeat(coarse, step, axis=0), step, axis=1)[:H, :W]
        out[m] = np.where(level, 2.0, 3.0)
        out[m][rng.random((H, W)) >= valid_share] = -1.0
    return out


def random_blobs(rng, n, H, W):
    """[n, H, W]: a sloped background with random discs at depths of their own, some valid pixels knocked out."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((n, H, W))
    for m in range(n):
        d = 5.0 + 0.004 * xx + 0.003 * yy
        for _ in range(int(rng.integers(5, 40))):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(1, 9)
            d = np.where((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r, rng.uniform(2.0, 9.0), d)
        d[rng.random((H, W)) < 0.05] = -1.0
        out[m] = d
    return out
