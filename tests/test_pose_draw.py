"""CPU tests of the pose-refinement reference (tests/pose_reference.py): its counter RNG is the oracle's, and its pixel draw (k_pose_rays, stated in
include/mon_core.h) keeps the 24-bit stream up to 2^24 pixels and reaches every pixel of a union of up to 2^28 above."""
import numpy as np
import pytest

import pose_reference as pref

FRAME = 240 * 320
TOTALS_SMALL = (1, 3, 4097, 12289, FRAME, 1 << 23, (1 << 24) - 1, 1 << 24)
TOTALS_LARGE = ((1 << 24) + 1, 256 * FRAME, (1 << 27) + 12345, pref.MAX_UNION)


@pytest.mark.parametrize("stream", [3, 4, 5])
def test_rand01_equals_oracle(orc, stream):
    L = orc.lib()
    steps = [0, 1, 7, 4095, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 0x9E3779B9]
    idx = [0, 1, 63, 64, 4095 * 64 + 63, (1 << 22) * 64 - 1, 1 << 27, (1 << 28) - 1, 0x0ABCDEF, 0x5555555,
           12345, 99999, 1 << 20, (1 << 28) - 64, 777777, 31, 32, 100, 1000, 10000]
    n = 0
    for seed in (1, 5, 0xFFFFFFFFFFFFFFFF):
        for step in steps[:len(steps) if seed == 1 else 3]:
            got = pref.rand01(seed, stream, step, np.array(idx, np.uint64))
            want = np.array([L.orc_rand01(seed, stream, step, i) for i in idx], np.float32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (seed, stream, step)
            n += len(idx)
    assert n >= 160


def test_rand01_is_the_mix_top_24_bits():
    z = pref.rand_mix(1, 5, 7, np.arange(1 << 16, dtype=np.uint64))
    u = pref.rand01(1, 5, 7, np.arange(1 << 16, dtype=np.uint64))
    # k_pose_rays before the fix: u24 = (uint32_t)(rand01 * 16777216.0f), exact in fp32
    assert np.array_equal((u * np.float32(16777216.0)).astype(np.uint64), z >> np.uint64(40))


@pytest.mark.parametrize("total", TOTALS_SMALL)
def test_draw_up_to_2_24_is_the_24_bit_stream(total):
    for seed, it in ((1, 0), (1, 7), (3, 99), (0xDEADBEEF, (1 << 32) - 1)):
        p = pref.draw(seed, it, 1 << 14, total)
        assert np.array_equal(p, pref.draw24(seed, it, 1 << 14, total)), (total, seed, it)
        assert p.max() < total
    # every pixel is reachable with 24 bits up to 2^24: consecutive u24 move the pixel by total / 2^24 <= 1
    q = np.unique(np.linspace(0, total - 1, 4097).astype(np.uint64))
    assert pref.reachable24(q, total).all()


@pytest.mark.parametrize("total", TOTALS_LARGE)
def test_draw_above_2_24_reaches_every_pixel(total):
    """p(u) = (u total) >> 32 for the 32-bit u = z >> 32: p(0) = 0, p(2^32 - 1) = total - 1, and since total <= 2^28 < 2^32,
    p(u + 1) - p(u) = floor((u + 1) total / 2^32) - floor(u total / 2^32) <= ceil(total / 2^32) = 1: consecutive draw values never skip a pixel, so every
    pixel of [0, total) is the draw of some u.  Checked at the ends, at every pixel boundary of a sample of pixels, and on the draws of the stream."""
    T = np.uint64(total); S = np.uint64(32)
    f = lambda u: (np.asarray(u, np.uint64) * T) >> S                                   # noqa: E731
    assert total <= pref.MAX_UNION < 1 << 32
    assert f(0) == 0 and f((1 << 32) - 1) == total - 1
    q = np.unique(np.linspace(1, total - 1, 1 << 16).astype(np.uint64))
    u = ((q << S) + T - np.uint64(1)) // T                                              # the smallest u with p(u) >= q
    assert (u < np.uint64(1 << 32)).all() and np.array_equal(f(u), q) and np.array_equal(f(u - np.uint64(1)), q - np.uint64(1))
    # the stream: its top 24 bits are the old u24, so the wider draw lands at most (u32 mod 2^8) total / 2^32 < total / 2^24 pixels past the old one
    z = pref.rand_mix(1, 5, 7, np.arange(1 << 16, dtype=np.uint64))
    p = pref.draw(1, 7, 1 << 16, total); old = pref.draw24(1, 7, 1 << 16, total)
    assert np.array_equal(p, f(z >> S)) and p.max() < total
    assert (p >= old).all() and ((p - old) <= np.uint64(-(-total // (1 << 24)))).all()


def test_24_bit_draw_misses_pixels_of_a_large_union():
    """The draw before the fix over 256 boxes naming one 240 x 320 frame: only 2^24 of the 19 660 800 pixels can be drawn (85.33 %)."""
    total = 256 * FRAME
    r = pref.reachable24(np.arange(total, dtype=np.uint64), total)
    print("24-bit draw over %d px: %.4f %% reachable" % (total, 100 * r.mean()))
    assert r.sum() == 1 << 24
    p = pref.draw(1, 0, 4096, total)
    miss = ~pref.reachable24(p, total)
    print("fixed draw, 4096 rays: %d land where the 24-bit draw cannot" % miss.sum())
    assert 400 <= miss.sum() <= 800                                   # ~14.7 % of uniform draws
