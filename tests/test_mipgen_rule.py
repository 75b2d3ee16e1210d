"""Mip rule M2-M4 (device option generate_mipmaps; csrc/mipgen.hip) as restated in tests/mipgen_rule.py, checked on the CPU against
float64 exact area averages and the level table, so that the GPU tests can hold the kernel to it bit for bit."""
import numpy as np
import pytest

import mipgen_rule as R


def _overlap_weights(s):
    """[d, s] float64: the fraction of destination texel x's footprint that source texel i covers (exact area average, no rule involved)."""
    d = max(1, s >> 1)
    W = np.zeros((d, s))
    for x in range(d):
        a, b = x * s / d, (x + 1) * s / d
        for i in range(int(np.floor(a)), min(s, int(np.ceil(b)))):
            W[x, i] = max(0.0, min(b, i + 1) - max(a, i))
        W[x] /= W[x].sum()
    return W


def _exact(src):
    sh, sw = src.shape[:2]
    Wy, Wx = _overlap_weights(sh), _overlap_weights(sw)
    return np.einsum("yj,jic,xi->yxc", Wy, src.astype(np.float64), Wx)


@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (1, 7), (7, 1), (3, 3), (3, 5), (5, 7), (33, 17), (64, 32), (64, 64), (127, 129), (100, 60), (9, 9), (12, 4)])
def test_every_level_is_the_rounded_exact_area_average_of_the_quantised_level_before(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    levels = R.chain(img)
    assert [l.shape[:2] for l in levels] == [(lh, lw) for lw, lh in R.level_sizes(w, h)]
    ties = 0
    for prev, cur in zip(levels, levels[1:]):
        ex = _exact(prev)
        diff = cur.astype(np.float64) - ex
        assert np.abs(diff).max() <= 0.5 + 1e-9
        tie = np.abs(np.abs(diff) - 0.5) < 1e-9
        assert np.all(diff[tie] > 0), "a tie rounded down"         # ties round up
        ties += int(tie.sum())
    if w * h >= 64 and w % 2 == 0 and h % 2 == 0:
        assert ties > 0                                              # the even x even path meets ties (a + b + c + d = 4k + 2) and rounds them up


def test_power_of_two_levels_are_the_four_texel_mean_rounded_up():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (64, 128, 4), dtype=np.uint8)
    l1 = R.next_level(img)
    s = img.astype(np.int32)
    assert np.array_equal(l1, (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2)
    # a 2 x 1 source takes the general path ((1, 1) / 2 along x, (1) / 1 along y): the pair's mean, ties up
    two = np.array([[[1, 2, 3, 4], [2, 3, 4, 5]]], dtype=np.uint8)
    assert np.array_equal(R.next_level(two), np.array([[[2, 3, 4, 5]]], dtype=np.uint8))


@pytest.mark.parametrize("w,h,count", [(1, 1, 1), (1, 7, 3), (7, 1, 3), (3, 5, 3), (64, 32, 7), (4096, 4096, 13), (1000, 600, 10), (65536, 1, 16), (1, 65536, 16), (2, 2, 2)])
def test_level_table(w, h, count):
    assert R.level_count(w, h) == count
    sizes = R.level_sizes(w, h)
    assert len(sizes) == count and sizes[0] == (w, h)
    for m, (lw, lh) in enumerate(sizes):
        assert (lw, lh) == (max(1, w >> m), max(1, h >> m))
    if count < R.MAX_MIPS:
        assert sizes[-1] == (1, 1)
    else:
        assert sizes[-1] == (2, 1) if w > h else (1, 2)


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (64, 64), (127, 31), (1, 9)])
def test_a_constant_texture_stays_constant(w, h):
    colour = np.array([17, 200, 255, 3], dtype=np.uint8)
    img = np.broadcast_to(colour, (h, w, 4)).copy()
    for l in R.chain(img):
        assert np.all(l == colour)


@pytest.mark.parametrize("w,h", [(64, 64), (33, 17), (127, 129), (1, 255)])
def test_every_level_keeps_level_0_alpha_bounds(w, h):
    """M5: minAlpha / maxAlpha of level 0 bound every level (opacity rules O1 / O2 keep using them)."""
    rng = np.random.default_rng(w + 7 * h)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = rng.integers(37, 201, (h, w), dtype=np.uint8)
    lo, hi = img[..., 3].min(), img[..., 3].max()
    for l in R.chain(img):
        assert l[..., 3].min() >= lo and l[..., 3].max() <= hi


def test_odd_weights_sum_to_the_divisor_and_are_the_exact_overlaps():
    for s in range(3, 1000, 2):
        taps, wts, D = R.axis_taps(s)
        assert D == s
        assert np.all(wts.sum(axis=1) == s)
        assert taps.max() == s - 1 and taps.min() == 0                   # every tap inside the level
        if s <= 201:
            W = np.zeros((s >> 1, s))
            for k in range(3):
                np.add.at(W, (np.arange(s >> 1), taps[:, k]), wts[:, k])
            assert np.allclose(W / s, _overlap_weights(s), atol=1e-12)
    for s in (2, 4, 6, 1000):
        taps, wts, D = R.axis_taps(s)
        assert D == 2 and np.all(wts.sum(axis=1) == 2) and taps.max() == s - 1


def test_large_odd_levels_use_exact_integers():
    """A 4101-tall odd level (Dy = 4101): the integer weights stay exact area averages far from the small sizes above."""
    rng = np.random.default_rng(5)
    col = rng.integers(0, 256, (4101, 1, 4), dtype=np.uint8)
    img = np.repeat(col, 5, axis=1)[:, :5]                                 # 5 wide keeps the test small; the height carries Dy = 4101
    l1 = R.next_level(img)
    ex = _exact(img)
    assert np.abs(l1 - ex).max() <= 0.5 + 1e-9


def test_dds_packer_layout():
    levels = R.chain(np.arange(6 * 10 * 4, dtype=np.uint8).reshape(6, 10, 4))
    raw = R.dds_rgba8(levels)
    assert bytes(raw[:4]) == b"DDS "
    u32 = lambda o: int.from_bytes(bytes(raw[o:o + 4]), "little")
    assert (u32(12), u32(16), u32(28)) == (6, 10, len(levels)) == (6, 10, 4)
    assert bytes(raw[84:88]) == b"DX10" and u32(128) == R.DXGI_R8G8B8A8_UNORM
    assert raw.size == 148 + sum(l.nbytes for l in levels)
    assert np.array_equal(raw[148:148 + 240].reshape(6, 10, 4), levels[0])
