"""Sharpening rule S1-S7 (RT64_VIEW_DESC.upscalerSharpness; csrc/upscale.hip) as restated in tests/sharpen_rule.py, checked on the CPU:
hand-made images with known answers, the clamp at the borders, strength that rises with the field, the float32 form against the float64 form within
the bound the rule file derives, and no subnormal intermediates on the images the GPU test compares bit for bit (tests/test_gpu_sharpen.py)."""
from fractions import Fraction

import numpy as np
import pytest

import sharpen_rule as R

W, H = 320, 180
STRENGTHS = (0.25, 0.5, 0.75, 1.0)


def _rgba(rgb, alpha=1.0):
    rgb = np.asarray(rgb, dtype=np.float32)
    if rgb.ndim == 2:
        rgb = np.repeat(rgb[..., None], 3, axis=2)
    return np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), alpha, dtype=np.float32)], axis=2)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def random_image():
    return np.random.default_rng(20261017).random((48, 64, 4), dtype=np.float32)


@pytest.fixture(scope="module")
def oracle_upscaled(sample_data):
    """The oracle's `upscaled` image of the sample scene behind the FSR slot in quality mode, after 8 frames."""
    from oracle import oracle_py
    o = oracle_py.OracleScene(sample_data)
    try:
        for _ in range(8):
            r = o.render(W, H, upscaler=3, upscalerMode=4)
    finally:
        o.close()
    up = r["upscaled"]
    assert up.shape == (H, W, 4) and up.dtype == np.float32
    return up


# ---- 1. hand-made images ---------------------------------------------------------------------------------------------------------

def test_strength_is_two_to_the_minus_stops():
    assert R.strength(1.0) == np.float32(1.0) and R.strength(0.5) == np.float32(0.5) and R.strength(2.0) == np.float32(1.0)
    assert R.strength(0.25) == np.float32(2.0 ** -1.5) and R.strength(1e-30) == np.float32(0.25)
    assert R.strength(0.0) is None and R.strength(-0.5) is None and R.strength(float("nan")) is None


@pytest.mark.parametrize("s", [0.01, 0.25, 0.5, 1.0, 3.0])
@pytest.mark.parametrize("value", [0.0, 0.2, 0.5, 1.0])
def test_a_constant_image_is_returned_unchanged(s, value):
    img = _rgba(np.full((5, 7), value), alpha=3.0)
    out, mask = R.rcas_f32(img, s)
    # unchanged in exact arithmetic: (lobe 4 v + v) / (4 lobe + 1) = v; the two forms round, each within its precision
    assert np.abs(R.rcas_f64(img, s) - img[..., :3].astype(np.float64)).max() < 1e-15
    assert np.abs(out[..., :3].astype(np.float64) - img[..., :3]).max() <= R.BOUND and not mask.any()
    assert np.array_equal(_bits(out[..., 3]), _bits(img[..., 3]))
    if value in (0.0, 0.5, 1.0):                 # numerator and denominator are then 1 : 2, 1 : 1 or 0 : 1 to the bit
        assert np.array_equal(_bits(out), _bits(img))


def test_a_pixel_whose_four_neighbours_equal_it_is_unchanged(random_image):
    img = random_image[:9, :9].copy()
    for c in range(3):
        img[3, 4, c] = img[5, 4, c] = img[4, 3, c] = img[4, 5, c] = img[4, 4, c] = np.float32(0.1 + 0.3 * c)
    out, _ = R.rcas_f32(img, 1.0)
    assert np.abs(out[4, 4, :3].astype(np.float64) - img[4, 4, :3]).max() <= R.BOUND and out[4, 4, 3] == img[4, 4, 3]
    assert np.abs(R.rcas_f64(img, 1.0)[4, 4] - img[4, 4, :3].astype(np.float64)).max() < 1e-15


def _by_hand(b, d, e, f, h, k):
    """S3-S5 of a grey pixel in exact rationals."""
    b, d, e, f, h, k = (v if isinstance(v, Fraction) else Fraction(float(v)) for v in (b, d, e, f, h, k))
    mn, mx = min(b, d, f, h), max(b, d, f, h)
    hit_min = Fraction(0) if mx == 0 else min(mn, e) / (4 * mx)
    hit_max = Fraction(0) if mn == 1 else (1 - max(mx, e)) / (4 * mn - 4)
    lobe = max(Fraction(-3, 16), min(max(-hit_min, hit_max), Fraction(0))) * k
    return min(max((lobe * (b + d + f + h) + e) / (4 * lobe + 1), Fraction(0)), Fraction(1))


def test_a_vertical_step_edge_gives_the_values_worked_out_by_hand():
    grey = np.full((5, 6), 0.25); grey[:, 3:] = 0.75
    img = _rgba(grey, alpha=7.0)
    lo, hi = Fraction(1, 4), Fraction(3, 4)
    left = _by_hand(lo, lo, lo, hi, lo, 1)           # the 0.25 pixel at the edge: lobe -1/12, (-1/8 + 1/4) / (2/3)
    right = _by_hand(hi, lo, hi, hi, hi, 1)          # the 0.75 pixel at the edge: lobe -1/12, (-5/24 + 3/4) / (2/3)
    assert (left, right) == (Fraction(3, 16), Fraction(13, 16))
    expect = grey.copy(); expect[:, 2] = float(left); expect[:, 3] = float(right)
    f64 = R.rcas_f64(img, 1.0)
    assert np.abs(f64 - expect[..., None]).max() < 1e-15
    out, mask = R.rcas_f32(img, 1.0)
    assert np.abs(out[..., :3].astype(np.float64) - expect[..., None]).max() <= R.BOUND and not mask.any()
    assert np.array_equal(_bits(out[..., 3]), _bits(img[..., 3]))
    # half strength: k = 1/2 halves the lobe
    half = R.rcas_f64(img, 0.5)
    assert abs(half[2, 2, 0] - float(_by_hand(lo, lo, lo, hi, lo, Fraction(1, 2)))) < 1e-15
    assert abs(half[2, 3, 0] - float(_by_hand(hi, lo, hi, hi, hi, Fraction(1, 2)))) < 1e-15


def test_a_ring_of_zeros_and_a_ring_of_ones_follow_the_two_special_cases():
    zero_ring = np.zeros((3, 3)); zero_ring[1, 1] = 0.6             # mx = 0: hitMin is 0, hitMax = (1 - 0.6) / -4: lobe_c = max(-0, -0.1) = -0 -> unchanged
    one_ring = np.ones((3, 3)); one_ring[1, 1] = 0.4                # mn = 1: hitMax is 0, hitMin = 0.4 / 4: lobe_c = max(-0.1, 0) = 0 -> unchanged
    for grey in (zero_ring, one_ring):
        img = _rgba(grey)
        with np.errstate(all="raise", divide="ignore", invalid="ignore"):
            out, mask = R.rcas_f32(img, 1.0)
            f64 = R.rcas_f64(img, 1.0)
        assert np.isfinite(out).all() and np.isfinite(f64).all() and not mask.any()
        assert out[1, 1, 0] == np.float32(grey[1, 1]) and f64[1, 1, 0] == float(np.float32(grey[1, 1]))
        assert _by_hand(grey[0, 1], grey[1, 0], np.float32(grey[1, 1]), grey[1, 2], grey[2, 1], 1) == Fraction(float(np.float32(grey[1, 1])))
    # the neighbours of the centre see one tap that differs: the zero ring's are pulled no lower than 0, the one ring's no higher than 1
    out0, _ = R.rcas_f32(_rgba(zero_ring), 1.0)
    out1, _ = R.rcas_f32(_rgba(one_ring), 1.0)
    assert out0[0, 1, 0] == 0.0 and out1[0, 1, 0] == 1.0
    # a channel whose ring is zero beside channels that sharpen: the lobe is the channels' maximum, so this pixel is left alone
    img = _rgba(np.full((3, 3), 0.5)); img[1, 1, :3] = (0.9, 0.1, 0.6); img[0, 1, 0] = img[2, 1, 0] = img[1, 0, 0] = img[1, 2, 0] = 0.0
    out, _ = R.rcas_f32(img, 1.0)
    assert np.array_equal(_bits(out[1, 1]), _bits(img[1, 1]))


def test_inputs_outside_zero_to_one_and_nan_are_saturated_first():
    rng = np.random.default_rng(7)
    clean = rng.random((6, 6, 4), dtype=np.float32)
    clean[2, 2, 0] = 0.0; clean[3, 4, 1] = 1.0; clean[1, 5, 2] = 0.0; clean[4, 1, 0] = 0.0
    dirty = clean.copy()
    dirty[2, 2, 0] = -3.5; dirty[3, 4, 1] = 17.0; dirty[1, 5, 2] = np.nan; dirty[4, 1, 0] = -0.0
    dirty[..., 3] = clean[..., 3] = np.arange(36, dtype=np.float32).reshape(6, 6)
    a, _ = R.rcas_f32(dirty, 0.8)
    b, _ = R.rcas_f32(clean, 0.8)
    assert np.array_equal(_bits(a), _bits(b)) and np.isfinite(a).all()
    assert np.array_equal(R.rcas_f64(dirty, 0.8), R.rcas_f64(clean, 0.8))
    assert a[..., :3].min() >= 0.0 and a[..., :3].max() <= 1.0
    inf = clean.copy(); inf[2, 3, 1] = np.inf; inf[3, 3, 2] = -np.inf
    one = clean.copy(); one[2, 3, 1] = 1.0; one[3, 3, 2] = 0.0
    assert np.array_equal(_bits(R.rcas_f32(inf, 1.0)[0]), _bits(R.rcas_f32(one, 1.0)[0]))


def test_alpha_passes_through_bit_for_bit(random_image):
    img = random_image.copy()
    img[..., 3] = np.arange(img.shape[0] * img.shape[1], dtype=np.float32).reshape(img.shape[:2]) - 100.0
    img[0, 0, 3] = np.nan; img[0, 1, 3] = np.inf; img[0, 2, 3] = -0.0; img[0, 3, 3] = 1e-45
    out, _ = R.rcas_f32(img, 0.6)
    assert np.array_equal(_bits(out[..., 3]), _bits(img[..., 3]))
    assert not np.array_equal(_bits(out[..., :3]), _bits(img[..., :3]))


# ---- 2. edges --------------------------------------------------------------------------------------------------------------------

def test_border_pixels_take_the_clamped_taps(random_image):
    img = random_image[:10, :12]
    padded = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="edge")
    for s in (0.3, 1.0):
        out, _ = R.rcas_f32(img, s)
        ref, _ = R.rcas_f32(padded, s)
        assert np.array_equal(_bits(out), _bits(ref[1:-1, 1:-1]))
        assert np.array_equal(R.rcas_f64(img, s), R.rcas_f64(padded, s)[1:-1, 1:-1])
    # one corner by hand: at (0, 0) above and left are the pixel itself
    grey = img[..., 0].astype(np.float64)
    want = _by_hand(grey[0, 0], grey[0, 0], grey[0, 0], grey[0, 1], grey[1, 0], 1)
    assert abs(R.rcas_f64(_rgba(img[..., 0]), 1.0)[0, 0, 0] - float(want)) < 1e-15
    want = _by_hand(grey[8, 11], grey[9, 10], grey[9, 11], grey[9, 11], grey[9, 11], 1)
    assert abs(R.rcas_f64(_rgba(img[..., 0]), 1.0)[9, 11, 0] - float(want)) < 1e-15


@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (9, 1), (2, 2)])
def test_degenerate_image_sizes(h, w):
    img = np.random.default_rng(h * 100 + w).random((h, w, 4), dtype=np.float32)
    out, mask = R.rcas_f32(img, 1.0)
    assert out.shape == (h, w, 4) and np.isfinite(out).all() and not mask.any()
    if (h, w) == (1, 1):                          # every tap is the pixel: unchanged in exact arithmetic
        assert np.abs(out.astype(np.float64) - img).max() <= R.BOUND
    grey = img[..., 0].astype(np.float64)
    f64 = R.rcas_f64(_rgba(img[..., 0]), 1.0)
    for y in range(h):
        for x in range(w):
            t = lambda yy, xx: grey[min(max(yy, 0), h - 1), min(max(xx, 0), w - 1)]
            assert abs(f64[y, x, 0] - float(_by_hand(t(y - 1, x), t(y, x - 1), t(y, x), t(y, x + 1), t(y + 1, x), 1))) < 1e-15


# ---- 3. monotone strength --------------------------------------------------------------------------------------------------------

def _check_monotone(img):
    base = R.laplacian(np.clip(img[..., :3], 0.0, 1.0))
    laps = [R.laplacian(R.rcas_f32(img, s)[0][..., :3]) for s in STRENGTHS]
    assert all(a < b for a, b in zip([base] + laps, laps)), (base, laps)
    at_one = R.rcas_f32(img, 1.0)[0]
    for s in (1.5, 4.0, float("inf")):
        assert np.array_equal(_bits(R.rcas_f32(img, s)[0]), _bits(at_one))


def test_sharpening_rises_with_the_field_on_a_random_image(random_image):
    _check_monotone(random_image)


def test_sharpening_rises_with_the_field_on_the_oracles_upscaled_image(oracle_upscaled):
    _check_monotone(oracle_upscaled)


# ---- 4. float32 against float64 --------------------------------------------------------------------------------------------------

def _f32_f64_distance(img):
    return max(float(np.abs(R.rcas_f32(img, s)[0][..., :3].astype(np.float64) - R.rcas_f64(img, s)).max()) for s in STRENGTHS)


def test_float32_form_stays_within_the_derived_bound_of_the_float64_form(random_image, oracle_upscaled):
    assert R.BOUND == 48.0 * 2.0 ** -24
    worst = {"random": _f32_f64_distance(random_image), "oracle": _f32_f64_distance(oracle_upscaled)}
    print("rcas_f32 - rcas_f64, max abs:", worst)
    assert max(worst.values()) <= R.BOUND, worst


# ---- 5. subnormal mask -----------------------------------------------------------------------------------------------------------

def test_the_subnormal_mask_marks_exactly_the_pixels_that_touch_a_subnormal():
    img = _rgba(np.full((5, 5), 0.5))
    img[2, 2, 1] = 1e-40                                           # a subnormal tap: the pixel and its four neighbours read it
    _, mask = R.rcas_f32(img, 1.0)
    want = np.zeros((5, 5), dtype=bool); want[2, 2] = want[1, 2] = want[3, 2] = want[2, 1] = want[2, 3] = True
    assert np.array_equal(mask, want)
    img[2, 2, 1] = 0.0                                             # zero is not subnormal
    assert not R.rcas_f32(img, 1.0)[1].any()


def test_the_subnormal_mask_is_empty_on_the_images_compared_bit_for_bit(random_image, oracle_upscaled):
    for s in (0.3, 1.0) + STRENGTHS:
        assert not R.rcas_f32(oracle_upscaled, s)[1].any()
        assert not R.rcas_f32(random_image, s)[1].any()
