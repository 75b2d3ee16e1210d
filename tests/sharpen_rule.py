"""Sharpening rule S1-S7 (RT64_VIEW_DESC.upscalerSharpness; csrc/upscale.hip rcas_sharpen_kernel) restated in numpy: AMD's public RCAS
("robust contrast-adaptive sharpening", the sharpener of FSR 1 / FSR 2) with the points it leaves to hardware pinned.  Test helper: imported by
tests/test_sharpen_rule.py and tests/test_gpu_sharpen.py.

  S1  s = min(upscalerSharpness, 1); k = 2^(2 s - 2), computed in double and rounded to the nearest float32.  s <= 0 or NaN: the stage does not run.
  S2  input: the upscaler's output of the frame, [h, w, 4] float32 (rgb + frame count).  Taps e (the pixel), b (above), d (left), f (right), h (below),
      coordinates clamped to the image; every rgb tap is saturated first, fminf(fmaxf(x, 0), 1): a NaN becomes 0 (and -0 becomes +0, as v_max_f32 orders
      the zeros).
  S3  per channel: mn = min(b, d, f, h), mx = max(b, d, f, h); hitMin = min(mn, e) / (4 mx), 0 when mx = 0; hitMax = (1 - max(mx, e)) / (4 mn - 4),
      0 when mn = 1; lobe_c = max(-hitMin, hitMax).
  S4  lobe = max(-0.1875, min(max(lobe_r, lobe_g, lobe_b), 0)) k.
  S5  out_c = saturate((lobe (((b + d) + f) + h) + e) / (4 lobe + 1)); alpha = the input's alpha, bit for bit.
  S6  float32 throughout, in exactly that order, IEEE divisions, no fused multiply-add, no noise-removal term.

`rcas_f32` rounds every step to float32 (numpy's float32 +, -, *, / are the IEEE operations); `rcas_f64` evaluates the same formulas in float64 on the
same float32 inputs with the same float32 k.

Distance between the two (BOUND), from the operation count, u = 2^-24 (half an ulp of 1), taps in [0, 1]:
  * the branches of S3 (mx = 0, mn = 1) and every min / max select on the exact float32 taps or are 1-Lipschitz, so both forms walk the same formula;
  * hitMin <= 1/4 (min(mn, e) <= mx): 4 mx is exact, one division: error <= u/4;
  * |hitMax| <= 1/4 (max(mx, e) >= mn): 1 - x is exact for x >= 1/2 and within u/2 of a value >= 1/2 otherwise (relative u), 4 mn is exact, 4 mn - 4
    rounds once (relative u), one division (relative u): error <= 3u/4;
  * lobe_c, its maximum over the channels and the clamp of S4 are 1-Lipschitz: <= 3u/4; times k <= 1, |lobe| <= 3/16: one more rounding, dL <= u;
  * the sum ((b + d) + f) + h <= 4: the three additions round by at most u, 2u, 2u: <= 5u;
  * lobe * sum, magnitude <= 3/4: 4 dL + (3/16) 5u + u/2 < 5.5u;  + e, magnitude <= 1: + u/2, so the numerator is within dN <= 6u;
  * 4 lobe is exact, + 1 lies in [1/4, 1]: dD <= 4 dL + u/2 = 4.5u;
  * the quotient q lies in [0, 1] (that is what the limiter of S3 is for) and the denominator is >= 1/4: (dN + q dD) / (1/4) + u/2 <= 42.5u; the
    saturation is 1-Lipschitz.
  First order 42.5u; BOUND = 48u = 2.86e-6 leaves room for the second-order terms.  Measured maximum over the seeded random image and the oracle's
  upscaled image of the sample scene at s in {0.25, 0.5, 0.75, 1}: 3.5e-7 (5.8u).
"""
import numpy as np

U = 2.0 ** -24
BOUND = 48.0 * U
TINY = np.finfo(np.float32).tiny              # 2^-126: smallest normal float32


def strength(sharpness):
    """S1: k as the float32 the kernel receives, or None when the stage does not run (sharpness <= 0 or NaN).  The field is a float32."""
    s = float(np.float32(sharpness))
    if not s > 0.0:
        return None
    return np.float32(2.0 ** (2.0 * min(s, 1.0) - 2.0))


def _taps(img):
    """S2: the rgb taps (e, b, d, f, h) of every pixel, coordinates clamped, in the dtype of img."""
    p = np.pad(img[..., :3], ((1, 1), (1, 1), (0, 0)), mode="edge")
    return p[1:-1, 1:-1], p[:-2, 1:-1], p[1:-1, :-2], p[1:-1, 2:], p[2:, 1:-1]


def _sat(x):
    """fminf(fmaxf(x, 0), 1): NaN -> 0, -0 -> +0."""
    zero, one = x.dtype.type(0), x.dtype.type(1)
    with np.errstate(invalid="ignore"):
        return np.where(x > zero, np.minimum(x, one), zero).astype(x.dtype)


def _rcas(img, k, T, watch):
    """S2-S5 in floating type T; watch(x) is called on every intermediate."""
    src = np.ascontiguousarray(img, dtype=np.float32)
    assert src.ndim == 3 and src.shape[2] == 4
    e, b, d, f, h = (watch(_sat(t.astype(T))) for t in _taps(src))
    k = T(np.float32(k))
    c0, c1, c4 = T(0), T(1), T(4)
    with np.errstate(divide="ignore", invalid="ignore"):
        mn = np.minimum(np.minimum(b, d), np.minimum(f, h))
        mx = np.maximum(np.maximum(b, d), np.maximum(f, h))
        hit_min = np.where(mx == c0, c0, watch(np.minimum(mn, e)) / watch(c4 * mx))
        hit_max = np.where(mn == c1, c0, watch(c1 - np.maximum(mx, e)) / watch(watch(c4 * mn) - c4))
    watch(hit_min); watch(hit_max)
    lobe_c = np.maximum(-hit_min, hit_max)                                                  # S3
    lobe = np.maximum(T(-0.1875), np.minimum(lobe_c.max(axis=2, keepdims=True), c0)) * k     # S4
    watch(lobe)
    total = watch(watch(watch(b + d) + f) + h)                                              # S6: ((b + d) + f) + h
    q = watch(watch(watch(lobe * total) + e) / watch(watch(c4 * lobe) + c1))                # S5
    return _sat(q.astype(T))


def rcas_f32(img, sharpness):
    """The rule in float32.  Returns (out [h, w, 4] float32, mask [h, w] bool): mask marks pixels where some non-zero float32 intermediate is
    subnormal (hardware may flush those; the GPU test compares them within BOUND instead of bit for bit).  sharpness must make the stage run."""
    k = strength(sharpness)
    assert k is not None, "S1: the stage does not run"
    src = np.ascontiguousarray(img, dtype=np.float32)
    mask = np.zeros(src.shape[:2], dtype=bool)

    def watch(x):
        assert x.dtype == np.float32, x.dtype
        a = np.abs(x)
        sub = (a > 0) & (a < TINY)
        mask[...] |= sub.any(axis=2) if sub.ndim == 3 else sub
        return x

    out = src.copy()                                                                        # alpha: the input's bits
    out[..., :3] = _rcas(src, k, np.float32, watch)
    return out, mask


def rcas_f64(img, sharpness):
    """The same formulas in float64 on the same float32 taps and the same float32 k.  Returns [h, w, 3] float64 (rgb)."""
    k = strength(sharpness)
    assert k is not None, "S1: the stage does not run"
    return _rcas(img, k, np.float64, lambda x: x)


def laplacian(img):
    """Mean absolute 4-neighbour Laplacian of the rgb channels, float64, coordinates clamped."""
    e, b, d, f, h = _taps(np.asarray(img, dtype=np.float64))
    return float(np.abs(b + d + f + h - 4.0 * e).mean())
