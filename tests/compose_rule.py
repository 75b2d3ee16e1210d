"""ComposePS as a rule in numpy float64 (rules C1-C6).  TEST INFRASTRUCTURE.

The library states ComposePS five times (`compose_post_kernel<true>` and `<false>` in csrc/image_passes.hip, `compose_pixel` in csrc/svgf.hip, `compose_lean_pixel`
and `compose_lean_value` in csrc/passes.hip) and the oracle a sixth (`pass_compose_post` in oracle/oracle_render.c); all were written from the same HLSL, and the tests
that compare them with each other cannot tell whether that reading is right.  This module states the pass once more, from the shader's meaning, in float64 on the
error-carrying values of tests/light_rule.py (`F`: a value and a first-order bound on what the float32 operations may have done to it).  It imports nothing from
oracle/ and was not written from the kernels.

Rules (C:n = ComposePS.hlsl line n; every image is read at the pixel itself: the full-screen triangle of FullScreenVS.hlsl:5-9 at render size puts uv on the texel
centre, where the LINEAR sampler returns the texel):

C1  Inputs.  gDiffuse is RGBA8: every channel is k / 255 for an integer k, exactly the float32 nearest to it.  The rule checks that of the readback (`unorm8_inputs`)
    and takes that float32 as the value the shader loads.  The light and the additive images are RGBA16F; their readbacks are exact.
C2  The alpha test (C:20).  a > EPSILON = 1e-6f.  a is 0 or at least 1 / 255: the test is exact and no pixel is undecided.
C3  Lit pixels (C:21-32).  result = lerp(d, d * (direct + indirect), a) + reflection + refraction + transparent, per channel, with lerp(x, y, s) = x + s * (y - x).
    Seven float32 operations; each rounds once (half an ulp of its result, no contraction: the build has -ffp-contract=off) and the bound carries the roundings
    through the operations that follow, first order.
C4  Unlit pixels (C:34-36).  result = d.rgb, exact.
C5  Alpha is 1 (C:32, C:35), exact.
C6  Lean frames (RT64_FRAME_STATS.leanFrame: giSamples = 0 and nothing reflects, refracts, is fogged or translucent).  The filtered copies and the three additive
    images are not produced.  direct is DIRECT_LIGHT_RAW (rt64_view.cpp:1438-1509 copies it to the filtered image unchanged); indirect is the constant
    IndirectRayGen.hlsl stores without GI samples, ambientBaseColor + ambientNoGIColor as one float32 sum rounded to the RGBA16F image; the additive images are
    exact zeros and x + 0 does not round, so the three sums are left out.  The rule takes the two colours from the scene description.

Held outputs: OUTPUT_RGBA32F within the bound.  With no separate post pass PostProcessPS.hlsl:34-35 is a passthrough of the same texel and the back buffer is
UNORM8: FINAL_RGBA8 lies in [unorm8(value - bound'), unorm8(value + bound')] with unorm8(x) = floor(255 sat(x) + 0.5) and bound' = bound plus the two roundings of
255 x + 0.5 in float32 (`to_final`).

Not covered: the mean over primary_spp sub-frames (oracle rule P3: the sub-frames cannot be read back), the HUD blend over the back buffer (tests/raster_rule.py)
and debug views."""
import numpy as np

import light_rule as L
from light_rule import F, U

MUTATIONS = ("no_alpha_lerp", "alpha_test_ge", "reflection_dropped", "indirect_not_f16_on_lean", "lean_reads_filtered")

EPSILON = L.EPSILON


def unorm8(x):
    """floor(255 sat(x) + 0.5) in float64."""
    return np.floor(255.0 * np.nan_to_num(np.clip(np.asarray(x, dtype=np.float64), 0.0, 1.0), nan=0.0) + 0.5).astype(np.int64)


def unorm8_of_float32(x):
    """The conversion of a float32 that is KNOWN, as Direct3D defines FLOAT -> UNORM: clamp to [0, 1] (a NaN becomes 0), scale by 255, add 0.5, drop the fraction,
    every step a float32 operation.  It is what the back buffer holds where the same launch stored the float32 beside it."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        s = np.where(x > 0.0, np.minimum(x, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    return np.floor(s * np.float32(255.0) + np.float32(0.5)).astype(np.int64)


def to_final(value, bound):
    """The UNORM8 interval of a float32 colour within value +- bound: (lo, hi), int64.  255 * x and + 0.5 round once each in float32; as an error of x that is
    U (255 |x| + (255 |x| + 0.5)) / 255."""
    v = np.asarray(value, dtype=np.float64)
    s = np.clip(np.abs(v), 0.0, 1.0)
    b = np.asarray(bound, dtype=np.float64) + U * (2.0 * s + 0.5 / 255.0)
    return unorm8(v - b), unorm8(v + b)


def _unorm8_input(image):
    """(C1) -> (the float32 of k / 255 as float64: what the shader's load returns, mask of texels that are one)."""
    d = np.asarray(image, dtype=np.float32)
    k = np.rint(d.astype(np.float64) * 255.0)
    exact = ((k / 255.0).astype(np.float32) == d) & (k >= 0) & (k <= 255)
    return d.astype(np.float64), exact.all(axis=-1)


def ambient_constant(ambient_base, ambient_no_gi, mutate=None):
    """(C6) float16(float32(base) + float32(noGI)), per channel, as float64."""
    s = np.asarray(ambient_base, dtype=np.float32) + np.asarray(ambient_no_gi, dtype=np.float32)
    if mutate == "indirect_not_f16_on_lean":
        return s.astype(np.float64)
    return s.astype(np.float16).astype(np.float64)


def compose(images, lean=False, ambient=None, mutate=None):
    """images: dict of (H, W, 4) readbacks: diffuse; direct, indirect (the FILTERED images); reflection, refraction, transparent; on a lean frame direct_raw instead
    of all five.  ambient: (ambientBaseColor, ambientNoGIColor), read on a lean frame only.
    Returns dict(value, bound (H, W, 4); lit (H, W) bool: the C2 branch; unorm8_inputs (H, W) bool; info: counts)."""
    d, ok = _unorm8_input(images["diffuse"])
    a = d[..., 3]
    lit = (a >= 0.0) if mutate == "alpha_test_ge" else (a > EPSILON)
    h, w = a.shape
    value = np.ones((h, w, 4)); bound = np.zeros((h, w, 4))
    if lean and mutate != "lean_reads_filtered":
        direct = np.asarray(images["direct_raw"], dtype=np.float64)[..., :3]
        indirect = np.broadcast_to(ambient_constant(ambient[0], ambient[1], mutate), (h, w, 3))
        extra = ()
    else:
        direct = np.asarray(images["direct"], dtype=np.float64)[..., :3]
        indirect = np.asarray(images["indirect"], dtype=np.float64)[..., :3]
        extra = () if lean else tuple(k for k in ("reflection", "refraction", "transparent") if not (mutate == "reflection_dropped" and k == "reflection"))
    for c in range(3):
        dc = F(d[..., c])
        r = L.mul(dc, L.add(F(direct[..., c]), F(indirect[..., c])))                # (C3) result *= direct + indirect
        if mutate != "no_alpha_lerp":
            r = L.add(dc, L.mul(F(a), L.sub(r, dc)))                                  # lerp(d, result, a)
        for k in extra:
            r = L.add(r, F(np.asarray(images[k], dtype=np.float64)[..., c]))
        value[..., c] = np.where(lit, r.v, d[..., c])                                # (C4)
        bound[..., c] = np.where(lit, r.e, 0.0)
    finite = np.isfinite(value).all(axis=-1) & np.isfinite(bound).all(axis=-1)
    counts = dict(lit=int(lit.sum()), unlit=int((~lit).sum()), partial=int(((a > 0.0) & (a < 1.0)).sum()), opaque=int((a == 1.0).sum()),
                  not_covered=int((~finite).sum()), not_unorm8=int((~ok).sum()))
    for k in ("reflection", "refraction", "transparent"):
        if k in images and images[k] is not None:
            counts[k] = int((np.asarray(images[k])[..., :3] != 0.0).any(axis=-1).sum())
    return dict(value=value, bound=bound, lit=lit, unorm8_inputs=ok, covered=finite, info=dict(counts=counts))


def ratio(stored, value, bound):
    """|stored - value| / bound per element; 0 where they are equal, inf where they differ and the bound is 0 (or anything is not a number)."""
    dev = np.abs(np.asarray(stored, dtype=np.float64) - value)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(dev == 0.0, 0.0, dev / bound)
    return np.where(np.isnan(r), np.inf, r)


def compare(output, final, rule):
    """OUTPUT_RGBA32F (and, where the frame had no separate post pass, FINAL_RGBA8; else None) against the rule.
    Returns dict(ratio: (largest, mean), bad (H, W) bool, two_candidates: pixels whose interval spans two RGBA8 steps, final_bad, final_not_output)."""
    r = ratio(np.asarray(output)[..., :4], rule["value"], rule["bound"]).max(axis=-1)
    bad = ~(r < 1.0) | ~rule["covered"]
    out = dict(ratio=(float(r.max()), float(np.where(np.isfinite(r), r, 1e9).mean())), bad=bad, two_candidates=0, final_bad=0, final_not_output=0)
    if final is not None:
        lo, hi = to_final(rule["value"], rule["bound"])
        f = np.asarray(final).astype(np.int64)
        out["final_bad"] = int(((f < lo) | (f > hi)).any(axis=-1).sum())
        out["two_candidates"] = int((hi > lo).any(axis=-1).sum())
        out["final_not_output"] = int((f != unorm8_of_float32(output)).any(axis=-1).sum())
    return out
