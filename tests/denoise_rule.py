"""The two GI filters restated in float64 numpy from their written specs -- not from csrc/svgf.hip, csrc/passes.hip or the oracle's C:
  denoiser_mode 1, SVGF: the spec at the top of oracle/oracle_svgf.c and DESIGN.md 4 (Schied et al. 2017, sections 4.2-4.4);
  denoiser_mode 0: the reference's GaussianFilterRGB3x3CS.hlsl, five passes (rt64_view.cpp:1512-1530).
Images are float arrays [h, w, 4]: rgb + variance (SVGF) or rgb + whatever alpha the buffer holds (Gaussian).  Every filter pass stores RGBA16F, so
its result is rounded to float16 here too.  Test helper: imported by tests/test_denoise_rule.py and tests/test_gpu_denoise.py."""
import numpy as np

B3 = np.array([1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0])     # 5-tap B3-spline kernel of the a-trous iterations
G3 = np.array([0.25, 0.5, 0.25])                                            # 3x3 Gaussian of the variance (luminance edge stop)
SIGMA_Z, SIGMA_L, PHI_N = 1.0, 4.0, 128.0
STEPS = (1, 2, 4, 8, 16)


def lum(rgb):
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]


def f16(x):
    """Round to the RGBA16F storage of the filter images."""
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def f16_ulp(x):
    """Spacing of float16 at |x| (the subnormal spacing 2^-24 below 2^-14)."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return np.exp2(e - 10.0)


# ---- guide --------------------------------------------------------------------------------------------------------------------------

def guide(depth, instance_id, normal):
    """What the edge stops read per pixel: valid (a surface: instance id >= 0), depth, the depth gradient = the larger absolute forward difference
    of the stored float32 depth to the right and downwards, the neighbour clamped to the frame's edge (a difference of 0 there), and the
    normal (its stored float16 values).  The gradient is the float32 difference of float32 depths, so that the GPU's record can be held to it bit
    for bit."""
    z = np.asarray(depth, dtype=np.float32)
    zx = np.concatenate([z[:, 1:], z[:, -1:]], axis=1)
    zy = np.concatenate([z[1:, :], z[-1:, :]], axis=0)
    gz = np.maximum(np.abs(zx - z), np.abs(zy - z)).astype(np.float32)
    return {"valid": np.asarray(instance_id) >= 0, "depth": z.astype(np.float64), "gz": gz.astype(np.float64),
            "normal": np.asarray(normal, dtype=np.float64)[..., :3]}


def unpack_guide(rec):
    """RT64_IMAGE_FILTER_GUIDE [h, w, 4] u32 -> the guide dict (normal x | y << 16 and z | valid << 16 as float16 bits, depth and gradient as f32 bits)."""
    rec = np.asarray(rec, dtype=np.uint32)
    h16 = lambda v: (v & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float64)
    n = np.stack([h16(rec[..., 0]), h16(rec[..., 0] >> 16), h16(rec[..., 1])], axis=-1)
    return {"valid": (rec[..., 1] >> 16) != 0, "depth": rec[..., 2].view(np.float32).astype(np.float64),
            "gz": rec[..., 3].view(np.float32).astype(np.float64), "normal": n}


def pack_guide(depth, instance_id, normal):
    """The guide record of RT64_IMAGE_FILTER_GUIDE made from float16 normals, float32 depth and the instance ids (the rule's own gradient)."""
    g = guide(depth, instance_id, normal)
    b = np.asarray(normal, dtype=np.float32)[..., :3].astype(np.float16).view(np.uint16).astype(np.uint32)
    rec = np.zeros(np.shape(depth) + (4,), dtype=np.uint32)
    rec[..., 0] = b[..., 0] | (b[..., 1] << 16)
    rec[..., 1] = b[..., 2] | (g["valid"].astype(np.uint32) << 16)
    rec[..., 2] = np.asarray(depth, dtype=np.float32).view(np.uint32)
    rec[..., 3] = g["gz"].astype(np.float32).view(np.uint32)
    return rec


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` outside the frame."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if h - abs(dy) > 0 and w - abs(dx) > 0:
        b[yd, xd] = a[ys, xs]
    return b


def _clamped(a, dy, dx):
    """b[y, x] = a[clamp(y + dy), clamp(x + dx)]."""
    h, w = a.shape[:2]
    yi = np.clip(np.arange(h) + dy, 0, h - 1)
    xi = np.clip(np.arange(w) + dx, 0, w - 1)
    return a[yi][:, xi]


def _edge_weight(g, ky, kx, dist):
    """w_z * w_n of the taps at offset (ky, kx) of every pixel (no clamp: max(0, n.n')^128 may exceed 1 for float16 normals), and whether the tap
    counts at all (inside the frame and on a surface)."""
    nq = _shift(g["normal"], ky, kx, 0.0)
    zq = _shift(g["depth"], ky, kx, 0.0)
    ok = _shift(g["valid"], ky, kx, False)
    wz = np.exp(-np.abs(g["depth"] - zq) / (SIGMA_Z * g["gz"] * dist + 1e-8))
    wn = np.maximum(0.0, np.sum(g["normal"] * nq, axis=-1)) ** PHI_N
    return wz * wn, ok


# ---- SVGF ---------------------------------------------------------------------------------------------------------------------------

def svgf_variance(raw, moments, g):
    """The filter's input image: rgb of the raw GI image, variance in alpha.  history (raw alpha) >= 4: max(0, mu2 - mu1^2); younger: the 7x7
    bilateral estimate (w_z w_n over the surface pixels inside the frame, the centre included) of the luminance's variance, x 4 / max(history, 1);
    pixels without a surface: 0."""
    raw = np.asarray(raw, dtype=np.float64)
    m = np.asarray(moments, dtype=np.float64)
    hist = raw[..., 3]
    var = np.maximum(0.0, m[..., 1] - m[..., 0] ** 2)
    l = lum(raw[..., :3])
    sw = np.zeros(hist.shape); s1 = np.zeros(hist.shape); s2 = np.zeros(hist.shape)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            w, ok = _edge_weight(g, dy, dx, np.sqrt(dx * dx + dy * dy))
            w = np.where(ok, w, 0.0)
            lq = _shift(l, dy, dx, 0.0)
            sw += w; s1 += np.where(w > 0.0, w * lq, 0.0); s2 += np.where(w > 0.0, w * lq * lq, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        m1, m2 = s1 / sw, s2 / sw
        spatial = np.where(sw > 0.0, np.maximum(0.0, m2 - m1 * m1) * (4.0 / np.maximum(hist, 1.0)), 0.0)
    var = np.where(hist >= 4.0, var, spatial)
    var = np.where(g["valid"], var, 0.0)
    out = raw.copy()
    out[..., 3] = f16(var)
    return out


def atrous(img, g, step):
    """One a-trous iteration with step `step`: 5x5 B3 taps at multiples of the step; a tap outside the frame or without a surface weighs 0; the
    centre tap carries the plain kernel weight, every other one h * w_z * w_n * w_l, w_l = exp(-|l_p - l_q| / (sigma_l sqrt(max(0, gauss3x3(var)_p)) + 1e-6))
    with the 3x3 Gaussian of the variance clamp-addressed.  colour' = sum(h w c) / sum(h w), variance' = sum((h w)^2 var) / sum(h w)^2; pixels
    without a surface pass through."""
    img = np.asarray(img, dtype=np.float64)
    gv = np.zeros(img.shape[:2])
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            gv += G3[dx + 1] * G3[dy + 1] * _clamped(img[..., 3], dy, dx)
    phi_l = SIGMA_L * np.sqrt(np.maximum(0.0, gv)) + 1e-6
    lp = lum(img[..., :3])
    sw = np.zeros(gv.shape); sc = np.zeros(img.shape[:2] + (3,)); sv = np.zeros(gv.shape)
    for ky in range(-2, 3):
        for kx in range(-2, 3):
            hk = B3[kx + 2] * B3[ky + 2]
            q = _shift(img, ky * step, kx * step, 0.0)
            if kx == 0 and ky == 0:
                w = np.full(gv.shape, hk)
            else:
                e, ok = _edge_weight(g, ky * step, kx * step, np.sqrt(kx * kx + ky * ky) * step)
                wl = np.exp(-np.abs(lp - lum(q[..., :3])) / phi_l)
                w = np.where(ok, hk * e * wl, 0.0)
            live = w > 0.0                                    # a tap of weight 0 does not count, whatever it holds
            sw += w; sc += np.where(live[..., None], w[..., None] * q[..., :3], 0.0); sv += np.where(live, w * w * q[..., 3], 0.0)
    out = np.empty_like(img)
    out[..., :3] = sc / sw[..., None]
    out[..., 3] = sv / (sw * sw)
    out = f16(out)
    return np.where(g["valid"][..., None], out, img)


def svgf(raw, moments, g, passes=5):
    """Variance + `passes` a-trous iterations (steps 1, 2, 4, 8, 16).  Returns (result, input of the last iteration)."""
    x = svgf_variance(raw, moments, g)
    prev = x
    for k in range(passes):
        prev, x = x, atrous(x, g, STEPS[k])
    return x, prev


# ---- GaussianFilterRGB3x3CS ---------------------------------------------------------------------------------------------------------

K00, K01, K11 = 0.077847, 0.123317, 0.195346
GAUSS_OFFSETS = ((0.5 - K01 / (K01 + K11), 0.5 - K01 / (K01 + K11)), (0.5 + 1.0, 0.5 - K00 / (K00 + K01)), (0.5 - K00 / (K00 + K01), 0.5 + 1.0))
# weights of (sample 0, 1, 2, gInput[DTid + 1]) in the shader's branch order
GAUSS_CASES = (
    ("interior", (K00 + K01 + K01 + K11, K00 + K01, K00 + K01, K00)),
    ("top-left", tuple(v / 0.519827 for v in (K11, K01, K01, K00))),
    ("top-right", tuple(v / 0.519827 for v in (K01 + K11, 0.0, 0.201164, 0.0))),
    ("bottom-left", tuple(v / 0.519827 for v in (K01 + K11, K00 + K01, 0.0, 0.0))),
    ("bottom-right", tuple(v / 0.519827 for v in (K00 + K01 + K01 + K11, 0.0, 0.0, 0.0))),
    ("left", tuple(v / 0.720991 for v in (K01 + K11, K00 + K01, K01, K00))),
    ("right", tuple(v / 0.720991 for v in (K00 + K01 + K01 + K11, 0.0, K00 + K01, 0.0))),
    ("top", tuple(v / 0.720991 for v in (K01 + K11, K01, K00 + K01, K00))),
    ("bottom", tuple(v / 0.720991 for v in (K00 + K01 + K01 + K11, K00 + K01, 0.0, 0.0))),
)


def gauss_case(w, h):
    """[h, w] index into GAUSS_CASES: the first branch of the shader whose condition holds (on a 1-wide or 1-high frame several do)."""
    x = np.arange(w)[None, :]; y = np.arange(h)[:, None]
    xl, xr, yt, yb = x == 0, x == w - 1, y == 0, y == h - 1
    conds = [(x > 0) & (y > 0) & (x < w - 1) & (y < h - 1), xl & yt, xr & yt, xl & yb, xr & yb, xl, xr, yt, np.ones((h, w), bool)]
    case = np.full((h, w), -1)
    for k, c in enumerate(conds):
        case = np.where((case < 0) & np.broadcast_to(c, (h, w)), k, case)
    return case


def _bilinear_clamp(rgb, sx, sy):
    """LINEAR filter, CLAMP addressing (the static sampler of rt64_device.cpp:737-742) at texel-space positions (sx, sy) = uv * size."""
    h, w = rgb.shape[:2]
    fx, fy = sx - 0.5, sy - 0.5
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = (fx - x0)[..., None], (fy - y0)[..., None]
    xa, xb = np.clip(x0.astype(int), 0, w - 1), np.clip(x0.astype(int) + 1, 0, w - 1)
    ya, yb = np.clip(y0.astype(int), 0, h - 1), np.clip(y0.astype(int) + 1, 0, h - 1)
    top = rgb[ya, xa] * (1 - ax) + rgb[ya, xb] * ax
    bot = rgb[yb, xa] * (1 - ax) + rgb[yb, xb] * ax
    return top * (1 - ay) + bot * ay


def gaussian_pass(img, out=None):
    """One GaussianFilterRGB3x3CS dispatch over the whole frame: three bilinear taps at the shader's fractional offsets + gInput[DTid + 1] (0 outside
    the texture), weighted by the branch of the pixel.  The shader writes float3: the alpha of the destination `out` is left as it is (0 without one)."""
    img = np.asarray(img, dtype=np.float64)
    h, w = img.shape[:2]
    rgb = img[..., :3]
    X, Y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    smp = [_bilinear_clamp(rgb, X + ox, Y + oy) for ox, oy in GAUSS_OFFSETS]
    smp.append(_shift(rgb, 1, 1, 0.0))
    wt = np.array([c[1] for c in GAUSS_CASES])[gauss_case(w, h)]          # [h, w, 4]
    res = np.zeros_like(img)
    res[..., :3] = f16(sum(wt[..., k:k + 1] * smp[k] for k in range(4)))
    if out is not None:
        res[..., 3] = np.asarray(out, dtype=np.float64)[..., 3]
    return res


def gaussian(raw, alpha1=None, passes=5):
    """The five passes over the ping-pong pair: image 0 = the raw GI image, pass k reads image k % 2 and writes the other; `alpha1` is the alpha that
    image 1 held before (0 without one).  Returns (result = image 1, input of the last pass = image 0)."""
    imgs = [np.asarray(raw, dtype=np.float64).copy(), np.zeros_like(np.asarray(raw, dtype=np.float64))]
    if alpha1 is not None:
        imgs[1][..., 3] = alpha1
    for k in range(passes):
        imgs[(k % 2) ^ 1] = gaussian_pass(imgs[k % 2], imgs[(k % 2) ^ 1])
    return imgs[1], imgs[0]
