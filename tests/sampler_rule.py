"""Texture spec T1-T3 and the primary-ray texture differentials restated in float64 numpy: the rule the software sampler of csrc/shade.h
(tex_address, tex_sample_level_impl, tex_sample_grad, compute_ray_diffs and the differential chain of surface_anyhit_view) is held to.

Written from the reference and D3D sampler semantics, not from the kernels:
  T1  texel = byte / 255.
  T2  POINT takes texel floor(u * w); LINEAR blends texels floor(u * w - 0.5) and the next one by the fraction.  WRAP repeats with period n,
      MIRROR reflects with period 2n, CLAMP holds the edge texel; per axis.  Level l is max(w >> l, 1) x max(h >> l, 1).
  T3  SampleGrad, isotropic: rho = max(|ddx * (w0, h0)|, |ddy * (w0, h0)|), lod = clamp(log2(rho), 0, mips - 1) (lod 0 when rho is 0).
      LINEAR blends levels floor(lod) and min(floor(lod) + 1, mips - 1) by lod - floor(lod); POINT takes level (int)(lod + 0.5).
  Ray differentials: PrimaryRayGen.hlsl:34-59 and Ray.hlsli:37-94 (computeRayDiffs with resolution.zw, the screen size; propagateRayDiffs;
  computeBarycentricDifferentials; computeTextureDifferentials), with the pinhole vectors cameraU / V / W of rt64_view.cpp:992-1009.

Inputs are what the GPU itself used: the texture levels read back with RT64_ReadbackTexture, the hit (t, barycentrics, primitive, instance)
bit for bit from the frame's images, the vertex buffers and transforms of the scene.  The interpolated uv is formed in float32 exactly as the
kernel forms it (the library is built with -ffp-contract=off, so every product and sum is rounded on its own); everything after that is float64.

Every discrete decision comes back with its margin next to the value: the texel index (in texels, per axis and level), the point-filter level
(distance of the lod to a half-integer) and the byte rounding of the result.  `sample_grad_bounds` turns the margins into the set of bytes a
float32 sampler may return: the rule evaluated at the corners of the box (u +- du, v +- dv, lod +- dlod), widened by the float32 arithmetic of
the filter.  Test helper: imported by tests/test_sampler_rule.py and tests/test_gpu_sampler.py.
"""
import numpy as np

WRAP, MIRROR, CLAMP = 0, 1, 2
POINT, LINEAR = 0, 1
F32 = np.float32


# ---- T1 / T2 -------------------------------------------------------------------------------------------------------------------------

def address(i, n, mode):
    """Texel index i (any integer, negative included) of an axis of n texels under WRAP / MIRROR / CLAMP."""
    i = np.asarray(i, dtype=np.int64)
    if mode == CLAMP:
        return np.clip(i, 0, n - 1)
    if mode == MIRROR:
        j = np.mod(i, 2 * n)
        return np.where(j < n, j, 2 * n - 1 - j)
    return np.mod(i, n)


def level_size(w0, h0, l):
    return max(w0 >> l, 1), max(h0 >> l, 1)


def _dist_to_int(s):
    return np.abs(s - np.round(s))


def sample_level(levels, u, v, lvl, filt, ha, va):
    """Sample levels[lvl] at (u, v) (float64 [N]); lvl int [N].  Returns (value [N, 4] float64, texel-index margin [N] in texels, raw
    unaddressed first texel index (x [N], y [N]))."""
    u = np.asarray(u, dtype=np.float64); v = np.asarray(v, dtype=np.float64)
    lvl = np.broadcast_to(np.asarray(lvl, dtype=np.int64), u.shape)
    n = u.shape[0]
    out = np.zeros((n, 4)); margin = np.full(n, np.inf); rx = np.zeros(n, dtype=np.int64); ry = np.zeros(n, dtype=np.int64)
    for l in np.unique(lvl):
        m = lvl == l
        tex = levels[int(l)].astype(np.float64) / 255.0
        h, w = tex.shape[:2]
        if filt == POINT:
            xs, ys = u[m] * w, v[m] * h
        else:
            xs, ys = u[m] * w - 0.5, v[m] * h - 0.5
        x0, y0 = np.floor(xs), np.floor(ys)
        margin[m] = np.minimum(_dist_to_int(xs), _dist_to_int(ys))
        xi, yi = x0.astype(np.int64), y0.astype(np.int64)
        rx[m], ry[m] = xi, yi
        if filt == POINT:
            out[m] = tex[address(yi, h, va), address(xi, w, ha)]
            continue
        fx, fy = (xs - x0)[:, None], (ys - y0)[:, None]
        xa, xb = address(xi, w, ha), address(xi + 1, w, ha)
        ya, yb = address(yi, h, va), address(yi + 1, h, va)
        top = tex[ya, xa] * (1.0 - fx) + tex[ya, xb] * fx
        bot = tex[yb, xa] * (1.0 - fx) + tex[yb, xb] * fx
        out[m] = top * (1.0 - fy) + bot * fy
    return out, margin, (rx, ry)


# ---- T3 -------------------------------------------------------------------------------------------------------------------------------

def raw_lod(ddx, ddy, w0, h0):
    """log2(rho) before the clamp (-inf where rho is 0) and rho itself."""
    ddx = np.asarray(ddx, dtype=np.float64); ddy = np.asarray(ddy, dtype=np.float64)
    sc = np.array([w0, h0], dtype=np.float64)
    rho = np.maximum(np.hypot(*(ddx * sc).T), np.hypot(*(ddy * sc).T))
    with np.errstate(divide="ignore"):
        return np.where(rho > 0.0, np.log2(np.where(rho > 0.0, rho, 1.0)), -np.inf), rho


def clamp_lod(raw, mips):
    return np.clip(np.where(np.isfinite(raw) | (raw > 0), raw, 0.0), 0.0, mips - 1)


def sample_at_lod(levels, u, v, lod, filt, ha, va):
    """T3 given the clamped lod [N].  Returns (value [N, 4], texel margin [N], lod margin [N], first level [N], second level [N], raw indices
    of the first level)."""
    mips = len(levels)
    lod = np.asarray(lod, dtype=np.float64)
    if filt == POINT:
        lvl = np.floor(lod + 0.5).astype(np.int64)
        if mips > 1:
            c = np.clip(np.round(lod - 0.5) + 0.5, 0.5, mips - 1.5)
            lod_margin = np.abs(lod - c)
        else:
            lod_margin = np.full(lod.shape, np.inf)
        val, tm, raw = sample_level(levels, u, v, lvl, filt, ha, va)
        return val, tm, lod_margin, lvl, lvl, raw
    l0 = np.floor(lod).astype(np.int64)
    l1 = np.minimum(l0 + 1, mips - 1)
    f = (lod - l0)[:, None]
    a, ma, raw = sample_level(levels, u, v, l0, filt, ha, va)
    b, mb, _ = sample_level(levels, u, v, l1, filt, ha, va)
    tm = np.where(f[:, 0] > 0.0, np.minimum(ma, mb), ma)
    return a * (1.0 - f) + b * f, tm, np.full(lod.shape, np.inf), l0, l1, raw


def sample_grad(levels, u, v, ddx, ddy, filt, ha, va):
    """SampleGrad: dict(value, lod, raw_lod, tex_margin, lod_margin, byte, byte_margin, level0, level1, raw_x, raw_y)."""
    h0, w0 = levels[0].shape[:2]
    raw, _ = raw_lod(ddx, ddy, w0, h0)
    lod = clamp_lod(raw, len(levels))
    val, tm, lm, l0, l1, (rx, ry) = sample_at_lod(levels, u, v, lod, filt, ha, va)
    t = val * 255.0
    return dict(value=val, lod=lod, raw_lod=raw, tex_margin=tm, lod_margin=lm, byte=to_byte(val),
                byte_margin=np.abs(t - (np.floor(t) + 0.5)).min(axis=1), level0=l0, level1=l1, raw_x=rx, raw_y=ry)


def to_byte(x):
    """UNORM8 store (D3D: round to nearest, saturate)."""
    return np.clip(np.floor(np.asarray(x, dtype=np.float64) * 255.0 + 0.5), 0, 255).astype(np.int64)


def sample_grad_bounds(levels, u, v, ddx, ddy, filt, ha, va, du, dv, dlod, eps):
    """The rule and what a float32 sampler may return.  du, dv ([N] or scalars, uv units) and dlod (lod units) bound the error of the
    sampler's texel coordinate and lod; eps bounds the float32 rounding of the filter arithmetic (value units).
    Returns sample_grad's dict plus:
      lo, hi        [N, 4] the lowest / highest byte over the corners of the box, widened by eps
      corners       [9, N, 4] the bytes at the centre and the eight corners (a POINT sample must equal one of them in every channel)
      strict        [N] the box holds a single byte in every channel: the sampler must return `byte` exactly
      vmin, vmax    [N, 4] lowest / highest value over the corners."""
    r = sample_grad(levels, u, v, ddx, ddy, filt, ha, va)
    mips = len(levels)
    vals = [r["value"]]
    for su in (-1.0, 1.0):
        for sv in (-1.0, 1.0):
            for sl in (-1.0, 1.0):
                lod = np.clip(r["lod"] + sl * dlod, 0.0, mips - 1) if mips > 1 else r["lod"]
                val = sample_at_lod(levels, u + su * du, v + sv * dv, lod, filt, ha, va)[0]
                vals.append(val)
    vals = np.stack(vals)
    vmin, vmax = vals.min(axis=0), vals.max(axis=0)
    r["lo"], r["hi"] = to_byte(vmin - eps), to_byte(vmax + eps)
    r["corners"] = to_byte(vals)
    r["vmin"], r["vmax"] = vmin, vmax
    r["strict"] = (r["lo"] == r["hi"]).all(axis=1)
    return r


# ---- primary rays and texture differentials ------------------------------------------------------------------------------------------

def _normalize(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def perspective_fov_rh(fov, aspect, zn, zf):
    """XMMatrixPerspectiveFovRH, row-vector convention (clip = [x, y, z, 1] @ P)."""
    h = 1.0 / np.tan(0.5 * fov)
    P = np.zeros((4, 4))
    P[0, 0] = h / aspect; P[1, 1] = h; P[2, 2] = zf / (zn - zf); P[2, 3] = -1.0; P[3, 2] = zf * zn / (zn - zf)
    return P


def camera_vectors(view, fov, near, far, aspect):
    """cameraU, cameraV, cameraW (rt64_view.cpp:992-1009): the view direction is view-space +z (getViewDirection, :1797-1802)."""
    viewI = np.linalg.inv(np.asarray(view, dtype=np.float64))
    focal = (near + far) / 2.0
    pos = np.array([0.0, 0.0, 0.0, 1.0]) @ viewI
    d = (np.array([0.0, 0.0, 1.0, 0.0]) @ viewI)[:3]
    d = d / np.linalg.norm(d)
    target = pos[:3] + d * focal
    W = _normalize(target - pos[:3]) * focal
    U = _normalize(np.cross(W, [0.0, 1.0, 0.0]))
    V = _normalize(np.cross(U, W))
    U = U * (focal * np.tan(fov * 0.5) * aspect)
    V = V * (focal * np.tan(fov * 0.5))
    return U, V, W


def primary_rays(view, fov, near, far, screen_w, screen_h, px, py, render_w, render_h):
    """PrimaryRayGen.hlsl:34-59 for pixels (px, py) of a render_w x render_h launch on a screen_w x screen_h device (no jitter).
    Returns (origin [3], rayDirection [N, 3] (not normalised), dDdx [N, 3], dDdy [N, 3])."""
    aspect = screen_w / screen_h
    view = np.asarray(view, dtype=np.float64)
    viewI = np.linalg.inv(view)
    projI = np.linalg.inv(perspective_fov_rh(fov, aspect, near, far))
    dx = ((np.asarray(px, dtype=np.float64) + 0.5) / render_w) * 2.0 - 1.0
    dy = ((np.asarray(py, dtype=np.float64) + 0.5) / render_h) * 2.0 - 1.0
    U, V, W = camera_vectors(view, fov, near, far, aspect)
    nonNorm = dx[:, None] * U + dy[:, None] * V + W
    target = np.stack([dx, -dy, np.ones_like(dx), np.ones_like(dx)], axis=1) @ projI
    D = np.concatenate([target[:, :3], np.zeros((len(dx), 1))], axis=1) @ viewI
    origin = (np.array([0.0, 0.0, 0.0, 1.0]) @ viewI)[:3]
    dDdx, dDdy = ray_diffs(nonNorm, U, V, screen_w, screen_h)
    return origin, D[:, :3], dDdx, dDdy


def ray_diffs(nonNorm, right, up, vw, vh):
    """computeRayDiffs (Igehy eq. 8), Ray.hlsli:37-45."""
    dd = np.einsum("ij,ij->i", nonNorm, nonNorm)[:, None]
    divd = 2.0 / (dd * np.sqrt(dd))
    dr = (nonNorm @ right)[:, None]; du = (nonNorm @ up)[:, None]
    dDdx = (dd * right - dr * nonNorm) * divd / vw
    dDdy = -(dd * up - du * nonNorm) * divd / vh
    return dDdx, dDdy


def texture_grads(D, t, dDdx, dDdy, posW, uv, normal_matrix, pos):
    """propagateRayDiffs + computeBarycentricDifferentials + computeTextureDifferentials (Ray.hlsli:47-94) for a primary ray
    (dOdx = dOdy = 0).  D [N, 3] the ray direction as traced, t [N] its hit distance, posW [N, 3, 3] world corners, uv [N, 3, 2],
    normal_matrix [N, 3, 3] (objectToWorldNormal, row-vector convention), pos [N, 3, 3] object-space corners (the triangle normal
    -cross(p2 - p0, p1 - p0) is taken there and transformed).  Returns (ddx [N, 2], ddy [N, 2])."""
    t = np.asarray(t, dtype=np.float64)[:, None]
    tn = -np.cross(pos[:, 2] - pos[:, 0], pos[:, 1] - pos[:, 0])
    N = _normalize(np.einsum("ni,nij->nj", tn, normal_matrix))
    dodx, dody = t * dDdx, t * dDdy
    rcpDN = 1.0 / np.einsum("ij,ij->i", D, N)[:, None]
    dodx = dodx + D * (-np.einsum("ij,ij->i", dodx, N)[:, None] * rcpDN)
    dody = dody + D * (-np.einsum("ij,ij->i", dody, N)[:, None] * rcpDN)
    e01, e02 = posW[:, 1] - posW[:, 0], posW[:, 2] - posW[:, 0]
    Nu, Nv = np.cross(e02, N), np.cross(e01, N)
    Lu = Nu / np.einsum("ij,ij->i", Nu, e01)[:, None]
    Lv = Nv / np.einsum("ij,ij->i", Nv, e02)[:, None]
    uv = np.asarray(uv, dtype=np.float64)
    uv01, uv02 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
    dot = lambda a, b: np.einsum("ij,ij->i", a, b)[:, None]
    ddx = dot(Lu, dodx) * uv01 + dot(Lv, dodx) * uv02
    ddy = dot(Lu, dody) * uv01 + dot(Lv, dody) * uv02
    return ddx, ddy


def interpolate_uv_f32(uv, bu, bv):
    """vertexUV = uv0 * b0 + uv1 * b1 + uv2 * b2 with b0 = 1 - u - v, every operation rounded to float32 in that order.
    uv [N, 3, 2] float32, bu / bv [N] float32 (the hit's barycentrics).  Returns [N, 2] float32."""
    uv = np.asarray(uv, dtype=F32); bu = np.asarray(bu, dtype=F32); bv = np.asarray(bv, dtype=F32)
    b0 = (F32(1.0) - bu) - bv
    return (uv[:, 0] * b0[:, None] + uv[:, 1] * bu[:, None]) + uv[:, 2] * bv[:, None]
