"""The software texture sampler of csrc/shade.h (tex_address, tex_sample_level_impl, tex_sample_grad) and the primary-ray differential chain that
feeds it (compute_ray_diffs, surface_anyhit_view), checked pixel by pixel against the float64 rule of tests/sampler_rule.py.

Every scene is opaque, drawn at 320 x 180 with a shader whose colour is TEX0 alone (no inputs, diffuseColorMix 0, no reflection or refraction),
so RT64_IMAGE_DIFFUSE holds round(255 * sample) of the surface hit.  A specular map sampled with uvDetailScale != 1 (scaled uv, scaled
gradients) comes back through RT64_IMAGE_SHADING_SPECULAR, an RGBA16F image that holds byte / 255.  The rule is fed the frame's own data:
levels read back with RT64_ReadbackTexture, (t, u, v, primitive) bit for bit from RT64_IMAGE_PRIMARY_HIT, the instance from
RT64_IMAGE_INSTANCE_ID, and the vertex buffers and transforms the scene was built from.

Bound.  The rule forms the interpolated uv in float32 exactly as the kernel does (-ffp-contract=off: every product and sum rounded alone), so
the uv itself is shared.  After that the kernel differs from the float64 rule by:
  * the texel coordinate u * w - 0.5 (u * w for POINT): exact in float32 when w is a power of two (then every level's width is one too);
    otherwise two roundings, at most ulp(|u| w) / 2 + ulp(|u| w + 0.5) / 2 texels, i.e. below DU = 2^-23 * (|u| + 1) in uv units;
  * the lod: the differential chain (about 60 float32 operations, s_rcp / s_sqrt / s_div at 1 ulp, no fma contraction) and log2f.  With
    2^-24 per step, a 1 / cos amplification of at most 16 in the projection onto the surface at the grazing angles drawn here, the relative
    error of rho stays below 60 * 16 * 2^-24 < 2^-14, i.e. below 2^-14 / ln 2 in the lod; DLOD = 2^-12 leaves a factor of 2.8;
  * the filter arithmetic: T1's texel in float32 and at most 9 roundings of values in [0, 1] -> EPS = 2^-19 in value units.
A pixel whose box (u +- DU, v +- DV, lod +- DLOD, value +- EPS) holds one byte per channel must return that byte exactly.  Every other pixel
is exempt, and must still return a byte within the box; a POINT pixel must return, in all three channels at once, the texel of one of the
box's corners (one of the two choices of each decision whose margin was below the bound).
"""
import copy
import math

import numpy as np
import pytest

import mipgen_rule
import sampler_rule as R
from test_gpu_combiners import OPT_ALPHA, OPT_EDGE, S0, TEX0, cc

pytestmark = pytest.mark.gpu

W, H = 320, 180
DLOD, EPS = 2.0 ** -12, 2.0 ** -19
MIN_PIXELS = 15000                 # compared pixels per case (the floor covers about 3/4 of the picture)
MIN_EDGE = 300                     # pixels outside [0, n) on each side of an axis, where the mode must wrap / mirror / clamp
# Exempt pixels (diffuse + specular samples whose box holds more than one byte, as a fraction of both), first MI355X run:
#   POINT                        at most 0.032 %  (texel or level boundaries within the bound)
#   LINEAR, power-of-two sizes   at most 1.66 %, 2.17 % with uv near 4096  (lod +- DLOD times a level difference straddles a byte)
#   LINEAR, other sizes          at most 3.24 %  (DU, DV of a rounded u * w add to it)
# The bars sit just above; a systematic error (half a texel, a level, a mirrored row) moves far more pixels out of their box than these.
EXEMPT_POINT, EXEMPT_LINEAR, EXEMPT_LINEAR_NPOT = 0.001, 0.025, 0.035
VERTEX = np.dtype([("position", "<f4", 4), ("normal", "<f4", 3), ("uv", "<f4", 2)])
SHADER = cc((S0, S0, S0, TEX0))
SHADER_EDGE = cc((S0, S0, S0, TEX0), (S0, S0, S0, TEX0), OPT_ALPHA | OPT_EDGE)


# ---- textures --------------------------------------------------------------------------------------------------------------------------

def _smooth(rng, w, h, alpha=255):
    """Random colours on a 4-texel lattice, interpolated, plus a little noise: slopes of tens of bytes per texel (a half-texel shift moves
    most pixels by several bytes) with few byte-rounding ties."""
    gx, gy = w // 4 + 2, h // 4 + 2
    lat = rng.integers(0, 256, (gy, gx, 4)).astype(np.float64)
    xs = np.arange(w) / 4.0; ys = np.arange(h) / 4.0
    x0 = np.floor(xs).astype(int); y0 = np.floor(ys).astype(int); fx = (xs - x0)[None, :, None]; fy = (ys - y0)[:, None, None]
    a = lat[y0][:, x0] * (1 - fx) + lat[y0][:, x0 + 1] * fx
    b = lat[y0 + 1][:, x0] * (1 - fx) + lat[y0 + 1][:, x0 + 1] * fx
    img = a * (1 - fy) + b * fy + rng.integers(-6, 7, (h, w, 4))
    img = np.clip(np.round(img), 0, 255).astype(np.uint8)
    if alpha is not None:
        img[..., 3] = alpha
    return img


def _tex_rgba8(name, img):
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    return sample_scene.TextureData(name, rt64.TEXTURE_FORMAT_RGBA8, img, img.shape[1], img.shape[0])


def _tex_dds(name, rng, w, h, levels=None):
    """An RGBA8 DDS chain: the M2-M4 averages of a smooth image, each level tinted by its own offset so that a wrong level is visible."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    chain = mipgen_rule.chain(_smooth(rng, w, h))[:levels]
    for l, lv in enumerate(chain):
        lv[..., :3] = np.clip(lv[..., :3].astype(int) * 3 // 4 + 24 * l, 0, 255).astype(np.uint8)
    return sample_scene.TextureData(name, rt64.TEXTURE_FORMAT_DDS, mipgen_rule.dds_rgba8(chain))


def _textures(kind, rng):
    """(diffuse, specular) TextureData of a case; 'gen' textures are RGBA8 that the device gives a chain (generate_mipmaps 1)."""
    if kind == "pow2":
        return _tex_rgba8("dif64", _smooth(rng, 64, 64)), _tex_rgba8("spc32x16", _smooth(rng, 32, 16))
    if kind == "npot":
        return _tex_dds("dif100x60", rng, 100, 60), _tex_dds("spc37x91", rng, 37, 91)
    if kind == "thin_npot":
        return _tex_dds("dif1x37", rng, 1, 37), _tex_dds("spc1x1", rng, 1, 1)
    if kind == "thin_pow2":
        return _tex_rgba8("dif1x64", _smooth(rng, 1, 64)), _tex_rgba8("spc64x1", _smooth(rng, 64, 1))
    if kind == "one_level":
        return _tex_dds("dif48x20", rng, 48, 20, levels=1), _tex_dds("spc1x1", rng, 1, 1)
    raise ValueError(kind)


# ---- geometry ------------------------------------------------------------------------------------------------------------------------

def _plane(origin, axis_a, axis_b, uv_a, uv_b, uv0, facing, cells=6):
    """A cells x cells grid over origin + s * axis_a + t * axis_b, uv = uv0 + s * uv_a + t * uv_b, wound so that its front face (primary
    rays cull back faces) looks along `facing`."""
    s, t = np.meshgrid(np.linspace(0, 1, cells + 1), np.linspace(0, 1, cells + 1), indexing="xy")
    s, t = s.ravel()[:, None], t.ravel()[:, None]
    v = np.zeros(len(s), dtype=VERTEX)
    v["position"][:, :3] = np.asarray(origin) + s * np.asarray(axis_a) + t * np.asarray(axis_b)
    v["position"][:, 3] = 1.0
    n = np.cross(axis_a, axis_b); v["normal"] = n / np.linalg.norm(n)
    v["uv"] = (np.asarray(uv0) + s * np.asarray(uv_a) + t * np.asarray(uv_b)).astype(np.float32)
    g = cells + 1
    i, j = np.meshgrid(np.arange(cells), np.arange(cells), indexing="xy")
    v0 = (j * g + i).ravel(); v1 = v0 + 1; v2 = v0 + g; v3 = v2 + 1
    flip = np.dot(np.cross(axis_a, axis_b), facing) > 0          # (the sample's floor: +x, +z wound v2 v1 v0 faces +y)
    idx = np.stack([v0, v1, v2, v3, v2, v1] if flip else [v2, v1, v0, v1, v2, v3], axis=1).astype(np.uint32).ravel()
    return v, idx


def _view(eye, pitch_deg, yaw_deg=0.0):
    """Row-vector view matrix of a camera at `eye` looking pitch_deg below the horizon, turned yaw_deg to the left of -z."""
    p, y = math.radians(pitch_deg), math.radians(yaw_deg)
    f = np.array([-math.sin(y) * math.cos(p), -math.sin(p), -math.cos(y) * math.cos(p)])
    right = np.cross(f, [0.0, 1.0, 0.0]); right /= np.linalg.norm(right)
    up = np.cross(right, f)
    cam = np.eye(4); cam[0, :3], cam[1, :3], cam[2, :3], cam[3, :3] = right, up, -f, eye
    return np.linalg.inv(cam).astype(np.float32)


def _scene(sample_data, kind, filt, ha, va, uv_offset=0.0, uv_detail=1.7, layout="floor", rng=None):
    """SceneData: one or two textured planes seen by a camera 2.5 above the floor; diffuse texture + specular map on every instance."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    rng = rng or np.random.default_rng(1)
    d = copy.copy(sample_data)
    dif, spc = _textures(kind, rng)
    d.textures = [dif, spc]
    d.sky = None
    d.shader_id = SHADER_EDGE if layout == "edge" else SHADER
    d.shader_filter, d.shader_haddr, d.shader_vaddr = filt, ha, va
    d.shader_flags = rt64.SHADER_RAYTRACE_ENABLED | rt64.SHADER_SPECULAR_MAP_ENABLED
    off = np.float32(uv_offset)
    # uv over the floor: u in [-1.44, 1.44], v in [-6.7, 1.7] (+ offset): several periods, negative values, both edges of [0, 1) crossed
    planes = [_plane((-12.0, 0.0, 2.0), (24.0, 0.0, 0.0), (0.0, 0.0, -84.0), (2.88, 0.0), (0.0, -8.4), (-1.44 + off, 1.7 + off), (0, 1, 0))]
    view = _view((0.0, 2.5, 4.0), 12.0)
    if layout == "wall":
        # a wall along the view direction on the left: the picture recedes across the screen, so rho comes from ddx
        planes.append(_plane((-3.0, -0.01, 2.0), (0.0, 0.0, -84.0), (0.0, 7.0, 0.0), (-8.4, 0.0), (0.0, 0.6), (1.3 + off, -0.2 + off), (1, 0, 0)))
        view = _view((0.0, 1.5, 4.0), 2.0, yaw_deg=-6.0)
    if layout == "edge":
        # the floor gets alpha holes; a second floor 0.7 below shows through them
        a = _smooth(rng, 64, 64, alpha=None)
        a[..., 3] = np.where(((np.arange(64)[:, None] // 8 + np.arange(64)[None, :] // 8) % 2) == 0, 255, 40)
        d.textures[0] = _tex_rgba8("dif64_holes", a)
        d.textures.append(_tex_rgba8("dif32_under", _smooth(rng, 32, 32)))
        planes.append(_plane((-30.0, -0.7, 2.0), (60.0, 0.0, 0.0), (0.0, 0.0, -84.0), (3.0, 0.0), (0.0, -6.0), (0.25, 0.5), (0, 1, 0)))
    d.meshes = [sample_scene.MeshData("plane%d" % k, rt64.MESH_RAYTRACE_ENABLED, v, i) for k, (v, i) in enumerate(planes)]
    d.instances = []
    for k in range(len(planes)):
        m = sample_scene.copy_material(sample_scene.base_material())
        m.uvDetailScale = uv_detail
        dif_k = 2 if (layout == "edge" and k == 1) else 0
        d.instances.append(sample_scene.InstanceData("plane%d" % k, k, np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32), dif_k, None, 1, m, 0))
    d.view = view
    return d


# ---- one frame against the rule ------------------------------------------------------------------------------------------------------

def _levels(lib, handle, tex):
    """Every level of a texture as RT64_ReadbackTexture returns it."""
    if tex.width > 0:
        w, h = tex.width, tex.height
    else:                                                   # DDS: height and width from the header
        hdr = np.frombuffer(tex.data[:20].tobytes(), dtype="<u4")
        h, w = int(hdr[3]), int(hdr[4])
    out, m = [], 0
    while True:
        n = lib.ReadbackTexture(handle, m, None, 0)
        if n == 0:
            return out
        mw, mh = max(1, w >> m), max(1, h >> m)
        assert n == mw * mh * 4
        a = np.zeros((mh, mw, 4), dtype=np.uint8)
        assert lib.ReadbackTexture(handle, m, a.ctypes.data, a.nbytes) == a.nbytes, lib.last_error()
        out.append(a)
        m += 1


def _render(rt64_lib, data, options=None, resolution_scale=1.0):
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    s = sample_scene.Rt64Scene(rt64_lib, data, W, H, hip_device=0, options=options)
    try:
        s.set_view_description(resolution_scale=resolution_scale)
        s.draw()
        img = {k: s.readback(getattr(rt64, "IMAGE_" + k)) for k in ("PRIMARY_HIT", "INSTANCE_ID", "DIFFUSE", "SHADING_SPECULAR")}
        levels = [_levels(rt64_lib, h, t) for h, t in zip(s.textures, data.textures)]
        st = s.stats()
    finally:
        s.close()
    return img, levels, st


def _coord_bound(u, n):
    """DU / DV of the module docstring."""
    return np.zeros_like(u) if n & (n - 1) == 0 else 2.0 ** -23 * (np.abs(u) + 1.0)


def _compare(levels, filt, ha, va, uv, ddx, ddy, got):
    """got [N, 3] bytes.  Returns (rule dict, strict [N], bad [N])."""
    u, v = uv[:, 0].astype(np.float64), uv[:, 1].astype(np.float64)
    h0, w0 = levels[0].shape[:2]
    r = R.sample_grad_bounds(levels, u, v, ddx, ddy, filt, ha, va, du=_coord_bound(u, w0), dv=_coord_bound(v, h0), dlod=DLOD, eps=EPS)
    lo, hi, byte = r["lo"][:, :3], r["hi"][:, :3], r["byte"][:, :3]
    strict = (lo == hi).all(axis=1)
    bad = (strict & (got != byte).any(axis=1)) | ~((got >= lo) & (got <= hi)).all(axis=1)
    if filt == R.POINT:
        bad |= ~(r["corners"][:, :, :3] == got[None]).all(axis=2).any(axis=0)
    return r, strict, bad


def _check_frame(data, img, levels, st, filt, ha, va, label, min_pixels=MIN_PIXELS, need_levels=2, coverage=True):
    """Compare the diffuse and specular samples of every hit pixel.  Returns a summary dict (printed)."""
    rw, rh = st.width, st.height
    hit, inst = img["PRIMARY_HIT"], img["INSTANCE_ID"]
    mask = (inst >= 0) & (hit[..., 3] != 0xFFFFFFFF)
    py, px = np.nonzero(mask)
    rec = hit[py, px]
    t = rec[:, 0].view(np.float32); bu = rec[:, 1].view(np.float32); bv = rec[:, 2].view(np.float32)
    prim = (rec[:, 3] & 0xFFFFFF).astype(np.int64)                         # (instance << 24) | primitive
    ins = inst[py, px]
    n = len(px)
    assert n >= min_pixels, (label, n)
    pos = np.zeros((n, 3, 3)); uvc = np.zeros((n, 3, 2), dtype=np.float32); dif_idx = np.zeros(n, dtype=np.int64); detail = np.zeros(n, dtype=np.float32)
    for k, instd in enumerate(data.instances):
        m = ins == k
        if not m.any():
            continue
        mesh = data.meshes[instd.mesh]
        idx = mesh.indices.astype(np.int64)[3 * prim[m][:, None] + np.arange(3)[None, :]]
        pos[m] = mesh.vertices["position"][idx][..., :3]
        uvc[m] = mesh.vertices["uv"][idx]
        dif_idx[m] = instd.diffuse
        detail[m] = np.float32(instd.material.uvDetailScale)
        assert np.array_equal(instd.transform, np.eye(4, dtype=np.float32))
    origin, D, dDdx, dDdy = R.primary_rays(data.view, data.fov, data.near, data.far, st.screenWidth, st.screenHeight, px, py, rw, rh)
    # the hit record, the vertex data and the rule's rays describe the same point
    b = np.stack([1.0 - bu.astype(np.float64) - bv, bu, bv], axis=1)
    p_bary = np.einsum("nk,nkj->nj", b, pos)
    p_ray = origin + D * t.astype(np.float64)[:, None]
    err = np.linalg.norm(p_bary - p_ray, axis=1) / np.maximum(np.linalg.norm(p_ray - origin, axis=1), 1.0)
    assert err.max() < 1e-4, (label, float(err.max()))
    ddx, ddy = R.texture_grads(D, t, dDdx, dDdy, pos, uvc, np.broadcast_to(np.eye(3), (n, 3, 3)), pos)
    uv = R.interpolate_uv_f32(uvc, bu, bv)
    out = dict(case=label, pixels=n, exempt=0, specular_exempt=0)
    got = img["DIFFUSE"][py, px, :3]
    gb = np.round(got * 255.0).astype(np.int64)
    assert np.abs(gb - got * 255.0).max() < 1e-3
    rules = {}
    for ti in np.unique(dif_idx):
        m = dif_idx == ti
        r, strict, bad = _compare(levels[ti], filt, ha, va, uv[m], ddx[m], ddy[m], gb[m])
        rules[int(ti)] = (m, r)
        out["exempt"] += int((~strict).sum())
        if bad.any():
            k = np.nonzero(bad)[0][:6]
            raise AssertionError("%s: %d of %d diffuse pixels differ from the rule (%d strict); first: %s" % (
                label, int(bad.sum()), int(m.sum()), int((bad & strict).sum()),
                [dict(px=int(px[m][i]), py=int(py[m][i]), gpu=gb[m][i].tolist(), rule=r["byte"][i, :3].tolist(), lo=r["lo"][i, :3].tolist(),
                      hi=r["hi"][i, :3].tolist(), lod=float(r["lod"][i]), uv=uv[m][i].tolist(), tex_margin=float(r["tex_margin"][i]),
                      lod_margin=float(r["lod_margin"][i])) for i in k]))
    # specular map: uv * uvDetailScale and gradients * uvDetailScale, stored as RGBA16F of byte / 255
    spec = img["SHADING_SPECULAR"][py, px, :3]
    sb = np.round(spec.astype(np.float64) * 255.0).astype(np.int64)
    assert np.abs(spec * 255.0 - sb).max() < 0.1                      # byte / 255 in float16: within 2^-12 of it
    suv = uv * detail[:, None]
    sd = detail.astype(np.float64)[:, None]
    r, strict, bad = _compare(levels[1], filt, ha, va, suv, ddx * sd, ddy * sd, sb)
    out["specular_exempt"] = int((~strict).sum())
    if bad.any():
        k = np.nonzero(bad)[0][:6]
        raise AssertionError("%s: %d of %d specular pixels differ from the rule; first: %s" % (
            label, int(bad.sum()), n, [dict(px=int(px[i]), py=int(py[i]), gpu=sb[i].tolist(), rule=r["byte"][i, :3].tolist(), lod=float(r["lod"][i]))
                                       for i in k]))
    # the sampler was exercised where it goes wrong: every addressing mode beyond both edges, several levels of a chain
    m0, r0 = rules[0]
    dl = levels[0]
    out["levels"] = sorted(set(np.unique(r0["level0"]).tolist()) | set(np.unique(r0["level1"]).tolist()))
    out["lod_range"] = (round(float(r0["raw_lod"][np.isfinite(r0["raw_lod"])].min()), 2), round(float(r0["raw_lod"].max()), 2))
    if len(dl) > 1:
        assert len(out["levels"]) >= need_levels, (label, out["levels"])
    if coverage:
        h0, w0 = dl[0].shape[:2]
        for name, raw, size in (("x", r0["raw_x"], np.maximum(w0 >> r0["level0"], 1)), ("y", r0["raw_y"], np.maximum(h0 >> r0["level0"], 1))):
            lo_n, hi_n = int((raw < 0).sum()), int((raw >= size).sum())
            out["beyond_" + name] = (lo_n, hi_n)
            assert lo_n >= MIN_EDGE and hi_n >= MIN_EDGE, (label, name, lo_n, hi_n)
    out["exempt_frac"] = round((out["exempt"] + out["specular_exempt"]) / (2.0 * n), 5)
    print("SAMPLER", out)
    pow2 = all(n & (n - 1) == 0 for lv in (levels[0], levels[1]) for n in lv[0].shape[:2])
    assert out["exempt_frac"] <= (EXEMPT_POINT if filt == R.POINT else (EXEMPT_LINEAR if pow2 else EXEMPT_LINEAR_NPOT)), out
    out.update(px=px, py=py, inst=ins, ddx=ddx, ddy=ddy, rule=r0, wh=(dl[0].shape[1], dl[0].shape[0]))
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------------

SAMPLERS = [(f, h, v) for f in (0, 1) for h in (0, 1, 2) for v in (0, 1, 2)]


@pytest.mark.parametrize("kind", ["pow2", "npot"])
@pytest.mark.parametrize("filt,ha,va", SAMPLERS, ids=["%s-%s-%s" % ("PL"[f], "WMC"[h], "WMC"[v]) for f, h, v in SAMPLERS])
def test_sampler_variant_per_pixel(rt64_lib, sample_data, filt, ha, va, kind):
    """All 18 filter x hAddr x vAddr variants on a receding floor (magnified in front, minified past the last level at the horizon), on
    power-of-two chains made by generate_mipmaps (mask addressing) and on non-power-of-two DDS chains down to 3x1 and 1x1 (integer remainder)."""
    rng = np.random.default_rng(500 + 9 * filt + 3 * ha + va)
    data = _scene(sample_data, kind, filt, ha, va, rng=rng)
    img, levels, st = _render(rt64_lib, data, options={"generate_mipmaps": 1})
    assert len(levels[0]) == 7
    out = _check_frame(data, img, levels, st, filt, ha, va, "%s %s" % (kind, "PL"[filt] + "WMC"[ha] + "WMC"[va]), need_levels=5)
    r0 = out["rule"]
    assert out["lod_range"][0] < -0.5 and out["lod_range"][1] > len(levels[0]) - 1     # magnification and minification past the last level
    if filt == 0:
        lv = r0["level0"]
        assert all((lv == l).sum() > 200 for l in range(4)), np.bincount(lv)          # point levels on both sides of several lod + 0.5 boundaries


@pytest.mark.parametrize("kind,filt,ha,va", [("pow2", 1, 0, 1), ("pow2", 0, 1, 0)])
def test_uv_offset_2p12(rt64_lib, sample_data, kind, filt, ha, va):
    """uv near 4096, where float32 uv has steps of 2^-12 (1/64 texel): the rule starts from the same float32 uv, and with power-of-two sizes
    the texel coordinate is exact, so every step shows.  (A non-power-of-two width rounds u * w by up to 0.05 texel there: nearly every
    pixel would be exempt.)"""
    rng = np.random.default_rng(4096 + filt)
    data = _scene(sample_data, kind, filt, ha, va, uv_offset=4096.0, rng=rng)
    img, levels, st = _render(rt64_lib, data, options={"generate_mipmaps": 1})
    _check_frame(data, img, levels, st, filt, ha, va, "uv+4096 %s %s" % (kind, "PL"[filt] + "WMC"[ha] + "WMC"[va]), need_levels=5,
                 coverage=False)


@pytest.mark.parametrize("kind", ["thin_npot", "thin_pow2", "one_level"])
@pytest.mark.parametrize("filt,ha,va", [(1, 1, 2), (0, 2, 1), (1, 0, 0)], ids=["L-M-C", "P-C-M", "L-W-W"])
def test_thin_and_single_level_textures(rt64_lib, sample_data, kind, filt, ha, va):
    """1 x 37 and 1 x 64 chains (every level one texel wide: wrap / mirror / clamp of an axis of 1), a 1 x 1 and a 64 x 1 specular map,
    and textures with a single level (no lod at all)."""
    rng = np.random.default_rng(37 + filt)
    data = _scene(sample_data, kind, filt, ha, va, rng=rng)
    img, levels, st = _render(rt64_lib, data, options={"generate_mipmaps": 1})
    _check_frame(data, img, levels, st, filt, ha, va, "%s %s" % (kind, "PL"[filt] + "WMC"[ha] + "WMC"[va]), need_levels=3, coverage=False)


@pytest.mark.parametrize("filt", [1, 0], ids=["linear", "point"])
def test_grazing_wall_takes_rho_from_ddx(rt64_lib, sample_data, filt):
    """A wall receding across the screen beside a floor receding up it: on the wall the footprint's long axis is the screen's x."""
    rng = np.random.default_rng(77 + filt)
    data = _scene(sample_data, "pow2", filt, 0, 1, layout="wall", rng=rng)
    img, levels, st = _render(rt64_lib, data, options={"generate_mipmaps": 1})
    out = _check_frame(data, img, levels, st, filt, 0, 1, "wall %s" % "PL"[filt], min_pixels=12000, coverage=False)
    wall = out["inst"] == 1
    assert wall.sum() > 3000
    wh = np.array(out["wh"], dtype=np.float64)
    fx, fy = np.linalg.norm(out["ddx"][wall] * wh, axis=1), np.linalg.norm(out["ddy"][wall] * wh, axis=1)
    assert (fx > 2.0 * fy).mean() > 0.5                                      # on the wall rho comes from ddx ...
    floor = out["inst"] == 0
    assert (np.linalg.norm(out["ddy"][floor] * wh, axis=1) > 2.0 * np.linalg.norm(out["ddx"][floor] * wh, axis=1)).mean() > 0.5   # ... on the floor from ddy
    assert np.unique(out["rule"]["level0"][wall]).size >= 4


@pytest.mark.parametrize("name,options,rs", [
    ("fused_lean 0", {"fused_lean": 0}, 1.0),
    ("simple_kernels 0", {"simple_kernels": 0}, 1.0),
    ("resolution_scale 0.75", {}, 0.75),
])
@pytest.mark.parametrize("filt,ha,va", [(1, 1, 0), (0, 0, 2)], ids=["L-M-W", "P-W-C"])
def test_kernel_paths(rt64_lib, sample_data, name, options, rs, filt, ha, va):
    """The separate primary_trace + primary_shade kernels, the general kernels on an all-power-of-two scene, and a render smaller than the
    screen (the ray differentials use resolution.zw, the screen size, and the pixel position the render size)."""
    rng = np.random.default_rng(900 + filt)
    data = _scene(sample_data, "pow2", filt, ha, va, rng=rng)
    img, levels, st = _render(rt64_lib, data, options=dict(options, generate_mipmaps=1), resolution_scale=rs)
    if rs != 1.0:
        assert (st.width, st.height) == (240, 135) and (st.screenWidth, st.screenHeight) == (W, H)
    _check_frame(data, img, levels, st, filt, ha, va, "%s %s" % (name, "PL"[filt] + "WMC"[ha] + "WMC"[va]),
                 min_pixels=int(MIN_PIXELS * rs * rs), need_levels=5)


@pytest.mark.parametrize("filt", [1, 0], ids=["linear", "point"])
def test_texture_edge_keeps_the_sampled_hit(rt64_lib, sample_data, filt):
    """Texture-edge any-hit (OPT_EDGE: a hit-list frame): the floor has alpha holes and a second floor shows through.  The kept hit's colour is
    its sample, and the rule's alpha at every kept floor hit is above 0.3."""
    rng = np.random.default_rng(300 + filt)
    data = _scene(sample_data, "pow2", filt, 0, 1, layout="edge", rng=rng)
    img, levels, st = _render(rt64_lib, data, options={"generate_mipmaps": 1})
    out = _check_frame(data, img, levels, st, filt, 0, 1, "edge %s" % "PL"[filt], coverage=False)
    top, under = int((out["inst"] == 0).sum()), int((out["inst"] == 1).sum())
    assert top > 5000 and under > 5000, (top, under)
    assert (out["rule"]["vmax"][:, 3] > 0.3).all()                          # the rule rows of texture 0 are the kept floor hits
