"""The GI filters pixel by pixel: SVGF (denoiser_mode 1, csrc/svgf.hip) and the reference's five GaussianFilterRGB3x3CS passes (denoiser_mode 0,
gaussian_kernel in csrc/passes.hip) against tests/denoise_rule.py, the float64 restatement of their specs, fed with the GPU's OWN filter inputs
(RT64_IMAGE_FILTER_GUIDE, RT64_IMAGE_GI_MOMENTS, RT64_IMAGE_FILTER_PING, RT64_IMAGE_INDIRECT_LIGHT_RAW).  What is left between the two sides is float32
arithmetic, the hardware exp2 / log2 and float16 rounding, so the bars are in float16 steps (ulps) per pixel and channel, not a whole-frame RMSE.
  guide       the records equal the rule's guide of DEPTH / INSTANCE_ID bit for bit (written by bounce_resolve_kernel or by svgf_guide_kernel);
  last pass   rule(FILTER_PING) = INDIRECT_LIGHT_FILTERED within 1 ulp on surface pixels, bit for bit on sky pixels;
  chain       variance + five iterations (or five Gaussian passes) from the raw image within CHAIN_ULPS_RGB / CHAIN_ULPS_VAR;
  compose     OUTPUT_RGBA32F = ComposePS restated in float32 from the readbacks, bit for bit (the folded Compose and its own launch)."""
import copy
import ctypes as C

import numpy as np
import pytest

import denoise_rule as R

pytestmark = pytest.mark.gpu

W, H = 320, 180
LAST_ULPS = 1
# Whole chain, per pixel and channel: the largest differences measured on the MI355X over this file's frames were 2 ulps in rgb (gi_bounces 2; 1 on
# every other frame) and 4 in the variance (the float32 mu2 - mu1^2 of the moments against float64, carried through five iterations with squared
# weights) for SVGF, 1 in rgb for the Gaussian.
CHAIN_ULPS_RGB = 3
CHAIN_ULPS_VAR = 4


def _variant(sample_data, fn=None):
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    d = copy.copy(sample_data)
    d.instances = [copy.copy(i) for i in sample_data.instances]
    for i in d.instances:
        i.material = sample_scene.copy_material(i.material)
    desc = rt64.SCENE_DESC(); C.memmove(C.byref(desc), C.byref(sample_data.desc), C.sizeof(rt64.SCENE_DESC)); d.desc = desc
    if fn:
        fn(d)
    return d


NAMES = ("DEPTH", "INSTANCE_ID", "FILTER_GUIDE", "FILTER_PING", "GI_MOMENTS", "INDIRECT_LIGHT_RAW", "INDIRECT_LIGHT_FILTERED")
COMPOSE = ("DIFFUSE", "DIRECT_LIGHT_FILTERED", "REFLECTION", "REFRACTION", "TRANSPARENT", "OUTPUT_RGBA32F")


class _Session:
    """One device per band (one for the whole frame without bands), GI with the denoiser."""

    def __init__(self, lib, data, w, h, mode=1, options=None, bands=None, gi_samples=1, resolution_scale=1.0):
        from sm64rt_legacy_renderer_amd import sample_scene
        self.data, self.bands = data, bands or [None]
        self.parts = []
        try:
            for band in self.bands:
                s = sample_scene.Rt64Scene(lib, data, w, h, hip_device=0)
                self.parts.append(s)
                s.set_view_description(gi_samples=gi_samples, denoiser=True, resolution_scale=resolution_scale)
                assert s.option("denoiser_mode", mode)
                for k, v in (options or {}).items():
                    assert s.option(k, v), k
                if band:
                    s.set_tile(*band)
        except Exception:
            self.close()
            raise

    def draw(self, can_reproject=True):
        for s in self.parts:
            s.draw(can_reproject)

    def read(self, names=NAMES):
        from sm64rt_legacy_renderer_amd import rt64
        return {k: np.concatenate([s.readback(getattr(rt64, "IMAGE_" + k)) for s in self.parts], axis=0) for k in names}

    def close(self):
        for s in self.parts:
            s.close()


def _ulps(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b) / R.f16_ulp(np.maximum(np.abs(a), np.abs(b)))


def check_guide(rb):
    """FILTER_GUIDE's valid flag, depth and depth gradient = the rule's guide of DEPTH and INSTANCE_ID, bit for bit."""
    got = np.asarray(rb["FILTER_GUIDE"], dtype=np.uint32)
    want = R.guide(rb["DEPTH"], rb["INSTANCE_ID"], np.zeros(rb["DEPTH"].shape + (3,)))
    assert np.array_equal((got[..., 1] >> 16) != 0, want["valid"]), "valid flag"
    assert np.array_equal(got[..., 2], np.asarray(rb["DEPTH"], dtype=np.float32).view(np.uint32)), "depth"
    gz = want["gz"].astype(np.float32).view(np.uint32)
    bad = got[..., 3] != gz
    assert not bad.any(), ("depth gradient", int(bad.sum()), np.argwhere(bad)[:5].tolist())


def check_svgf(rb, rows=None):
    """Last iteration and whole chain of SVGF against the rule; `rows` = the slice of rows to hold to it (a band's own rows).  Returns the largest
    differences in ulps (last pass, chain rgb, chain variance).
    Regression: svgf_atrous_kernel clamped the edge-stop exponent at 0 (exp2(min(e, 0))), so a tap whose max(0, n.n')^128 exceeds 1 (float16
    normals) weighed less than the spec says: up to 4 ulps off in the last pass, 11 in its variance, mostly on the frame's last row and column."""
    g = R.unpack_guide(rb["FILTER_GUIDE"])
    rows = rows or slice(None)
    valid = g["valid"][rows]
    filt = rb["INDIRECT_LIGHT_FILTERED"].astype(np.float64)
    last = R.atrous(rb["FILTER_PING"], g, 16)
    chain, _ = R.svgf(rb["INDIRECT_LIGHT_RAW"], rb["GI_MOMENTS"], g)
    dl = _ulps(last[rows], filt[rows])[valid]
    dc = _ulps(chain[rows], filt[rows])[valid]
    sky_last = np.array_equal(last[rows][~valid], filt[rows][~valid])
    sky_chain = np.array_equal(chain[rows][~valid], filt[rows][~valid])
    stats = (float(dl.max(initial=0.0)), float(dc[:, :3].max(initial=0.0)), float(dc[:, 3].max(initial=0.0)))
    print("svgf ulps: last %.0f, chain rgb %.0f variance %.0f (%d surface px)" % (stats + (int(valid.sum()),)))
    assert sky_last and sky_chain, ("sky pixels", sky_last, sky_chain)
    assert stats[0] <= LAST_ULPS, ("last pass", stats, np.argwhere(_ulps(last[rows], filt[rows]).max(axis=-1) * valid > LAST_ULPS)[:5].tolist())
    assert stats[1] <= CHAIN_ULPS_RGB and stats[2] <= CHAIN_ULPS_VAR, ("chain", stats)
    return stats


def check_gaussian(rb):
    """rgb of the last Gaussian pass and of the five passes from the raw image against the rule (the shader writes rgb only)."""
    filt = rb["INDIRECT_LIGHT_FILTERED"][..., :3].astype(np.float64)
    last = R.gaussian_pass(rb["FILTER_PING"])[..., :3]
    chain, ping = R.gaussian(rb["INDIRECT_LIGHT_RAW"])
    stats = (float(_ulps(last, filt).max()), float(_ulps(chain[..., :3], filt).max()))
    print("gaussian ulps: last %.0f, chain rgb %.0f" % stats)
    assert stats[0] <= LAST_ULPS, ("last pass", stats)
    assert stats[1] <= CHAIN_ULPS_RGB, ("chain", stats)
    assert np.array_equal(rb["FILTER_PING"][..., 3], rb["INDIRECT_LIGHT_RAW"][..., 3])      # image 0 = the raw image: alpha = its history
    return stats


def compose_rule(rb):
    """ComposePS (ComposePS.hlsl:18-37) in float32, in its order of operations, from the readbacks of its inputs."""
    f = lambda k: np.asarray(rb[k], dtype=np.float32)
    d = f("DIFFUSE"); dif = d[..., :3]
    res = dif * (f("DIRECT_LIGHT_FILTERED")[..., :3] + f("INDIRECT_LIGHT_FILTERED")[..., :3])
    res = dif + (res - dif) * d[..., 3:4]
    res = res + f("REFLECTION")[..., :3]
    res = res + f("REFRACTION")[..., :3]
    res = res + f("TRANSPARENT")[..., :3]
    out = np.ones(d.shape, dtype=np.float32)
    out[..., :3] = np.where(d[..., 3:4] > np.float32(1e-6), res, dif)
    return out


def _run(lib, data, w, h, frames, mode=1, options=None, bands=None, check_at=None, names=NAMES, **kw):
    """Draw `frames` frames; returns the readbacks after the frames listed in check_at (default: the last one)."""
    s = _Session(lib, data, w, h, mode=mode, options=options, bands=bands, **kw)
    out = {}
    try:
        for f in range(1, frames + 1):
            s.draw()
            if f in (check_at or (frames,)):
                out[f] = s.read(names)
    finally:
        s.close()
    return out


def _surface_mix(rb):
    hist = rb["INDIRECT_LIGHT_RAW"][..., 3]; valid = rb["INSTANCE_ID"] >= 0
    return int((valid & (hist < 4.0)).sum()), int((valid & (hist >= 4.0)).sum())


# ---- tests ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fold_guide", [1, 0])
def test_guide_records_equal_the_rule(rt64_lib, sample_data, fold_guide):
    """Written by bounce_resolve_kernel (fold_guide 1) or by svgf_guide_kernel (fold_guide 0): the same bits as the rule's guide, the depth
    gradient a forward difference clamped at the right and bottom edges -- on a ragged frame too."""
    for (w, h) in ((W, H), (33, 17)):
        rb = _run(rt64_lib, sample_data, w, h, 2, options={"fold_guide": fold_guide})[2]
        check_guide(rb)


def test_svgf_history_frames_static_camera(rt64_lib, sample_data):
    """Frames 1-6 of a static camera: every surface pixel is young (7x7 variance estimate) until its history reaches 4, then the variance comes from
    the moments.  Each frame: last iteration within 1 ulp, sky bit for bit, whole chain within CHAIN_ULPS_RGB / CHAIN_ULPS_VAR."""
    got = _run(rt64_lib, sample_data, W, H, 6, check_at=range(1, 7))
    for f, rb in got.items():
        check_guide(rb)
        check_svgf(rb)
    young1, old1 = _surface_mix(got[1])
    young6, old6 = _surface_mix(got[6])
    assert young1 > 0 and old1 == 0 and old6 > 0, (young1, old1, young6, old6)


@pytest.mark.parametrize("fold_variance", [1, 0])
def test_svgf_strafing_camera_and_moving_instance(rt64_lib, sample_data, fold_variance):
    """A camera that strafes and a sphere that moves: disocclusions mix young and old pixels inside one 32x8 workgroup of the variance kernel (the
    svgfYoung marks of bounce_resolve_kernel with fold_variance 1, every pixel again with 0); then one frame drawn with can_reproject = False (the history
    is reprojected with this frame's matrices instead of the previous ones), and one after it."""
    data = _variant(sample_data)
    k = next(i for i, inst in enumerate(data.instances) if inst.name == "sphere")
    s = _Session(rt64_lib, data, W, H, options={"fold_variance": fold_variance})
    checked = 0
    try:
        for f in range(9):
            v = data.view.copy(); v[3, 0] += 0.04 * f; data.view = v
            inst = copy.copy(data.instances[k])
            inst.previous_transform = inst.transform.copy()
            t = inst.transform.copy(); t[3, 1] += 0.05; inst.transform = t
            data.instances[k] = inst
            s.draw(can_reproject=(f != 6))
            if f in (5, 6, 7, 8):
                rb = s.read()
                check_svgf(rb)
                if f in (5, 8):
                    valid = rb["INSTANCE_ID"] >= 0
                    young = valid & (rb["INDIRECT_LIGHT_RAW"][..., 3] < 4.0); old = valid & ~young
                    hh, ww = (H + 7) // 8 * 8, (W + 31) // 32 * 32
                    tile = lambda m: np.pad(m, ((0, hh - H), (0, ww - W))).reshape(hh // 8, 8, ww // 32, 32).any(axis=(1, 3))
                    assert (tile(young) & tile(old)).any(), "no workgroup holds both young and old pixels"
                    checked += 1
    finally:
        s.close()
    assert checked == 2


@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (33, 17), (65, 9), (123, 77)])
def test_svgf_ragged_frames(rt64_lib, sample_data, w, h):
    """Sizes that cut the 64-wide a-trous rows and the 32x8 variance tile, down to one pixel; frames 3 and 6 (young / old history).
    Regression: with the exponent unbounded, 65x9 frame 3 came out with NaN pixels -- sky taps (weight 0) whose guide normal is no unit vector made
    exp2(e) overflow, and 0 * inf is NaN."""
    for rb in _run(rt64_lib, sample_data, w, h, 6, check_at=(3, 6)).values():
        assert rb["FILTER_GUIDE"].shape == (h, w, 4) and rb["GI_MOMENTS"].shape == (h, w, 2) and rb["FILTER_PING"].shape == (h, w, 4)
        check_guide(rb)
        check_svgf(rb)


def test_svgf_resolution_scale(rt64_lib, sample_data):
    """resolution_scale 0.75: the filter runs at the render size (240 x 135), which is what the debug images hold."""
    rb = _run(rt64_lib, sample_data, W, H, 5, resolution_scale=0.75)[5]
    assert rb["FILTER_GUIDE"].shape == (135, 240, 4)
    check_guide(rb)
    check_svgf(rb)


@pytest.mark.parametrize("variant", ["gi_bounces", "primary_spp", "mirror_floor"])
def test_svgf_path_variants(rt64_lib, sample_data, variant):
    """Two GI bounces; two primary samples per pixel (the filter runs once per sub-sample: the debug images and INDIRECT_LIGHT_FILTERED hold the
    last one); a mirror floor with overlap_reflection 1, whose reflection passes run beside the a-trous iterations (reflectBeside)."""
    data, options = sample_data, {}
    if variant == "gi_bounces":
        options = {"gi_bounces": 2}
    elif variant == "primary_spp":
        options = {"primary_spp": 2}
    else:
        def mirror(d):
            for inst in d.instances:
                if inst.name == "floor":
                    inst.material.reflectionFactor = 1.0
        data, options = _variant(sample_data, mirror), {"overlap_reflection": 1, "max_reflections": 2}
    rb = _run(rt64_lib, data, W, H, 5, options=options)[5]
    check_guide(rb)
    check_svgf(rb)


def test_svgf_two_bands(rt64_lib, sample_data):
    """Two devices, one band each (the halo re-rendered): each band's own rows against the rule applied to the bands' readbacks."""
    bands = [(0, 83), (83, H)]
    rb = _run(rt64_lib, sample_data, W, H, 5, bands=bands)[5]
    check_guide(rb)
    for y0, y1 in bands:
        check_svgf(rb, rows=slice(y0, y1))


@pytest.mark.parametrize("w,h", [(W, H), (33, 17), (7, 3), (1, 1), (5, 1), (1, 6)])
def test_gaussian_passes(rt64_lib, sample_data, w, h):
    """denoiser_mode 0: the last of the five GaussianFilterRGB3x3CS passes within 1 ulp of the rule applied to FILTER_PING, the five passes from the raw
    image within CHAIN_ULPS_RGB -- every border case, and the 1-wide / 1-high frames where the shader's branch order picks the case."""
    rb = _run(rt64_lib, sample_data, w, h, 3, mode=0)[3]
    check_gaussian(rb)


@pytest.mark.parametrize("fold_compose", [1, 0])
def test_compose_of_the_filtered_image(rt64_lib, sample_data, fold_compose):
    """OUTPUT_RGBA32F = ComposePS in float32 from DIFFUSE, DIRECT_LIGHT_FILTERED, INDIRECT_LIGHT_FILTERED, REFLECTION, REFRACTION and TRANSPARENT,
    bit for bit, whether the last a-trous iteration composes its pixel (fold_compose 1) or compose_post_kernel does."""
    def refl(d):
        for inst in d.instances:
            if inst.name == "floor":
                inst.material.reflectionFactor = 0.3
    rb = _run(rt64_lib, _variant(sample_data, refl), W, H, 5, options={"fold_compose": fold_compose}, names=NAMES + COMPOSE)[5]
    check_svgf(rb)
    want = compose_rule(rb)
    bad = rb["OUTPUT_RGBA32F"].view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (int(bad.sum()), np.abs(rb["OUTPUT_RGBA32F"] - want).max())
