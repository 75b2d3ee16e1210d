"""Debug views (device option visualization_mode) and the motion blur tap count (device option motion_blur_samples).

visualization_mode m = 1..16 draws DebugPS.hlsl:47-157 in PostProcess's place (rt64_view.cpp:1628-1650): the image RT64_IMAGE_* = m of the same frame, read
nearest at render pixel uint2(uv * resolution.xy) (zeros out of range), shown as DebugPS shows it and alpha-blended over the back buffer the background pass
left (alphaBlendDesc, rt64_device.cpp:532-538); the foreground list goes on top.  The expectation below restates DebugPS in numpy from the frame's own
RT64_ReadbackDevice images, in fp32 like the shader."""

import numpy as np
import pytest

from test_gpu_features import _variant, _rmse

pytestmark = pytest.mark.gpu

W, H = 256, 144
MODES = range(1, 17)
CLEARED = np.array([0, 0, 0, 255], dtype=np.uint8)


def _no_hud(d):
    d.instances = [i for i in d.instances if not i.name.startswith("hud")]


def _mirrors(d):
    """Glass / mirror scene: the floor mirrors, the sphere refracts and reflects (test_gpu_features.test_fog_reflection_refraction without fog)."""
    _no_hud(d)
    for i in d.instances:
        if i.name == "floor":
            i.material.reflectionFactor = 0.6; i.material.reflectionShineFactor = 0.2
        if i.name == "sphere":
            i.material.refractionFactor = 0.9; i.material.solidAlphaMultiplier = 0.6; i.material.reflectionFactor = 0.3


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _to_unorm8(x):
    x = _f32(x)
    with np.errstate(invalid="ignore"):
        q = np.floor(x * np.float32(255.0) + np.float32(0.5))
        return np.where(~(x > 0), 0, np.where(x >= 1, 255, q)).astype(np.uint8)


def _instance_colours(ids, oracle_lib):
    import ctypes as C
    out = {}
    for i in np.unique(ids):
        if i < 0:
            continue
        seed = C.c_uint32(oracle_lib.oracle_init_rand(int(i), 0, 16))
        out[int(i)] = [oracle_lib.oracle_next_rand(C.byref(seed)) for _ in range(3)]
    return out


def debug_expect(mode, img, under, oracle_lib, scissor=None, viewport=None):
    """DebugPS for visualization mode `mode` over the RGBA8 back buffer `under` (screen size).  img: the readback of image `mode` (render size).
    scissor (x0, y0, x1, y1) / viewport (x, y, w, h): the rectangles of the ray-traced picture, top-left origin (default: the screen).
    Returns the expected back buffer and, for mode 13, the pixels whose float64 line distance is within 1e-3 of 1 (either result is right there)."""
    sh, sw = under.shape[:2]
    rh, rw = img.shape[:2]
    scissor = scissor or (0, 0, sw, sh)
    vx, vy, vw, vh = [np.float32(v) for v in (viewport or (0, 0, sw, sh))]
    cx = (np.arange(sw, dtype=np.float32) + np.float32(0.5))[None, :]
    cy = (np.arange(sh, dtype=np.float32) + np.float32(0.5))[:, None]
    xs, ys = np.arange(sw)[None, :], np.arange(sh)[:, None]
    inside = (xs >= scissor[0]) & (xs < scissor[2]) & (ys >= scissor[1]) & (ys < scissor[3])
    inside &= (cx >= vx) & (cx < vx + vw) & (cy >= vy) & (cy < vy + vh)
    u, v = (cx - vx) / vw, (cy - vy) / vh
    px, py = np.broadcast_to(u * np.float32(rw), (sh, sw)), np.broadcast_to(v * np.float32(rh), (sh, sw))

    def texel(tx, ty):
        ok = (tx >= 0) & (tx < rw) & (ty >= 0) & (ty < rh)
        val = img[np.clip(ty, 0, rh - 1), np.clip(tx, 0, rw - 1)]
        return np.where(ok[..., None] if val.ndim == 3 else ok, val, 0)

    ambiguous = np.zeros((sh, sw), dtype=bool)
    if mode == 13:      # getMotionVector: 1-px line from the 32 x 32 block centre along the flow sampled there
        sx = np.floor(px / np.float32(32)) * np.float32(32) + np.float32(16)
        sy = np.floor(py / np.float32(32)) * np.float32(32) + np.float32(16)
        fl = texel(sx.astype(np.int64), sy.astype(np.int64)).astype(np.float64)
        s = np.stack([sx, sy], -1).astype(np.float64); e = s + fl; p = np.stack([px, py], -1).astype(np.float64)
        l2 = ((e - s) ** 2).sum(-1)
        t = np.clip(((p - s) * (e - s)).sum(-1) / np.where(l2 == 0, 1, l2), 0, 1)
        q = np.where((l2 == 0)[..., None], s, s + t[..., None] * (e - s))
        dist = np.sqrt(((p - q) ** 2).sum(-1))
        lit = dist < 1
        ambiguous = np.abs(dist - 1) < 1e-3
        c = np.where(lit[..., None], np.float32(1), np.float32(0)).repeat(4, -1).astype(np.float32)
    else:
        t = texel(px.astype(np.int64), py.astype(np.int64))
        c = np.zeros((sh, sw, 4), dtype=np.float32); c[..., 3] = 1
        if mode == 5:    # getInstanceId: a colour per instance, nothing on a miss
            colours = _instance_colours(t, oracle_lib)
            for i, rgb in colours.items():
                c[t == i, :3] = rgb
            c[t < 0] = 0
        elif mode in (14, 15, 16):
            c[..., :3] = t[..., None]
        elif mode == 2:
            c[..., :3] = (_f32(t[..., :3]) + np.float32(1)) / np.float32(2)
        else:
            c[..., :3] = t[..., :3]
    with np.errstate(invalid="ignore"):
        c = np.where(c > 0, np.minimum(c, np.float32(1)), np.float32(0)).astype(np.float32)
    a = c[..., 3:4]
    d = under.astype(np.float32) / np.float32(255)
    out = np.concatenate([c[..., :3] * a + d[..., :3] * (np.float32(1) - a), a + d[..., 3:4] * (np.float32(1) - a)], -1)
    return np.where(inside[..., None], _to_unorm8(out), under), ambiguous & inside


def assert_debug_equal(got, exp, ambiguous=None):
    d = np.abs(got.astype(np.int32) - exp.astype(np.int32)).max(-1)
    if ambiguous is not None:
        d[ambiguous] = 0
    assert d.max() <= 1 and (d > 0).mean() <= 1e-4, (int(d.max()), float((d > 0).mean()))


def _scene(rt64_lib, data, w=W, h=H, view_desc=None):
    from sm64rt_legacy_renderer_amd import sample_scene
    s = sample_scene.Rt64Scene(rt64_lib, data, w, h, hip_device=0)
    if view_desc:
        s.set_view_description(**view_desc)
    return s


def _check_all_modes(rt64_lib, oracle_lib, data, warmup=1, view_desc=None, scissor=None, viewport=None, stats=None):
    """One device: `warmup` frames in mode 0, then one frame in each mode; each back buffer against DebugPS of that frame's image over the cleared buffer."""
    from sm64rt_legacy_renderer_amd import rt64
    s = _scene(rt64_lib, data, view_desc=view_desc)
    try:
        for _ in range(warmup):
            s.draw()
        for m in MODES:
            assert s.option("visualization_mode", m) == 1
            s.draw()
            st = s.stats()
            assert st.leanFrame == 0 and st.fusedFrame == 0 and st.packedFinal == 0
            if stats:
                stats(st)
            final = s.readback(rt64.IMAGE_FINAL_RGBA8)
            exp, amb = debug_expect(m, s.readback(m), np.broadcast_to(CLEARED, final.shape), oracle_lib, scissor, viewport)
            assert_debug_equal(final, exp, amb if m == 13 else None)
    finally:
        s.close()


def test_every_mode_on_the_lean_sample_frame(rt64_lib, oracle_lib, sample_data):
    """(a) the sample scene: lean / one-kernel in mode 0, a frame of the separate kernels in a debug mode."""
    from sm64rt_legacy_renderer_amd import rt64
    data = _variant(sample_data, _no_hud)
    s = _scene(rt64_lib, data)
    try:
        s.draw(); s.draw()
        assert s.stats().leanFrame == 1 and s.stats().fusedFrame == 1
        normal = s.readback(rt64.IMAGE_FINAL_RGBA8)
    finally:
        s.close()
    _check_all_modes(rt64_lib, oracle_lib, data)
    # the view really replaced the frame: the instance view of a frame is not its composed picture
    s = _scene(rt64_lib, data)
    try:
        s.option("visualization_mode", 5); s.draw()
        assert np.abs(s.readback(rt64.IMAGE_FINAL_RGBA8).astype(np.int32) - normal.astype(np.int32)).max() > 64
    finally:
        s.close()


def test_every_mode_on_a_gi_svgf_frame(rt64_lib, oracle_lib, sample_data):
    """(b) one GI sample + SVGF, three frames of history: the light images and the denoiser's output."""
    _check_all_modes(rt64_lib, oracle_lib, _variant(sample_data, _no_hud), warmup=2, view_desc=dict(gi_samples=1, denoiser=True))


def test_every_mode_on_a_glass_and_mirror_frame_shows_the_g_buffer_after_reflection(rt64_lib, oracle_lib, sample_data):
    """(c) reflections rewrite position / normal / instance id of mirrored pixels (ReflectionRayGen.hlsl:117-124): modes 1, 2 and 5 show the rewritten
    G-buffer, which differs from the first hit's on the mirror."""
    from sm64rt_legacy_renderer_amd import rt64
    data = _variant(sample_data, _mirrors)
    _check_all_modes(rt64_lib, oracle_lib, data)
    s = _scene(rt64_lib, data)
    try:
        s.draw()
        ids, first = s.readback(rt64.IMAGE_INSTANCE_ID), s.readback(rt64.IMAGE_FIRST_INSTANCE_ID)
        assert (ids != first).mean() > 0.01
    finally:
        s.close()


@pytest.mark.parametrize("view_desc", [dict(resolution_scale=0.75), dict(resolution_scale=1.5), "upscaler"])
def test_every_mode_with_a_render_size_other_than_the_screen(rt64_lib, oracle_lib, sample_data, view_desc):
    """(d) resolutionScale and the built-in upscaler: the view reads the render-size image at uint2(uv * resolution.xy)."""
    from sm64rt_legacy_renderer_amd import rt64
    if view_desc == "upscaler":
        view_desc = dict(upscaler=rt64.UPSCALER_FSR, upscaler_mode=rt64.UPSCALER_MODE_PERFORMANCE)

    def sizes(st):
        assert (st.width, st.height) != (st.screenWidth, st.screenHeight)
    _check_all_modes(rt64_lib, oracle_lib, _variant(sample_data, _no_hud), view_desc=view_desc, stats=sizes)


def test_every_mode_inside_the_first_instances_viewport_and_scissor(rt64_lib, oracle_lib, sample_data):
    """(e) the view is drawn with the ray-traced picture's rectangles; the cleared buffer stays around them."""
    def mod(d):
        _no_hud(d)
        rt = next(i for i in d.instances if i.name == "sphere")
        rt.viewport = (30, 20, 180, 100)
        rt.scissor = (40, 25, 150, 80)
    # API rectangles have a bottom-left origin (rt64_view.cpp:1258-1271): top-left rows are H - y - h
    _check_all_modes(rt64_lib, oracle_lib, _variant(sample_data, mod), scissor=(40, H - 25 - 80, 190, H - 25), viewport=(30, H - 20 - 100, 180, 100))


def test_alpha_zero_shows_the_background_pass_and_the_foreground_goes_on_top(rt64_lib, oracle_lib, sample_data):
    """Misses of the instance view and pixels off the flow lines have alpha 0: the cleared buffer and the background instances show there (the
    back buffer of the same background list with nothing ray traced).  The opaque foreground HUD is drawn over the view as over the frame."""
    from sm64rt_legacy_renderer_amd import rt64
    bg_only = _variant(sample_data, lambda d: setattr(d, "instances", [i for i in d.instances if i.name == "hudA"]))
    fg_only = _variant(sample_data, lambda d: setattr(d, "instances", [i for i in d.instances if i.name == "hudB"]))
    finals = {}
    for name, data in (("bg", bg_only), ("fg", fg_only)):
        s = _scene(rt64_lib, data)
        try:
            s.draw()
            finals[name] = s.readback(rt64.IMAGE_FINAL_RGBA8).copy()
        finally:
            s.close()
    under = finals["bg"]
    assert (under != CLEARED).any(-1).sum() > 100
    covered = (finals["fg"] != CLEARED).any(-1)
    assert covered.sum() > 100
    no_fg = _variant(sample_data, lambda d: setattr(d, "instances", [i for i in d.instances if i.name != "hudB"]))
    for data, fg in ((no_fg, False), (sample_data, True)):
        s0 = _scene(rt64_lib, data)
        try:
            s0.draw()
            normal = s0.readback(rt64.IMAGE_FINAL_RGBA8).copy()
        finally:
            s0.close()
        for m in (5, 13):
            s = _scene(rt64_lib, data)
            try:
                assert s.option("visualization_mode", m) == 1
                s.draw()
                final = s.readback(rt64.IMAGE_FINAL_RGBA8)
                exp, amb = debug_expect(m, s.readback(m), under, oracle_lib)
                amb = amb if m == 13 else None
                if m == 5:
                    assert (s.readback(rt64.IMAGE_INSTANCE_ID) < 0).sum() > 100                   # misses: alpha 0
                else:
                    assert ((exp == under).all(-1) & (under != CLEARED).any(-1)).sum() > 20      # off the lines, over the background HUD
                if fg:
                    assert np.array_equal(final[covered], normal[covered])
                    assert_debug_equal(np.where(covered[..., None], exp, final), exp, amb)
                else:
                    assert_debug_equal(final, exp, amb)
            finally:
                s.close()


def _all_images(s):
    from sm64rt_legacy_renderer_amd import rt64
    return {i: s.readback(i).copy() for i in range(1, 21)}


@pytest.mark.parametrize("scene", ["sample", "gi"])
def test_debug_frames_change_nothing_but_their_back_buffer(rt64_lib, sample_data, scene):
    """Two devices on the same calls; one shows modes {1, 5, 9, 13, 16} for two frames each and returns to mode 0.  Every image but the back buffer
    is the same bytes on both throughout, and every back buffer outside the debug frames too (history, accumulations, frame count, RNG untouched)."""
    from sm64rt_legacy_renderer_amd import rt64
    data = _variant(sample_data, lambda d: None)
    vd = dict(gi_samples=1, denoiser=True) if scene == "gi" else None
    a, b = _scene(rt64_lib, data, view_desc=vd), _scene(rt64_lib, data, view_desc=vd)
    try:
        f = 0
        for m in (1, 5, 9, 13, 16):
            for mode in (0, m, m, 0, 0):
                assert b.option("visualization_mode", mode) == 1
                a.draw(); b.draw()
                sa, sb = a.stats(), b.stats()
                if mode:
                    assert sb.leanFrame == 0 and sb.fusedFrame == 0 and sb.packedFinal == 0
                else:
                    assert (sb.leanFrame, sb.fusedFrame) == (sa.leanFrame, sa.fusedFrame)
                    assert np.array_equal(a.readback(rt64.IMAGE_FINAL_RGBA8), b.readback(rt64.IMAGE_FINAL_RGBA8)), (m, f)
                if scene == "sample" and f % 5 == 4:
                    assert sb.leanFrame == 1 and sb.fusedFrame == 1
                ia, ib = _all_images(a), _all_images(b)
                for k in ia:
                    assert np.array_equal(ia[k].view(np.uint8), ib[k].view(np.uint8)), (m, mode, f, k)
                f += 1
    finally:
        a.close(); b.close()


def _partition_final(rt64_lib, data, mode, parts, vd=None, bands=True):
    from sm64rt_legacy_renderer_amd import rt64, tiles
    out = np.zeros((H, W, 4), dtype=np.uint8)
    for r in range(parts):
        s = _scene(rt64_lib, data, view_desc=vd)
        try:
            assert s.option("visualization_mode", mode) == 1
            if bands:
                y0, y1 = tiles.band_range(H, r, parts)
                s.set_tile(y0, y1)
                rows = [(y0, y1)]
            else:
                s.set_interleave(r, parts)
                rows = tiles.strip_ranges(H, r, parts)
            for _ in range(3):
                s.draw()
            mine = s.readback(rt64.IMAGE_FINAL_RGBA8)
            assert mine.shape[0] == sum(b - a for a, b in rows)
            k = 0
            for a, b in rows:
                out[a:b] = mine[k:k + b - a]; k += b - a
        finally:
            s.close()
    return out


def test_partitions_reassemble_the_whole_frame_debug_view(rt64_lib, sample_data):
    """3-way bands and 3-way interleaved strips, each device drawing its own rows of the view: together the whole frame's view.  The flow view is
    refused on a partitioned device (a row's line depends on the flow of its block's centre row, which another device may own)."""
    from sm64rt_legacy_renderer_amd import rt64
    data = _variant(sample_data, lambda d: None)
    gi = dict(gi_samples=1, denoiser=True)
    for mode, vd, layouts in ((2, None, (True, False)), (5, None, (True, False)), (9, gi, (True,))):
        s = _scene(rt64_lib, data, view_desc=vd)
        try:
            s.option("visualization_mode", mode)
            for _ in range(3):
                s.draw()
            whole = s.readback(rt64.IMAGE_FINAL_RGBA8).copy()
        finally:
            s.close()
        for bands in layouts:
            assert np.array_equal(_partition_final(rt64_lib, data, mode, 3, vd, bands), whole), (mode, bands)
    s = _scene(rt64_lib, data)
    try:
        s.set_tile(0, 48)
        s.draw()
        before = s.readback(rt64.IMAGE_FINAL_RGBA8).copy()
        assert s.option("visualization_mode", 13) == 1
        s.draw()
        assert "visualization_mode 13" in rt64_lib.last_error()
        assert np.array_equal(s.readback(rt64.IMAGE_FINAL_RGBA8), before)          # the device still shows its last complete frame
    finally:
        s.close()


def test_out_of_range_option_values_are_refused_and_change_nothing(rt64_lib, sample_data):
    """Both keys refuse what is outside their range (visualization_mode 0..16, motion_blur_samples 0..1024, whole numbers) and keep their value:
    the same calls without the refused ones give the same back buffers -- two debug frames, then a blurred frame of a moving camera."""
    from sm64rt_legacy_renderer_amd import rt64
    data = _variant(sample_data, _no_hud)
    base = data.view.copy()
    finals = []
    for probe in (True, False):
        s = _scene(rt64_lib, data, view_desc=dict(motion_blur=1.0))
        try:
            assert s.option("visualization_mode", 3) == 1 and s.option("motion_blur_samples", 7) == 1
            if probe:
                for bad in (-1, 17, 2.5, 1e9, float("nan")):
                    assert s.option("visualization_mode", bad) == 0, bad
                for bad in (-1, 1025, 3.5, float("nan")):
                    assert s.option("motion_blur_samples", bad) == 0, bad
            frames = []
            for f in range(3):
                if f == 2:
                    assert s.option("visualization_mode", 0) == 1
                v = base.copy(); v[3, 0] = base[3, 0] - 0.35 * f; data.view = v
                s.draw()
                frames.append(s.readback(rt64.IMAGE_FINAL_RGBA8).copy())
            finals.append(frames)
        finally:
            s.close(); data.view = base
    for x, y in zip(*finals):
        assert np.array_equal(x, y)


def test_motion_blur_samples_match_the_oracle(rt64_lib, sample_data):
    """PostProcessPS.hlsl:14-33 with motionBlurSamples taps, against the oracle rendered with the same count (camera strafing, as in
    test_gpu_features.test_motion_blur_gathers_along_the_flow, at its tolerance)."""
    from sm64rt_legacy_renderer_amd import rt64
    from oracle import oracle_py
    data = _variant(sample_data, lambda d: None)
    base = data.view.copy()
    finals = {}
    for n in (1, 7, 64):
        s = _scene(rt64_lib, data, view_desc=dict(motion_blur=1.0))
        o = oracle_py.OracleScene(data)
        try:
            assert s.option("motion_blur_samples", n) == 1
            for f in range(3):
                v = base.copy(); v[3, 0] = base[3, 0] - 0.35 * f; data.view = v
                s.draw()
                ref = o.render(W, H, images=(f == 2), motionBlurStrength=1.0, motionBlurSamples=n)
            got_out, got = s.readback(rt64.IMAGE_OUTPUT_RGBA32F), s.readback(rt64.IMAGE_FINAL_RGBA8)
            assert np.abs(ref["flow"]).max() > 2.0
            assert _rmse(got_out[..., :3], ref["output"][..., :3]) <= 1e-3
            d = np.abs(got.astype(np.int32) - ref["final"].astype(np.int32))
            assert d.max() <= 2 and (d > 1).mean() < 1e-3, n
            finals[n] = got.copy()
        finally:
            s.close(); o.close(); data.view = base
    assert np.abs(finals[1].astype(np.int32) - finals[64].astype(np.int32)).mean() > 0.5
