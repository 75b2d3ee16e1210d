"""GPU parity of the per-pixel hit list when it runs over: the saturated sheet stacks of tests/test_oracle_kbuffer.py (20 and 40 translucent sheets
between the floor and the light) through every kernel that keeps the list -- primary trace, indirect (one and two bounces), reflection, refraction -- and shadow rays
through the stack.  Past 16 entries the result depends on the order in which hits arrive (slot 16, nhits; rt64_shader.cpp:553-580): this is where the
kernels and the oracle must agree on a traversal order of their own.

Every case is a hit-list frame: the sheets' alpha 0.1 makes an instance non-opaque, which sets the library's anyNonOpaque (View::update) -- the flag is
not visible from Python, the scene is built so that it cannot be anything else.  One light, so no light-selection threshold can flip."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_features import _rmse
from test_oracle_kbuffer import EDGE_SHADER_ID, W, H, covered_mask, floor_ray_mask, kbuffer_scene, render_oracle, set_edge_shader_oracle

pytestmark = pytest.mark.gpu

PIXEL_BAR = 2e-3            # per-pixel |output - oracle| on the saturated pixels: under half of one layer-17 contribution (0.9^16 x 0.1 x colour)


def _mirror_floor(d):
    d.instances[d.floor_instance].material.reflectionFactor = 0.5


def _refractive_top(d):
    m = d.instances[d.floor_instance + 1].material
    m.refractionFactor = 0.9


def _shadow_stack(d):
    for inst in d.instances[d.floor_instance + 1:]:
        inst.material.shadowAlphaMultiplier = 0.04                  # 20 layers: 1 - 0.96^20 = 0.56 of full shadow


# name -> (scene change, view description, device options, oracle overrides, frames).  Primary rays cross the stack in the upper half of the view;
# GI, mirror and shadow rays cross it on their way up from the floor in the lower half.
RAYS = {
    "primary": (None, None, {}, {}, 1),
    "gi_svgf": (None, dict(gi_samples=1, denoiser=True), {"denoiser_mode": 1}, dict(giSamples=1, denoiserEnabled=1, denoiserMode=1), 2),
    "gi_bounces2": (None, dict(gi_samples=1), {"gi_bounces": 2}, dict(giSamples=1, giBounces=2), 1),
    "mirror_overlap1": (_mirror_floor, None, {"overlap_reflection": 1}, {}, 1),
    "mirror_overlap0": (_mirror_floor, None, {"overlap_reflection": 0}, {}, 1),
    "refraction": (_refractive_top, None, {}, {}, 1),
    "shadow": (_shadow_stack, None, {}, {}, 1),
}
LAYOUTS = ("instances", "one_mesh", "depth_bias", "ignored_hits")
CASES = [(layout, 20, ray, {}) for layout in LAYOUTS for ray in RAYS]
CASES += [(layout, 40, ray, {}) for layout in LAYOUTS for ray in ("primary", "gi_svgf")]
CASES += [(layout, 20, ray, opts) for layout in ("instances", "one_mesh") for ray in ("primary", "gi_svgf")
          for opts in ({"lds_cache": 0}, {"host_tlas": 0})]


def _case_id(c):
    layout, K, ray, opts = c
    return "-".join([layout, "K%d" % K, ray] + ["%s%d" % kv for kv in opts.items()])


def _render(rt64_lib, data, ray, extra_opts):
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    from oracle import oracle_py
    _, view_desc, opts, ora_kw, frames = RAYS[ray]
    s = sample_scene.Rt64Scene(rt64_lib, data, W, H, hip_device=0)
    o = oracle_py.OracleScene(data)
    edge_shader = None
    try:
        set_edge_shader_oracle(o, data)
        if data.edge_instance is not None:             # the texture-edge sheet has a shader of its own (Rt64Scene gives every instance the scene's one shader)
            edge_shader = rt64_lib.CreateShader(s.device, EDGE_SHADER_ID, data.shader_filter, data.shader_haddr, data.shader_vaddr, data.shader_flags)
            assert edge_shader, rt64_lib.last_error()
            desc = s._instance_desc(data.instances[data.edge_instance]); desc.shader = edge_shader
            rt64_lib.SetInstanceDescription(s.instances[data.edge_instance], desc)
        if view_desc:
            s.set_view_description(**view_desc)
        for k, v in list(opts.items()) + list(extra_opts.items()):
            assert s.option(k, v), k
        s.option("count_traversal", 1)
        for f in range(frames):
            s.draw()
            ref = o.render(W, H, images=(f == frames - 1), **ora_kw)
        names = ("OUTPUT_RGBA32F", "FINAL_RGBA8", "INSTANCE_ID", "PRIMARY_HIT", "INDIRECT_LIGHT_FILTERED", "REFLECTION", "REFRACTION", "DIRECT_LIGHT_RAW")
        got = {k: s.readback(getattr(rt64, "IMAGE_" + k)) for k in names}
        return got, ref, s.stats()
    finally:
        if edge_shader:                                 # like Rt64Scene.close: shaders first, then the device
            rt64_lib.DestroyShader(edge_shader)
        s.close(); o.close()


@pytest.mark.parametrize("layout,K,ray,opts", CASES, ids=[_case_id(c) for c in CASES])
def test_saturated_hit_list_matches_the_oracle(rt64_lib, sample_data, layout, K, ray, opts):
    data = kbuffer_scene(sample_data, K, layout, mutate=RAYS[ray][0])
    sheets = [i for k, i in enumerate(data.instances) if k > data.floor_instance and k != data.edge_instance]
    assert sheets and all(i.material.solidAlphaMultiplier < 1.0 for i in sheets)        # non-opaque instances: a hit-list frame
    got, ref, st = _render(rt64_lib, data, ray, opts)
    plain = render_oracle(kbuffer_scene(sample_data, K, layout))     # the masks come from view directions without mirrors
    m = covered_mask(plain, data, K)
    assert m.sum() > 15000
    if ray.startswith("mirror") or ray == "shadow":
        f = floor_ray_mask(plain, data, K, "mirror" if ray.startswith("mirror") else "shadow")
        assert f.sum() > 5000
        m = m | f
    # hit records and traversal exactly
    assert np.array_equal(got["PRIMARY_HIT"], ref["primaryHit"])
    if ray not in ("mirror_overlap1", "mirror_overlap0"):           # reflection rewrites gInstanceId (ReflectionRayGen.hlsl:120)
        assert np.array_equal(got["INSTANCE_ID"], ref["instanceId"])
    c = ref["counters"]
    for k in ("primaryRays", "shadowRays", "indirectRays", "reflectionRays", "refractionRays", "nodesVisited", "trianglesTested"):
        assert getattr(st, k) == c[k], (k, getattr(st, k), c[k])
    # the images within the bars of their neighbouring tests (test_gpu_features)
    assert _rmse(got["OUTPUT_RGBA32F"][..., :3], ref["output"][..., :3]) <= 1e-3
    assert _rmse(got["FINAL_RGBA8"][..., :3] / 255.0, ref["final"][..., :3] / 255.0) <= 1e-3
    if ray.startswith("gi"):
        assert _rmse(got["INDIRECT_LIGHT_FILTERED"][..., :3], ref["filteredIndirect"][..., :3]) <= 2e-3
        assert st.indirectRays > 0
    if ray.startswith("mirror"):
        assert np.abs(got["REFLECTION"] - ref["reflection"]).max() < 8e-3 and st.reflectionRays > 0
    if ray == "refraction":
        assert np.abs(got["REFRACTION"] - ref["refraction"]).max() < 8e-3 and st.refractionRays > 0
    # ... and per pixel where the stack covers the ray: a wrong slot 16 or nhits moves such a pixel by ~0.0185 x colour
    d = np.abs(got["OUTPUT_RGBA32F"][..., :3] - ref["output"][..., :3]).max(axis=-1)[m]
    print("saturated pixels %d, largest output difference %.3g" % (int(m.sum()), float(d.max())))
    assert d.max() <= PIXEL_BAR, (float(d.max()), int((d > PIXEL_BAR).sum()))
