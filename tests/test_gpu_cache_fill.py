"""The scene-cache fill of the CACHED ray kernels (fill_scene_cache, csrc/trace.h) at the edges of its chunking, and the foreground (HUD) record test of
raster_blend_pixel (csrc/raster_pixel.h) that reads a record's pixel box through scalar loads.

Fill: a workgroup of 256 threads copies the cache image in chunks of 256 16-byte words, at most six (RT_CACHE_MAX_WORDS = 1536); every thread issues all six
loads from an index clamped to the image's last word and stores only the words it owns.  The scenes below put the word count
4 m + 4 max(m - 1, 1) + 4 sum(max(T - 1, 1)) (m ray-traced instances of T triangles each) on those edges:

    12    one instance of one triangle              three of the four waves store nothing and still reach the barrier
    256   meshes of 32 and 31 triangles             exactly one chunk
    260   33 and 31                                 one chunk and a partial one
    1292  the sample scene (320 and 2)              the benchmark's own shape
    1536  300 and 83                                the maximum: every thread stores six words
    1540  300 and 84                                over the maximum: the cache stays off, `lds_cache` must change nothing

What is compared is `lds_cache = 1` against `lds_cache = 0` (the same walk from HBM / L2): the back buffer byte for byte and every traversal counter of
`count_traversal = 1`, on the one-kernel lean frame, on the same frame with `max_frame_groups = 4` (one fill serves several tiles), on a frame with one GI sample
and the denoiser (the cached bounce kernels) and on one RT64_TraceViewRays batch (the query kernels' fill).  A word of the image that lands in the wrong place, or
does not land, is a wrong node or instance record: the walk then visits other nodes, and the counters and the picture differ.

A case whose cache is silently off would prove nothing, so every case asserts the word count from the frame statistics (instanceCount, tlasNodeBytes,
blasNodeBytes) and the second half of the host's enabling rule, TLAS depth + deepest BLAS <= 16, from RT64_MeshTreeDepth -- a pure host function, the depth
RT64_SetMesh itself derives.  The meshes are regular grids cut off after T triangles; on the CPU (no device needed) RT64_MeshTreeDepth gives 1 for the
one-triangle mesh, 5 / 6 / 9 for the walls of 32 / 33 / 300 triangles, 5 / 7 / 7 for the floors of 31 / 83 / 84 and 10 / 1 for the sample's sphere and floor:
with the one TLAS level of two instances at most 11 of the 16 entries.

HUD: foreground lists of 0, 1 and 5 records, a triangle the clipper cuts into several pieces (extraCount > 0), a box wholly off screen, and boxes whose four
edges fall on the first or the last pixel of an 8-pixel wave block, each drawn folded into the frame kernel (`fold_foreground = 1`, 8 x 8-pixel waves) and by
raster_draw_kernel (`fold_foreground = 0`, 32 x 2-pixel waves): the same back buffer byte for byte.
"""
import copy

import numpy as np
import pytest

from test_gpu_features import _variant
from test_gpu_raster import _hud_mesh

pytestmark = pytest.mark.gpu

W, H = 96, 64
CACHE_MAX_WORDS, CACHED_STACK = 1536, 16
COUNTERS = ("primaryRays", "shadowRays", "indirectRays", "reflectionRays", "refractionRays", "nodesVisited", "trianglesTested",
            "nodesPrimary", "trianglesPrimary", "nodesDirect", "trianglesDirect", "nodesIndirect", "trianglesIndirect")
# words -> (triangles of the mesh in the sphere's place, triangles of the floor; None: the sample scene as it is; floor 0: no floor instance)
SHAPES = {12: (1, 0), 256: (32, 31), 260: (33, 31), 1292: None, 1536: (300, 83), 1540: (300, 84)}


def _grid_mesh(sample_scene, name, flags, count, origin, du, dv):
    """The first `count` triangles of a regular grid over origin + [0, 1] du + [0, 1] dv, two per cell, front face along du x dv."""
    g = 1
    while 2 * g * g < count:
        g += 1
    o, du, dv = (np.asarray(a, dtype=np.float64) for a in (origin, du, dv))
    n = np.cross(du, dv); n /= np.linalg.norm(n)
    v = np.zeros((g + 1) * (g + 1), dtype=sample_scene.VERTEX_DTYPE)
    for j in range(g + 1):
        for i in range(g + 1):
            k = j * (g + 1) + i
            v["position"][k, :3] = o + du * (i / g) + dv * (j / g); v["position"][k, 3] = 1.0
            v["uv"][k] = (i / g, j / g)
    v["normal"] = n; v["input1"] = 1.0
    idx = []
    for j in range(g):
        for i in range(g):
            a = j * (g + 1) + i; b = a + 1; c = a + g + 1; d = c + 1
            idx += [a, b, c, b, d, c]
    return sample_scene.MeshData(name, flags, v, np.asarray(idx[:3 * count], dtype=np.uint32))


def _shape_scene(sample_data, words):
    from sm64rt_legacy_renderer_amd import sample_scene
    if SHAPES[words] is None:
        return sample_data

    def mod(d):
        wall, floor = SHAPES[words]
        sphere = next(i for i in d.instances if i.name == "sphere"); ground = next(i for i in d.instances if i.name == "floor")
        d.meshes[sphere.mesh] = _grid_mesh(sample_scene, "wall", d.meshes[sphere.mesh].flags, wall, (-2.0, 0.0, 0.0), (4.0, 0.0, 0.0), (0.0, 3.5, 0.0))
        if floor:
            d.meshes[ground.mesh] = _grid_mesh(sample_scene, "floor", d.meshes[ground.mesh].flags, floor, (-1.5, 0.0, -1.0), (0.0, 0.0, 2.0), (2.5, 0.0, 0.0))
        else:
            d.instances = [i for i in d.instances if i is not ground]
    return _variant(sample_data, mod)


def _traced_meshes(data):
    from sm64rt_legacy_renderer_amd import rt64
    return [data.meshes[i.mesh] for i in data.instances if data.meshes[i.mesh].flags & rt64.MESH_RAYTRACE_ENABLED]


def _assert_cache_rule(rt64_lib, data, st, words):
    """The frame's cache image has `words` words, and the host's rule (View::update) enables the cache exactly when that is at most the maximum."""
    meshes = _traced_meshes(data)
    assert st.instanceCount == len(meshes)
    assert 4 * st.instanceCount + (st.tlasNodeBytes + st.blasNodeBytes) // 16 == words
    deepest = 0
    for m in meshes:
        v, i = np.ascontiguousarray(m.vertices), np.ascontiguousarray(m.indices, dtype=np.uint32)
        depth = rt64_lib.MeshTreeDepth(v.ctypes.data, len(v), v.dtype.itemsize, i.ctypes.data, len(i))
        assert depth >= 1
        deepest = max(deepest, depth)
    assert max(len(meshes) - 1, 1) + deepest <= CACHED_STACK          # the depth half of the rule holds for every case: the word count alone decides


def _frame(rt64_lib, data, words, lds_cache, mode):
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    s = sample_scene.Rt64Scene(rt64_lib, data, W, H, hip_device=0)
    try:
        assert s.option("lds_cache", lds_cache) and s.option("count_traversal", 1)
        if mode == "groups":
            assert s.option("max_frame_groups", 4)
        if mode == "gi":
            s.set_view_description(gi_samples=1, denoiser=True)
        for f in range(2 if mode == "gi" else 1):
            s.draw()
        st = s.stats()
        assert st.traversalOverflow == 0
        assert (st.fusedFrame == 1) == (mode != "gi")
        _assert_cache_rule(rt64_lib, data, st, words)
        out = {"final": s.readback(rt64.IMAGE_FINAL_RGBA8).copy(), "counters": {k: int(getattr(st, k)) for k in COUNTERS}}
        if mode == "query":
            ys, xs = np.mgrid[0:H, 0:W]
            rays = sample_scene.camera_rays(data, W, H, np.stack([xs.ravel(), ys.ravel()], axis=1))
            out["hits"] = rt64.trace_rays(rt64_lib, s.view, rays, 0).view(np.uint32).copy()
        return out
    finally:
        s.close()


@pytest.mark.parametrize("mode", ["lean", "groups", "gi", "query"])
@pytest.mark.parametrize("words", sorted(SHAPES))
def test_cached_walk_equals_the_walk_from_memory_at_every_fill_shape(rt64_lib, sample_data, words, mode):
    data = _shape_scene(sample_data, words)
    on, off = _frame(rt64_lib, data, words, 1, mode), _frame(rt64_lib, data, words, 0, mode)
    assert on["counters"] == off["counters"], (on["counters"], off["counters"])
    assert on["counters"]["primaryRays"] == W * H and on["counters"]["nodesVisited"] > 0 and on["counters"]["trianglesTested"] > 0
    assert on["counters"]["shadowRays"] > 0                                    # geometry is on screen and lit
    if mode == "gi":
        assert on["counters"]["indirectRays"] > 0
    assert np.array_equal(on["final"], off["final"])
    if mode == "query":
        assert np.array_equal(on["hits"], off["hits"])
        assert (on["hits"].view(np.int32)[:, 3] >= 0).sum() > W * H // 20 and on["hits"][:, 5].any()


# ---- HUD ----------------------------------------------------------------------------------------------------------------------------------------------------

FULL = [(-1.0, -1.0), (3.0, -1.0), (-1.0, 3.0)]          # covers every pixel: its record's box is the instance's scissor rectangle


def _hud_scene(sample_data, case):
    from sm64rt_legacy_renderer_amd import rt64, sample_scene

    def add(d, mesh, **kw):
        d.meshes.append(mesh)
        i = copy.copy(d.instances[0]); i.mesh = len(d.meshes) - 1; i.material = sample_scene.copy_material(d.instances[0].material); i.name = "hud%d" % len(d.instances)
        for k, v in kw.items():
            setattr(i, k, v)
        d.instances.append(i)

    def mod(d):
        assert d.instances[0].name == "hudB" and d.instances[0].flags == 0          # the sample's one foreground triangle
        if case == "none":
            d.instances = d.instances[1:]
        elif case == "five":
            add(d, _hud_mesh(sample_scene, rt64, [[(-0.9, -0.8), (0.6, -0.6), (-0.2, 0.9)], [(-0.5, -0.9), (0.9, 0.1), (-0.7, 0.5)],
                                                  [(0.1, -0.7), (0.8, 0.8), (-0.6, 0.2)], [(-0.3, -0.3), (0.3, -0.3), (0.0, 0.4)]], alpha=0.6))
        elif case == "clipped":          # a corner behind the eye and one far outside the guard band: several pieces each
            m = _hud_mesh(sample_scene, rt64, [[(0, 0)] * 3] * 2, alpha=0.7)
            for k, p in enumerate([(-0.8, -0.6, 0.2, 1.0), (0.9, -0.7, 0.2, 1.0), (0.1, 0.4, 0.5, -0.5), (-30.0, -0.5, 0.5, 1.0), (0.9, -0.6, 0.5, 1.0), (0.2, 25.0, 0.5, 1.0)]):
                m.vertices["position"][k] = p
            add(d, m)
        elif case == "offscreen":
            add(d, _hud_mesh(sample_scene, rt64, [[(1.5, -0.5), (2.5, -0.5), (2.0, 0.5)]], alpha=0.8))
        elif case == "borders":
            # scissors are (x, y, w, h) from the bottom left; in pixels from the top left the boxes are x 16..47, y 24..47 (each edge a block's first or last pixel,
            # the box made of whole blocks) and x 23..40, y 15..32 (px0 and py0 a block's last pixel, px1 and py1 a block's first)
            add(d, _hud_mesh(sample_scene, rt64, [FULL], alpha=0.6), scissor=(16, H - 24 - 24, 32, 24))
            add(d, _hud_mesh(sample_scene, rt64, [FULL], alpha=0.5), scissor=(23, H - 15 - 18, 18, 18))
        else:
            assert case == "one"
    return _variant(sample_data, mod)


def _hud_final(rt64_lib, data, fold):
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    s = sample_scene.Rt64Scene(rt64_lib, data, W, H, hip_device=0)
    try:
        assert s.option("fold_foreground", fold)
        s.draw()
        assert s.stats().fusedFrame == 1
        return s.readback(rt64.IMAGE_FINAL_RGBA8).copy()
    finally:
        s.close()


@pytest.fixture(scope="module")
def bare_final(rt64_lib, sample_data):
    """The frame without any foreground record."""
    return _hud_final(rt64_lib, _hud_scene(sample_data, "none"), 1)


@pytest.mark.parametrize("case", ["none", "one", "five", "clipped", "offscreen", "borders"])
def test_folded_hud_equals_its_own_launch(rt64_lib, sample_data, bare_final, case):
    data = _hud_scene(sample_data, case)
    folded, drawn = _hud_final(rt64_lib, data, 1), _hud_final(rt64_lib, data, 0)
    assert np.array_equal(folded, drawn)
    touched = (folded != bare_final).any(axis=2)
    if case == "none":
        assert not touched.any()
    else:
        assert touched.any()                                                   # the sample's triangle (and whatever the case adds) is in the picture
    if case == "borders":                                                      # the two scissor boxes, and nothing of the full-screen triangles outside them
        ys, xs = np.nonzero(touched[:, 16:])                                   # (left of x = 16 lies the sample's own triangle)
        assert xs.min() + 16 == 16 and xs.max() + 16 == 47 and ys.min() == 15 and ys.max() == 47
        assert touched[24:48, 16:48].all() and touched[15:33, 23:41].all()
