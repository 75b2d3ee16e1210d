"""GPU parity tests: HIP render path (through the C ABI) vs the CPU oracle on the reference's sample scene.

Bars: geometry (hit records: t, u, v, instance, primitive; BVH nodes; Morton order) is BIT-EXACT;
shading is compared within tolerances written next to each assert (libm vs device transcendental functions).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene_256(rt64_lib, sample_data):
    from sm64rt_legacy_renderer_amd import sample_scene
    s = sample_scene.Rt64Scene(rt64_lib, sample_data, 256, 256, hip_device=0)
    s.option("count_traversal", 1)
    s.draw()
    yield s
    s.close()


@pytest.fixture(scope="module")
def oracle_256(sample_data, oracle_lib):
    from oracle import oracle_py
    o = oracle_py.OracleScene(sample_data)
    r = o.render(256, 256)
    yield o, r
    o.close()


def test_c1_primary_visibility_bit_exact(scene_256, oracle_256):
    """BASELINE config C1: 256x256 primary visibility.  t/u/v bits, instance and primitive ids must be identical."""
    from sm64rt_legacy_renderer_amd import rt64
    _, ref = oracle_256
    hit = scene_256.readback(rt64.IMAGE_PRIMARY_HIT)
    assert hit.shape == ref["primaryHit"].shape
    mism = np.any(hit != ref["primaryHit"], axis=-1)
    assert mism.sum() == 0, f"{mism.sum()} pixels differ, first at {np.argwhere(mism)[:5]}"
    ids = scene_256.readback(rt64.IMAGE_INSTANCE_ID)
    assert np.array_equal(ids, ref["instanceId"])
    # coverage probed by brute force in SURVEY 8 (43.7 % at 16:9); at 1:1 just require both instances visible
    assert (ids == 0).any() and (ids == 1).any() and (ids == -1).any()


def test_traversal_counters_match_oracle(scene_256, oracle_256):
    """Same BVH + same traversal order => identical node / triangle visit counts (they define the algorithmic bytes)."""
    _, ref = oracle_256
    st = scene_256.stats()
    c = ref["counters"]
    assert st.primaryRays == c["primaryRays"] == 256 * 256
    assert st.shadowRays == c["shadowRays"]
    assert st.nodesVisited == c["nodesVisited"]
    assert st.trianglesTested == c["trianglesTested"]


def test_gbuffer_parity(scene_256, oracle_256):
    """The G-buffer of the sample scene against the oracle's.  Its flow line is on a STATIC frame (still camera, previousTransform = transform), where every value is 0
    or near it, and its depth line on that one frame: flow with a moving camera, moving instances, a jittered frame and a canReproject = false frame, depth, the masks
    and the loop's bookkeeping are held pixel by pixel to the float64 rule of tests/primary_rule.py in tests/test_gpu_primary_rule.py."""
    from sm64rt_legacy_renderer_amd import rt64
    _, ref = oracle_256
    pos = scene_256.readback(rt64.IMAGE_SHADING_POSITION)
    # shading position = origin + dir * t with identical t: exact
    assert np.array_equal(pos, ref["shadingPosition"])
    depth = scene_256.readback(rt64.IMAGE_DEPTH)
    assert np.allclose(depth, ref["depth"], rtol=0, atol=1e-6)
    # normals / specular are RGBA16F, diffuse RGBA8: allow one quantisation step on a tiny fraction of pixels
    # (device log2f/sqrt chains vs libm flip a rounding here and there)
    for image, key, step in ((rt64.IMAGE_SHADING_NORMAL, "shadingNormal", 2e-3), (rt64.IMAGE_SHADING_SPECULAR, "shadingSpecular", 2e-3),
                             (rt64.IMAGE_DIFFUSE, "diffuse", 1.0 / 255.0 + 1e-6)):
        a = scene_256.readback(image)
        d = np.abs(a - ref[key])
        assert d.max() <= step, (key, float(d.max()))
        assert (d > 0).mean() < 0.01, (key, float((d > 0).mean()))
    vd = scene_256.readback(rt64.IMAGE_VIEW_DIRECTION)
    assert np.array_equal(vd, ref["viewDirection"])
    flow = scene_256.readback(rt64.IMAGE_FLOW)
    assert np.allclose(flow, ref["flow"], atol=1e-3)


def test_c2_full_frame_rmse(rt64_lib, sample_data, oracle_lib):
    """BASELINE config C2 at reduced size (480x270, 16:9): primary + shadow rays, direct light, compose, post.
    Gate from BASELINE.json: per-pixel fp32 RMSE <= 1e-3 on the composed RGBA32F output."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    from oracle import oracle_py
    W, H = 480, 270
    s = sample_scene.Rt64Scene(rt64_lib, sample_data, W, H, hip_device=0)
    try:
        s.draw()
        out = s.readback(rt64.IMAGE_OUTPUT_RGBA32F)
        final = s.readback(rt64.IMAGE_FINAL_RGBA8)
        direct = s.readback(rt64.IMAGE_DIRECT_LIGHT_RAW)
        indirect = s.readback(rt64.IMAGE_INDIRECT_LIGHT_RAW)
    finally:
        s.close()
    o = oracle_py.OracleScene(sample_data)
    try:
        ref = o.render(W, H)
    finally:
        o.close()
    rmse = float(np.sqrt(np.mean((out[..., :3].astype(np.float64) - ref["output"][..., :3]) ** 2)))
    assert rmse <= 1e-3, rmse
    rmse8 = float(np.sqrt(np.mean(((final[..., :3].astype(np.float64) - ref["final"][..., :3]) / 255.0) ** 2)))
    assert rmse8 <= 1e-3, rmse8
    assert np.abs(final.astype(np.int32) - ref["final"].astype(np.int32)).max() <= 1
    assert np.abs(direct - ref["directLight"]).max() <= 4e-3          # RGBA16F steps near 1.0 are 9.8e-4
    assert np.array_equal(indirect, ref["indirectLight"])              # constant ambient (giSamples = 0)
    # the frame is not trivially black / constant
    assert final[..., :3].std() > 20


def _accel(lib, fn, handle, what, dtype):
    n = fn(handle, what, None, 0)
    assert n > 0, lib.last_error()
    buf = np.empty(n, dtype=np.uint8)
    assert fn(handle, what, buf.ctypes.data, n) == n
    return buf.view(dtype)


def test_blas_tlas_bit_exact(scene_256, oracle_256):
    """LBVH built on the GPU (LDS sort + Karras + fit) == CPU oracle LBVH: same Morton order, same nodes, same leaves."""
    from sm64rt_legacy_renderer_amd import rt64
    from oracle import oracle_py
    o, _ = oracle_256
    lib = scene_256.lib
    for mesh_index in (0, 3):                                     # sphere (320 triangles), floor (2)
        ref = o.mesh_bvh(mesh_index)
        h = scene_256.meshes[mesh_index]
        assert np.array_equal(_accel(lib, lib.ReadbackMeshAccel, h, rt64.ACCEL_MORTON, np.uint32), ref["morton"])
        assert np.array_equal(_accel(lib, lib.ReadbackMeshAccel, h, rt64.ACCEL_SORTED_INDEX, np.uint32), ref["sortedIndex"])
        nodes = _accel(lib, lib.ReadbackMeshAccel, h, rt64.ACCEL_NODES, oracle_py.NODE_DTYPE)
        for f in ("lmin", "lmax", "rmin", "rmax", "left", "right", "pad"):
            assert np.array_equal(nodes[f], ref["nodes"][f]), (mesh_index, f)
        assert np.array_equal(nodes["parent"][1:], ref["nodes"]["parent"][1:])
        tris = _accel(lib, lib.ReadbackMeshAccel, h, rt64.ACCEL_TRIANGLES, oracle_py.TRI_DTYPE)
        rt = o.mesh_tris(mesh_index)
        for f in ("v0", "v1", "v2", "prim"):
            assert np.array_equal(tris[f], rt[f])
        hdr = _accel(lib, lib.ReadbackMeshAccel, h, rt64.ACCEL_HEADER, np.float32)
        assert np.array_equal(hdr[0:3], ref["bmin"]) and np.array_equal(hdr[4:7], ref["bmax"])
    tl = o.tlas()
    assert np.array_equal(_accel(lib, lib.ReadbackViewAccel, scene_256.view, rt64.ACCEL_SORTED_INDEX, np.uint32), tl["sortedIndex"])
    nodes = _accel(lib, lib.ReadbackViewAccel, scene_256.view, rt64.ACCEL_NODES, oracle_py.NODE_DTYPE)
    for f in ("lmin", "lmax", "rmin", "rmax", "left", "right"):
        assert np.array_equal(nodes[f], tl["nodes"][f]), f


@pytest.mark.parametrize("extra", [0, 1, 37, 62, 80])
def test_tlas_host_and_gpu_builders_agree(rt64_lib, oracle_lib, extra):
    """The TLAS of a few instances is built on the host and uploaded with the frame tables (rt64_host.cpp host_build_tlas); above
    RT64_HOST_TLAS_MAX = 64 the GPU builder runs.  Both must give the oracle's tree bit for bit (Geometry spec G1-G6), and the frames
    rendered through either must be identical.  `extra` rotated / scaled / translated copies of the sphere are added to the sample scene
    (2 + 62 = the last host-built size; 0 with the floor removed = the single-leaf tree)."""
    import copy
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    from oracle import oracle_py
    data = sample_scene.make_sample_scene()
    rng = np.random.default_rng(1234 + extra)
    sphere = next(i for i in data.instances if i.name == "sphere")
    if extra == 0:
        data.instances = [i for i in data.instances if i.name != "floor"]
    for k in range(extra):
        a, b = rng.uniform(0, 2 * np.pi, 2)
        ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
        rot = np.array([[ca, sa, 0, 0], [-sa, ca, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]) @ np.array([[1, 0, 0, 0], [0, cb, sb, 0], [0, -sb, cb, 0], [0, 0, 0, 1]])
        m = np.diag(list(rng.uniform(0.1, 0.6, 3)) + [1.0]) @ rot
        m[3, :3] = rng.uniform(-6, 6, 3) * (1.0, 0.3, 1.0) + (0.0, 2.0, 0.0)
        t = m.astype(np.float32)
        if k % 7 == 3:
            t = data.instances[-1].transform.copy()                        # the same box again: equal Morton codes, ordered by instance index (G3)
        data.instances.append(sample_scene.InstanceData("copy%d" % k, sphere.mesh, t, t, sphere.diffuse, sphere.normal, sphere.specular, sample_scene.copy_material(sphere.material), 0))
    o = oracle_py.OracleScene(data)
    ref = o.render(160, 90)                                                # builds the oracle's TLAS
    tl = o.tlas()
    s = sample_scene.Rt64Scene(rt64_lib, data, 160, 90, hip_device=0)
    try:
        got = {}
        for host in (1, 0):
            s.option("host_tlas", host); s.option("always_rebuild", 1)
            s.draw()
            got[host] = dict(index=_accel(rt64_lib, rt64_lib.ReadbackViewAccel, s.view, rt64.ACCEL_SORTED_INDEX, np.uint32).copy(),
                             morton=_accel(rt64_lib, rt64_lib.ReadbackViewAccel, s.view, rt64.ACCEL_MORTON, np.uint32).copy(),
                             nodes=_accel(rt64_lib, rt64_lib.ReadbackViewAccel, s.view, rt64.ACCEL_NODES, oracle_py.NODE_DTYPE).copy(),
                             header=_accel(rt64_lib, rt64_lib.ReadbackViewAccel, s.view, rt64.ACCEL_HEADER, np.uint32).copy(),
                             frame=s.readback(rt64.IMAGE_FINAL_RGBA8).copy(), hit=s.readback(rt64.IMAGE_PRIMARY_HIT).copy())
        assert np.array_equal(got[1]["hit"], ref["primaryHit"])              # many-instance traversal (TLAS stack, LDS cache off above 16 instances)
        for host in (1, 0):
            g = got[host]
            assert np.array_equal(g["index"], tl["sortedIndex"]), host
            assert np.array_equal(g["morton"], tl["morton"]), host
            for f in ("lmin", "lmax", "rmin", "rmax", "left", "right", "pad"):
                assert np.array_equal(g["nodes"][f].view(np.uint32), tl["nodes"][f].view(np.uint32)), (host, f)
        assert np.array_equal(got[0]["nodes"]["parent"][1:], got[1]["nodes"]["parent"][1:])
        assert np.array_equal(got[0]["header"][[0, 1, 2, 3, 4, 5, 6]], got[1]["header"][[0, 1, 2, 3, 4, 5, 6]])      # bounds + count
        if len(tl["sortedIndex"]) <= 64:
            assert got[0]["header"][7] == got[1]["header"][7]                                                        # tree depth (single-workgroup builder)
        assert np.array_equal(got[0]["frame"], got[1]["frame"]) and np.array_equal(got[0]["hit"], got[1]["hit"])
    finally:
        s.close(); o.close()


@pytest.mark.parametrize("subdiv,grid", [(2, 1), (3, 64), (5, 1)])
def test_large_meshes_bit_exact(rt64_lib, oracle_lib, subdiv, grid):
    """Stress variant of the sample scene: 5 120 / 20 480-triangle spheres (multi-block radix path above 4096
    leaves), 8 192-triangle floor; and a 327 680-triangle sphere -- above 131 072 leaves the bottom-up box fit of the large-tree builder
    takes two group levels (lg_fit_group_kernel, lbvh.hip) and its 37 MB of nodes and triangles no longer sit in one XCD's L2, so the
    one-step-per-trip walk (trace_ray_stepwise) fetches from the Infinity Cache / HBM.  BLAS arrays, the rendered hit records and the
    visit counters must still equal the oracle's bit for bit."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    from oracle import oracle_py
    data = sample_scene.make_sample_scene(subdiv=subdiv, floor_grid=grid)
    s = sample_scene.Rt64Scene(rt64_lib, data, 320, 180, hip_device=0)
    o = oracle_py.OracleScene(data)
    try:
        s.option("count_traversal", 1)
        s.draw()
        ref = o.render(320, 180)
        for mesh_index in (0, 3):
            rb = o.mesh_bvh(mesh_index)
            h = s.meshes[mesh_index]
            assert np.array_equal(_accel(rt64_lib, rt64_lib.ReadbackMeshAccel, h, rt64.ACCEL_MORTON, np.uint32), rb["morton"])
            assert np.array_equal(_accel(rt64_lib, rt64_lib.ReadbackMeshAccel, h, rt64.ACCEL_SORTED_INDEX, np.uint32), rb["sortedIndex"])
            nodes = _accel(rt64_lib, rt64_lib.ReadbackMeshAccel, h, rt64.ACCEL_NODES, oracle_py.NODE_DTYPE)
            for f in ("lmin", "lmax", "rmin", "rmax", "left", "right"):
                assert np.array_equal(nodes[f], rb["nodes"][f]), (mesh_index, f)
        assert np.array_equal(s.readback(rt64.IMAGE_PRIMARY_HIT), ref["primaryHit"])
        st = s.stats()
        assert st.nodesVisited == ref["counters"]["nodesVisited"] and st.trianglesTested == ref["counters"]["trianglesTested"]
        out = s.readback(rt64.IMAGE_OUTPUT_RGBA32F)
        assert float(np.sqrt(np.mean((out[..., :3].astype(np.float64) - ref["output"][..., :3]) ** 2))) <= 1e-3
    finally:
        s.close(); o.close()


@pytest.mark.parametrize("subdiv,grid", [(6, 256), (7, 256)])
def test_stress_scene_at_1080p_against_the_oracle(rt64_lib, oracle_lib, subdiv, grid):
    """The stress variant SURVEY 8(d) defines (sphere subdivided to >= 1.3 M triangles + a tessellated floor: a BVH that leaves every cache) and the one
    bench.py measures (--subdiv 7 --floor-grid 256: 5.4 M triangles, 344 MB of nodes), at 1920 x 1080: the large-tree builder (radix sort over 5.2 M keys, three
    levels of box fit), the one-wave form of the frame kernel with its cost-ordered tiles and the walk from HBM.  Hit records of all 2 M pixels and the visit
    counters of all 3 M rays equal the oracle's; three frames, so that the second and third start their tiles in the recorded cost order."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    from oracle import oracle_py
    data = sample_scene.make_sample_scene(subdiv=subdiv, floor_grid=grid)
    s = sample_scene.Rt64Scene(rt64_lib, data, 1920, 1080, hip_device=0)
    o = oracle_py.OracleScene(data)
    try:
        s.option("count_traversal", 1)
        for _ in range(3):
            s.draw()
        st = s.stats()
        assert st.fusedFrame == 1 and st.traversalOverflow == 0
        ref = o.render(1920, 1080)
        assert np.array_equal(s.readback(rt64.IMAGE_PRIMARY_HIT), ref["primaryHit"])
        c = ref["counters"]
        assert (st.primaryRays, st.shadowRays) == (c["primaryRays"], c["shadowRays"])
        assert st.nodesVisited == c["nodesVisited"] and st.trianglesTested == c["trianglesTested"]
        assert st.nodesPrimary == c["nodesVisitedPrimary"] and st.nodesDirect == c["nodesVisitedShadow"]
        out = s.readback(rt64.IMAGE_OUTPUT_RGBA32F)
        assert float(np.sqrt(np.mean((out[..., :3].astype(np.float64) - ref["output"][..., :3]) ** 2))) <= 1e-3
        d = np.abs(s.readback(rt64.IMAGE_FINAL_RGBA8).astype(np.int32) - ref["final"].astype(np.int32))
        assert d.max() <= 1
    finally:
        s.close(); o.close()


def test_picking_returns_instance_pointer(scene_256):
    lib = scene_256.lib
    centre = lib.GetViewRaytracedInstanceAt(scene_256.view, 128, 150)
    assert centre == scene_256.instances[1]          # the sphere instance handle (scene order: hudB, sphere, hudA, floor)
    floor = lib.GetViewRaytracedInstanceAt(scene_256.view, 20, 250)
    assert floor == scene_256.instances[3]
    sky = lib.GetViewRaytracedInstanceAt(scene_256.view, 10, 10)
    assert not sky
    assert not lib.GetViewRaytracedInstanceAt(scene_256.view, -5, 1000)


def test_error_convention(rt64_lib):
    """NULL + RT64_GetLastError() instead of exceptions across the C boundary (rt64_common.h:379-383)."""
    from sm64rt_legacy_renderer_amd import rt64
    dev = rt64_lib.CreateDeviceHeadless(64, 64, 0)
    assert dev
    d = rt64.TEXTURE_DESC()
    junk = (C.c_uint8 * 64)()
    d.bytes = C.addressof(junk); d.byteCount = 64; d.format = rt64.TEXTURE_FORMAT_DDS; d.width = d.height = d.rowPitch = -1
    assert not rt64_lib.CreateTexture(dev, d)
    assert "DDS" in rt64_lib.last_error()
    assert not rt64_lib.CreateDeviceHeadless(64, 64, 4096)
    assert "out of range" in rt64_lib.last_error()
    rt64_lib.DestroyDevice(dev)
