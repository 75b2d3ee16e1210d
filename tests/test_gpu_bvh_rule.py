"""The BVH builders on the device -- lbvh.hip's single-workgroup and multi-kernel paths, the batch launch, the refit, the TLAS builder -- and the host's
TLAS builder against tests/bvh_rule.py (rules B1-B12), over the case grid of tests/bvh_cases.py: keys, order, every link of every
node (`parent` and `pad` too), the four boxes, the triangle records and the header, bit for bit; a TLAS's leaf boxes within the bound B11 derives.
`leafParent` has no readback: it is held through `parent`, `left` and `right` and through the refit, which reads nothing else of the topology.
The oracle takes no part.  Run with -s for the figures of profiles/bvh_rule_deviation.txt.

The longest case, scattered-524289 (build, refit, three frames, two readbacks of 63 MB and the rule's own tree twice), took 1.5 to 1.7 s on the MI355X box
where it was measured, most of it the rule on the host; the next, equal-131072, 0.8 s; every case of up to 4097 leaves under 0.1 s.  Each is an id of
its own."""
import time

import numpy as np
import pytest

import bvh_cases as BC
import bvh_rule as R
from test_gpu_mesh_fuzz import scene_with_mesh
from test_gpu_parity import _accel

pytestmark = pytest.mark.gpu
W, H = 64, 36


def read_tree(lib, fn, handle, tris=True):
    from sm64rt_legacy_renderer_amd import rt64
    return R.tree_of(_accel(lib, fn, handle, rt64.ACCEL_MORTON, np.uint32), _accel(lib, fn, handle, rt64.ACCEL_SORTED_INDEX, np.uint32),
                     _accel(lib, fn, handle, rt64.ACCEL_NODES, R.NODE_DTYPE), header=_accel(lib, fn, handle, rt64.ACCEL_HEADER, np.uint32),
                     tris=_accel(lib, fn, handle, rt64.ACCEL_TRIANGLES, R.TRI_DTYPE) if tris else None)


def header_depth(n):
    return "rule" if n <= BC.SMALL_MAX else BC.LARGE_DEPTH


def frame(s):
    s.draw()
    st = s.stats()
    assert st.traversalOverflow == 0, st.traversalOverflow
    assert not (s.lib.last_error() and "dropped" in s.lib.last_error()), s.lib.last_error()


@pytest.mark.parametrize("case", BC.CASES, ids=BC.case_id)
def test_the_device_builds_and_refits_the_rules_tree(rt64_lib, sample_data, case):
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    kind, n = case
    t0 = time.perf_counter()
    p, i = BC.mesh(kind, n)
    data = scene_with_mesh(sample_data, p)             # in the sphere's place; indices 0 .. 3n - 1, as bvh_cases.mesh gives them
    full = data.meshes[0]
    full.flags |= rt64.MESH_RAYTRACE_UPDATABLE if n > 1 else 0
    data.meshes[0] = sample_scene.MeshData(full.name, full.flags, full.vertices[:3], full.indices[:3])
    s = sample_scene.Rt64Scene(rt64_lib, data, W, H, hip_device=0)
    try:
        frame(s)                                       # the mesh's first triangle and the floor: two small trees, built together
        s.set_mesh(s.meshes[0], full.vertices, full.indices)
        frame(s)                                       # the mesh alone, another count: built anew by a launch of its own (lbvh_launch; the batch launch has its own test)
        first = R.mesh_tree(p, i)
        bad = R.compare(read_tree(rt64_lib, rt64_lib.ReadbackMeshAccel, s.meshes[0]), first, header_depth(n))
        if n > 1:
            q = BC.moved(kind, n, p)
            s.set_mesh(s.meshes[0], BC.vertices(q), i)
            frame(s)
            bad += R.check_refit(read_tree(rt64_lib, rt64_lib.ReadbackMeshAccel, s.meshes[0]), first, q, i, header_depth(n))
    finally:
        s.close()
    print("bvh_rule gpu %-18s leaves=%-7d depth=%-3d header_depth=%-4s findings=%d refit=%s %.2fs" % (
        BC.case_id(case), n, first["depth"], first["depth"] if n <= BC.SMALL_MAX else BC.LARGE_DEPTH, len(bad), n > 1, time.perf_counter() - t0))
    assert not bad, bad


BATCH = [("skewed", 4096), ("scattered", 1), ("equal", 2), ("clustered", 3), ("collinear", 64), ("far", 65), ("equal", 1024), ("skewed", 1025), ("clustered", 4097),
         ("scattered", 65), ("skewed", 3)]


def test_meshes_built_in_one_batch_are_the_rules_trees(rt64_lib, sample_data):
    """Meshes of different sizes set between two frames: RT64_DrawDevice builds the small ones in ONE launch, one workgroup per tree with blockDim from the
    largest (4096 leaves: 1024 threads), so the one-, two- and three-leaf trees run with far more threads than leaves; the 4097-leaf mesh takes the
    multi-kernel path in the same flush.  The odd ones are UPDATABLE and refitted, again together, before a third frame."""
    import copy
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    d = copy.copy(sample_data)
    d.meshes = list(sample_data.meshes); d.instances = list(sample_data.instances)
    meshes = [BC.mesh(kind, n) for kind, n in BATCH]
    first = len(d.meshes)
    for k, (p, i) in enumerate(meshes):                                        # created with one triangle each; the real meshes come between the frames
        d.meshes.append(sample_scene.MeshData("batch%d" % k, rt64.MESH_RAYTRACE_ENABLED | (rt64.MESH_RAYTRACE_UPDATABLE if k % 2 else 0), BC.vertices(p[:3]), i[:3]))
        inst = copy.copy(sample_data.instances[1]); inst.mesh = first + k; inst.name = "batch%d" % k; inst.material = sample_scene.copy_material(inst.material)
        if BATCH[k][0] == "far":
            t = np.array(inst.transform, dtype=np.float32).copy(); t[3, :3] -= p.mean(axis=0); inst.transform = inst.previous_transform = t
        d.instances.append(inst)
    s = sample_scene.Rt64Scene(rt64_lib, d, W, H, hip_device=0)
    bad = []
    try:
        frame(s)
        for k, (p, i) in enumerate(meshes):
            s.set_mesh(s.meshes[first + k], BC.vertices(p), i)
        frame(s)
        rules = []
        for k, (p, i) in enumerate(meshes):
            rules.append(R.mesh_tree(p, i))
            bad += ["%s-%d: %s" % (BATCH[k] + (b,)) for b in R.compare(read_tree(rt64_lib, rt64_lib.ReadbackMeshAccel, s.meshes[first + k]), rules[k], header_depth(BATCH[k][1]))]
        moved = {k: BC.moved(*BATCH[k], meshes[k][0]) for k in range(1, len(meshes), 2)}
        for k, q in moved.items():
            s.set_mesh(s.meshes[first + k], BC.vertices(q), meshes[k][1])
        frame(s)
        for k, q in moved.items():
            got = read_tree(rt64_lib, rt64_lib.ReadbackMeshAccel, s.meshes[first + k])
            bad += ["%s-%d: %s" % (BATCH[k] + (b,)) for b in R.check_refit(got, rules[k], q, meshes[k][1], header_depth(BATCH[k][1]))]
    finally:
        s.close()
    print("bvh_rule gpu batch of %d meshes (%s) findings=%d" % (len(BATCH), " ".join(BC.case_id(c) for c in BATCH), len(bad)))
    assert not bad, bad


@pytest.mark.parametrize("count", BC.TLAS_SIZES)
def test_both_tlas_builders_build_the_rules_tree(rt64_lib, sample_data, count):
    """Instances of four small meshes under rotations, non-uniform scales, mirrors and far translations (bvh_cases.transforms): the device's builder, and up
    to RT64_HOST_TLAS_MAX = 64 instances the host's, each against the instance form of the rule."""
    from sm64rt_legacy_renderer_amd import sample_scene
    data, transforms, which = BC.tlas_scene(sample_data, count)
    boxes = [R.leaf_boxes(*BC.mesh(kind, n))[:2] for kind, n in BC.TLAS_MESHES]
    lo = np.stack([R.keys(mn, mx)[0] for mn, mx in boxes])[which]; hi = np.stack([R.keys(mn, mx)[1] for mn, mx in boxes])[which]
    s = sample_scene.Rt64Scene(rt64_lib, data, W, H, hip_device=0)
    try:
        for host in (1, 0):
            s.option("host_tlas", host); s.option("always_rebuild", 1)
            frame(s)
            got = read_tree(rt64_lib, rt64_lib.ReadbackViewAccel, s.view, tris=False)
            bad, ratio = R.check_tlas(got, lo, hi, transforms, header_depth(count))
            print("bvh_rule gpu tlas-%-5d %-27s findings=%d largest leaf-box deviation / bound = %.4f" % (
                count, "host_tlas=%d (%s builder)" % (host, "host" if host and count <= 64 else "device"), len(bad), ratio))
            assert not bad, (host, bad)
            assert got["count"] == count
    finally:
        s.close()
