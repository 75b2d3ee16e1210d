"""The case grid of the BVH rule (tests/bvh_rule.py, DESIGN.md section 4 "The BVH builders against an independent rule"): deterministic meshes,
every size the smallest shape on either side of a switch in csrc/lbvh.hip.  TEST INFRASTRUCTURE: the meshes and transforms are numpy only, the scene
helpers at the end put them into the sample scene's description.

Kinds
  scattered   centres uniform in a 4-unit cube, edges shrinking with the count
  equal       every triangle's box has the same centre (0, 1.5, 0) and its own extents, all exact in float32: all keys are equal, the tree is decided
              by the leaf number alone, ranges cut purely by index bits, and yet no two boxes are the same
  clustered   a handful of centres with offsets far below a key cell: runs of equal keys among distinct ones
  collinear   every vertex on one line: two axes without extent (scale 0)
  far         offsets of 1e-3 at coordinates of a few thousand
  skewed      box centres on a staircase along the diagonal, in the cell just below 2^-k of the extent on every axis, so that leaf m (= leaf mod 30)
              has the key 2^(m+1) - 1: every split peels one key off, a chain of 30 key levels, deeper with the duplicates of m (index bits).  It
              holds depth, pad and parent on a lopsided tree and stays far inside the traversal stack the host sizes (a radix tree over these keys
              is at most 62 deep, and the stack holds any such tree); no case is meant to approach an overflow.
No position is -0, NaN or infinite.

Sizes                 switch in lbvh.hip
  1, 2, 3             smallest trees
  64, 65              the launch rounds threads to whole waves
  1024, 1025          rank-by-counting <-> 1-bit LDS radix; items per thread 1 <-> 2
  4096, 4097          one workgroup in LDS <-> the multi-kernel path; 4097 is three sort tiles, the last with one key, and three fit chunks
  131072, 131073      64 chunks, one group level <-> 65 chunks, two levels of lg_fit_group_kernel
  524289              257 sort tiles: the second turn of lg_scan_rows_kernel's carry loop
Three group levels need more than 64 * 64 * 2048 = 8.3 M leaves: out of scope.  Every kind at every size up to 4097; scattered and equal at 131072 and
131073; scattered alone at 524289.  Every size above 1 also runs a refit (moved())."""
import zlib

import numpy as np

KINDS = ("scattered", "equal", "clustered", "collinear", "far", "skewed")
SMALL_SIZES = (1, 2, 3, 64, 65, 1024, 1025, 4096, 4097)
CASES = ([(k, n) for n in SMALL_SIZES for k in KINDS] + [(k, n) for n in (131072, 131073) for k in ("scattered", "equal")] + [("scattered", 524289)])
SMALL_MAX = 4096                       # LBVH_SMALL_MAX: up to here one workgroup builds the tree and the header holds its depth; above, 255
LARGE_DEPTH = 255


def case_id(case):
    return "%s-%d" % case


def _rng(kind, n, salt=0):
    return np.random.default_rng([zlib.crc32(kind.encode()), n, salt])


def mesh(kind, n):
    """-> (positions [3n, 3] float32, indices [3n] uint32).  Triangle p has the corners 3p, 3p + 1, 3p + 2."""
    f32 = np.float32
    rng = _rng(kind, n)
    up = np.array([0.0, 1.5, 0.0], dtype=f32)
    e = rng.uniform(-0.3, 0.3, size=(n, 3, 3)).astype(f32) * f32(min(1.0, (64.0 / n) ** (1.0 / 3.0)))
    if kind == "scattered":
        p = rng.uniform(-2.0, 2.0, size=(n, 1, 3)).astype(f32) + up + e
    elif kind == "equal":
        r = (1 + rng.integers(0, 4093, size=(n, 3))).astype(f32) * f32(2.0 ** -12)           # half extents, multiples of 2^-12 below 1: up +- r is exact
        third = up + r * rng.uniform(-0.9, 0.9, size=(n, 3)).astype(f32)                         # a corner inside the box
        p = np.stack([up - r, up + r, third], axis=1)
    elif kind == "clustered":
        centres = rng.uniform(-2.0, 2.0, size=(max(1, n // 50 + 1), 3)).astype(f32) + up
        p = centres[rng.integers(0, len(centres), size=n)][:, None, :] + e * f32(1e-4)
    elif kind == "collinear":
        t = rng.uniform(-2.0, 2.0, size=(n, 3, 1)).astype(f32)
        p = np.array([0.0, 1.0, 0.0], dtype=f32) + t * np.array([1.0, 0.0, 0.0], dtype=f32)
    elif kind == "far":
        p = (rng.uniform(-2.0, 2.0, size=(n, 1, 3)).astype(f32) + up + e) * f32(1e-3) + np.array([4096.0, 2048.0, -8192.0], dtype=f32)
    elif kind == "skewed":
        m = np.arange(n) % 30
        j = np.stack([(m + 3) // 3, (m + 2) // 3, (m + 1) // 3], axis=1)                          # bits of x, y, z among the code's bits 0 .. m
        c = ((2.0 ** j - 0.5) * 2.0 ** -8).astype(f32)                                           # cell 2^j - 1 of 1024 over an extent of 4, at its middle
        r = (1 + rng.integers(0, 3, size=(n, 3))).astype(f32) * f32(2.0 ** -11)                  # box = c +- r inside the cell: exact, so the centre is c
        third = c + r * rng.uniform(-0.9, 0.9, size=(n, 3)).astype(f32)
        p = np.stack([c - r, c + r, third], axis=1)
        p[0, 0] = 0.0; p[0, 1] = 4.0                                                             # leaf 0 spans the whole extent [0, 4]^3
        p = p + np.array([-2.0, 0.0, -2.0], dtype=f32)
    else:
        raise ValueError(kind)
    p = np.ascontiguousarray(p.reshape(-1, 3), dtype=f32) + f32(0.0)                             # (-0 + 0 = +0)
    return p, np.arange(len(p), dtype=np.uint32)


def moved(kind, n, positions):
    """The vertices of the refit: every one moved, far enough to change most keys had the builder re-sorted."""
    rng = _rng(kind, n, 1)
    d = rng.uniform(-0.4, 0.4, size=positions.shape).astype(np.float32) * np.float32(1e-3 if kind == "far" else 1.0)
    if kind == "collinear":
        d[:, 1:] = 0.0
    return np.ascontiguousarray(positions + d, dtype=np.float32) + np.float32(0.0)


# ---- TLAS: instances of small meshes -----------------------------------------------------------------------------------------------------------
TLAS_SIZES = (1, 2, 64, 65, 1025, 4097)  # one leaf; the smallest tree; RT64_HOST_TLAS_MAX = 64, the last size the host builds <-> the first only the device builds; counting <-> radix; the multi-kernel path


def transforms(count):
    """[count, 4, 4] float32, row vectors (translation in row 3): rotations, non-uniform scales, every fifth a mirror (negative determinant), every
    seventh far away, every eleventh the transform before it again (equal keys, ordered by the instance number)."""
    rng = _rng("tlas", count)
    out = np.zeros((count, 4, 4), dtype=np.float64)
    a, b = rng.uniform(0, 2 * np.pi, size=(2, count))
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    rz = np.zeros((count, 3, 3)); rz[:, 0, 0] = ca; rz[:, 0, 1] = sa; rz[:, 1, 0] = -sa; rz[:, 1, 1] = ca; rz[:, 2, 2] = 1
    rx = np.zeros((count, 3, 3)); rx[:, 0, 0] = 1; rx[:, 1, 1] = cb; rx[:, 1, 2] = sb; rx[:, 2, 1] = -sb; rx[:, 2, 2] = cb
    scale = rng.uniform(0.05, 0.4, size=(count, 3))
    k = np.arange(count)
    scale[k % 5 == 2, 0] *= -1.0
    out[:, :3, :3] = scale[:, :, None] * (rz @ rx)
    out[:, 3, :3] = rng.uniform(-6, 6, size=(count, 3)) * (1.0, 0.3, 1.0) + (0.0, 2.0, 0.0)
    out[k % 7 == 3, 3, :3] += (3000.0, -1500.0, 6000.0)
    out[:, 3, 3] = 1.0
    out = out.astype(np.float32)
    again = np.flatnonzero((k % 11 == 5) & (k > 0))
    out[again] = out[again - 1]
    assert count < 3 or (np.linalg.det(out[:, :3, :3].astype(np.float64)) < 0).any()
    return out


TLAS_MESHES = (("scattered", 64), ("skewed", 65), ("collinear", 3), ("equal", 2))               # the instances' meshes, in turn


def vertices(positions):
    """Vertex records around the positions, as test_gpu_mesh_fuzz.scene_with_mesh makes them."""
    from sm64rt_legacy_renderer_amd import sample_scene
    v = np.zeros(len(positions), dtype=sample_scene.VERTEX_DTYPE)
    v["position"][:, :3] = positions; v["position"][:, 3] = 1.0
    v["normal"] = (0.0, 1.0, 0.0); v["uv"] = positions[:, :2] * np.float32(0.25); v["input1"] = (1.0, 1.0, 1.0, 1.0)
    return v


def tlas_scene(sample_data, count):
    """-> (scene data of `count` ray-traced instances and nothing else, their transforms, the mesh number of each)"""
    import copy
    from sm64rt_legacy_renderer_amd import sample_scene
    d = copy.copy(sample_data)
    d.meshes = []
    for kind, n in TLAS_MESHES:
        p, i = mesh(kind, n)
        d.meshes.append(sample_scene.MeshData("%s-%d" % (kind, n), sample_data.meshes[0].flags, vertices(p), i))
    sphere = next(i for i in sample_data.instances if i.name == "sphere")
    t = transforms(count); which = np.arange(count) % len(TLAS_MESHES)
    d.instances = [sample_scene.InstanceData("i%d" % k, int(which[k]), t[k], t[k], sphere.diffuse, sphere.normal, sphere.specular, sample_scene.copy_material(sphere.material), 0)
                   for k in range(count)]
    return d, t, which
