"""The scenes the surface records are checked on (tests/test_surface_rule.py on the CPU, tests/test_gpu_surface_query.py on the GPU).  TEST INFRASTRUCTURE.

Each case is (name, scene data, ray seed, device options).  The rays are ray_rule.random_rays of the scene, 2000 per case."""
import copy
import math

import numpy as np

RAYS = 2000
NO_UV_SHADER = 0x00200200          # colour = alpha = vertex input 1, no texture: float4 position, float3 normal, float3 input = 40 bytes, no UV
NO_UV_DTYPE = np.dtype([("position", "<f4", 4), ("normal", "<f4", 3), ("input1", "<f4", 3)])


def _copy_scene(data):
    d = copy.copy(data)
    d.instances = [copy.copy(i) for i in data.instances]
    d.meshes = [copy.copy(m) for m in data.meshes]
    return d


def _with_sphere_transform(data, m3):
    d = _copy_scene(data)
    t = np.array(d.instances[1].transform, dtype=np.float32).copy()
    t[:3, :3] = (np.asarray(m3, dtype=np.float64) @ t[:3, :3].astype(np.float64)).astype(np.float32)
    d.instances[1].transform = t; d.instances[1].previous_transform = t
    return d


def rotated_scaled(data):
    """The sphere under rotation x scale (1, 0.5, 2): the inverse transpose is not the transform."""
    a, b = 0.7, -0.4
    ry = np.array([[math.cos(a), 0, -math.sin(a)], [0, 1, 0], [math.sin(a), 0, math.cos(a)]])
    rx = np.array([[1, 0, 0], [0, math.cos(b), math.sin(b)], [0, -math.sin(b), math.cos(b)]])
    return _with_sphere_transform(data, np.diag([1.0, 0.5, 2.0]) @ ry @ rx)


def mirrored(data):
    """The sphere mirrored in x (negative determinant: the winding the ray sees is flipped)."""
    return _with_sphere_transform(data, np.diag([-1.0, 1.0, 1.0]))


def zero_normals(data):
    """The sphere's vertex normals all zero: A7's fallback to the triangle normal."""
    d = _copy_scene(data)
    v = d.meshes[d.instances[1].mesh].vertices.copy()
    v["normal"] = 0.0
    d.meshes[d.instances[1].mesh].vertices = v
    return d


def no_uv(data):
    """A shader that reads no texture: every mesh repacked to the 40-byte layout without UVs."""
    d = _copy_scene(data)
    d.shader_id = NO_UV_SHADER
    for m in d.meshes:
        v = np.zeros(len(m.vertices), dtype=NO_UV_DTYPE)
        v["position"] = m.vertices["position"]; v["normal"] = m.vertices["normal"]; v["input1"] = m.vertices["input1"][:, :3]
        m.vertices = v
    return d


def cases(sample_data, with_random=True):
    from sm64rt_legacy_renderer_amd import sample_scene
    out = [("sample lds_cache=1", sample_data, 10, {"lds_cache": 1}),
           ("sample lds_cache=0", sample_data, 11, {"lds_cache": 0}),
           ("sphere 5120 triangles", sample_scene.make_sample_scene(subdiv=2), 10, {})]
    if with_random:
        from test_gpu_fuzz import random_scene
        for seed in (3, 6):
            out.append(("random scene %d" % seed, random_scene(sample_data, seed)[0], 100 + seed, {"lds_cache": seed % 2}))
    out += [("rotation x scale (1, .5, 2)", rotated_scaled(sample_data), 12, {}),
            ("mirrored x = -1", mirrored(sample_data), 13, {}),
            ("zero vertex normals", zero_normals(sample_data), 14, {}),
            ("no UV layout", no_uv(sample_data), 15, {})]
    return out
