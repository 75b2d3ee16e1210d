"""The scenes the camera rays and texture footprints are checked on (tests/test_footprint_rule.py on the CPU, tests/test_gpu_footprint_query.py on the GPU).
TEST INFRASTRUCTURE.

Each case is a dict: name, data (a SceneData), seed (of its 2000 ray_rule.random_rays and their random differentials), options (device options), screen (the device's
size), view (keywords of Rt64Scene.set_view_description, or None), frames (how many are drawn before the queries), and what the rule needs to know of the frame that
results: render (its render size) and jitter (its pixel jitter).  Frames are 64 x 36 unless the case says otherwise.  Small on purpose, in the manner of
tests/material_cases.py, whose scenes these are."""
import numpy as np

import footprint_rule as R
import material_cases as MC

RAYS = 2000
W, H = 64, 36
UPSCALER_FSR, UPSCALER_MODE_NATIVE = 3, 6
TEXEL1_ONLY = MC.cc((MC.TEX1, MC.S0, MC.IN1, MC.S0), (MC.S0, MC.S0, MC.S0, MC.IN1), MC.OPT_ALPHA)          # reads texel 1 and an input: a UV in the layout, no texel 0


def _lowered(data, eye_y):
    """The sample camera moved down to height eye_y: it looks along the floor."""
    v = np.array(data.view, dtype=np.float32).copy(); v[3, 1] = np.float32(-eye_y)
    data.view = v
    return data


def grazing_floor(sample_data):
    return _lowered(MC.small_sample(sample_data), 1.4)


def grazing_floor_point(sample_data):
    """The same under a POINT sampler: every fetch takes the level (int)(lod + 0.5), and the floor runs through levels 0 to 3."""
    d = grazing_floor(sample_data)
    d.shader_filter = 0
    return d


def other_sizes(sample_data):
    """Normal and specular maps of 32 x 32 under diffuse maps of 64 x 64, uvDetailScale 0.5 on the sphere and 3 on the floor."""
    d = MC.small_sample(sample_data)
    d.instances[3].normal, d.instances[3].specular = 1, 2
    d.instances[1].material.uvDetailScale = 0.5; d.instances[3].material.uvDetailScale = 3.0
    return d


def texel1_only(sample_data):
    """Every instance under a shader that reads texel 1 and never texel 0, normal and specular maps on: F7's quirk."""
    rng = np.random.default_rng(71)
    d = MC.small_sample(sample_data)
    d.shader_id = TEXEL1_ONLY
    d.meshes = [MC.relayout(m, TEXEL1_ONLY, rng) for m in d.meshes]
    return d


def _case(name, data, seed, options=None, screen=(W, H), view=None, frames=1, render=None, jitter=(0.0, 0.0)):
    return dict(name=name, data=data, seed=seed, options=dict(options or {}), screen=screen, view=view, frames=frames, render=render or screen, jitter=jitter)


def cases(sample_data):
    mips = {"generate_mipmaps": 1}
    return [
        _case("sample, generated mips", MC.small_sample(sample_data), 210, mips),
        _case("floor at a grazing angle", grazing_floor(sample_data), 211, mips),
        _case("maps of other sizes, detail scales", other_sizes(sample_data), 212, mips),
        _case("texel 1 only, maps on", texel1_only(sample_data), 213, mips),
        _case("no UV layout", MC.no_uv(sample_data), 214),
        _case("mirrored x = -1", MC.mirrored(sample_data), 215, mips),
        _case("resolutionScale 0.5", MC.small_sample(sample_data), 216, mips, screen=(2 * W, 2 * H), view=dict(resolution_scale=0.5), render=(W, H)),
        _case("upscaler, third frame", MC.small_sample(sample_data), 217, mips, view=dict(upscaler=UPSCALER_FSR, upscaler_mode=UPSCALER_MODE_NATIVE), frames=3,
              jitter=R.upscaler_jitter(2, 8)),          # NATIVE: render size = screen size, 8 (screen / render)^2 = 8 phases
        _case("NPOT textures, LINEAR", MC.sampler_case(sample_data, 1, 0), 218, mips),
        _case("POINT sampler, MIRROR", MC.sampler_case(sample_data, 0, 1), 219, mips),
        _case("floor at a grazing angle, POINT", grazing_floor_point(sample_data), 220, mips),
    ]


NAMES = ["sample, generated mips", "floor at a grazing angle", "maps of other sizes, detail scales", "texel 1 only, maps on", "no UV layout", "mirrored x = -1",
         "resolutionScale 0.5", "upscaler, third frame", "NPOT textures, LINEAR", "POINT sampler, MIRROR", "floor at a grazing angle, POINT"]


def mipmapped(case):
    return bool(case["options"].get("generate_mipmaps", 0))


def camera_of(case):
    return R.camera(case["data"], case["screen"][0], case["screen"][1], case["render"][0], case["render"][1], case["jitter"])


def all_pixels(case):
    w, h = case["render"]
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.uint32)


def random_diffs(seed, rays):
    """One RT64_RAY_DIFFERENTIAL per ray, (N, 16) float32: dDdx, dDdy of 1e-4 .. 3e-2 of the direction's length in random directions; dOdx, dOdy of 1e-3 .. 1e-1 on
    two rays of three and 0 on the third; every 50th differential all zero; the reserved words random bits (F4: ignored)."""
    rng = np.random.default_rng(5000 + seed)
    n = len(rays)
    out = np.zeros((n, 16), dtype=np.float32)
    dlen = np.linalg.norm(rays[:, 4:7].astype(np.float64), axis=1)[:, None]
    for col in (8, 12):
        out[:, col:col + 3] = rng.normal(size=(n, 3)) * dlen * 10.0 ** rng.uniform(-4.0, -1.5, size=(n, 1))
    for col in (0, 4):
        out[:, col:col + 3] = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3.0, -1.0, size=(n, 1))
    out[2::3, 0:3] = 0.0; out[2::3, 4:7] = 0.0
    out[::50] = 0.0
    out.view(np.uint32)[:, [3, 7, 11, 15]] = rng.integers(0, 2 ** 32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    return out
