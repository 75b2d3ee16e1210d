"""The scenes the sampled direct-light records are checked on (tests/test_sampled_lighting_rule.py on the CPU, tests/test_gpu_sampled_lighting_query.py on the
GPU).  TEST INFRASTRUCTURE.

Each case is light_cases.make_case's scene of that name on material_cases.small_sample with its view description (maxLights, diSamples) and the number of frames
drawn before the query, at light_cases' 88 x 72.  One is added: "noise", a quad between the first near light and the floor whose shader is the scene's with the
noise option and shadowAlphaMultiplier 2 -- its shadow alpha clamps to exactly 1 before J8's factor, so a key either sees it as an opaque caster or not at all.

The records are the camera rays of every pixel of every second row (3168 of them, somewhat under half of which hit) plus 120 of ray_rule.random_rays.  The random
rays are few on purpose: on the far side of the sphere a candidate's intensity falls to the size of the error the unquantised normal's bound gives the others
(material_rule: about 1e-5 relative), and once the brighter candidates are drawn no float64 rule can say how the rest of the walk goes -- whatever the key is; a
case that draws all its candidates leaves about one such hit in six undecided there, against one in seventy among the camera's.  Keys: the camera rays' first half is
keyed by its pixel and the case's first frame value, the second half by the pixel moved off the frame by multiples of 64 (the noise tile repeats; the seed of J8
does not) at the second frame value; the random rays take random x, y below 4096 and the frame values in turn.  Every case has a frame value whose draws or
samples cross a multiple of 64.
"""
import numpy as np

import light_cases as LC
import material_cases as MC
import material_rule as M
import ray_rule

W, H = LC.W, LC.H
NAMES = ("four", "pick-one", "twenty", "falloff", "radius-1", "radius-4", "material", "noise")
SEEDS = {name: 501 + k for k, name in enumerate(NAMES)}
RANDOM_RAYS = 120

# key.frame values per case: the frame the case draws, one whose draws or samples cross slice 63 -> 0, and two more; "twenty" keeps light_cases' 9.  On these
# records the undecided share does not move with the frame value (every slice holds the byte 255 sixteen times); tests/test_sampled_lighting_rule.py asserts that
# the rule's own evaluation stays under the cap for the keys chosen here.
FRAMES = {"four": (0, 62, 5, 200), "pick-one": (0, 63, 7, 129), "twenty": (9, 57, 73, 201), "falloff": (0, 63, 18, 130), "radius-1": (0, 63, 3, 190),
          "radius-4": (0, 61, 11, 4294967295), "material": (0, 62, 6, 77), "noise": (0, 63, 4, 131)}

# What makes a case worth running, as shares of its real hits measured on the rule: at least this much in shadow, with more than one light drawn, with a noise
# factor of 0.  Well under what the geometry gives, above what a broken case would show.
SHARES = {"four": (0.10, 0.90, 0.0), "pick-one": (0.01, 0.0, 0.0), "twenty": (0.20, 0.90, 0.0), "falloff": (0.02, 0.50, 0.0), "radius-1": (0.05, 0.90, 0.0),
          "radius-4": (0.05, 0.90, 0.0), "material": (0.10, 0.90, 0.0), "noise": (0.05, 0.90, 0.30)}
UNDECIDED_CAP = 0.02          # of a case's real hits: lighting_rule's cap

# the case built to catch each wrong variant of the rule, and the overrides it is run with (None: the view's own)
MUTATION_CASE = {
    "key_frame_ignored": "four", "xy_swapped": "radius-4", "mod64_dropped": "radius-4", "noise_frame_of_view": "noise", "noise_row_of_64": "noise",
    "overrides_ignored": "four", "invprob_always": "four", "not_zeroed": "twenty", "sample_slot_up": "radius-4", "radius_at_zero": "pick-one",
    "unshadowed_shadowed": "four", "drawn_by_index": "twenty",
}
OVERRIDES = {"four": (16, 0)}          # J4: "four" (drawn with 3 lights, 2 samples) is evaluated a second time with every candidate drawn and no disc; "overrides_ignored" is held to those records


def make_case(sample_data, name):
    """-> (SceneData, view description, frames drawn)."""
    if name != "noise":
        return LC.make_case(MC.small_sample(sample_data), name)
    from sm64rt_legacy_renderer_amd import rt64
    d, _view, _frames = LC.make_case(MC.small_sample(sample_data), "material")
    veil = LC._add_quad(d, (-3.0, 2.0, 2.0), half=1.5)
    veil.material.shadowAlphaMultiplier = 2.0          # interpolated input alpha (1 up to a float32 rounding of the barycentrics) x 2, clamped: exactly 1
    veil.shader = (d.shader_id | M.OPT_NOISE, d.shader_filter, d.shader_haddr, d.shader_vaddr, rt64.SHADER_RASTER_ENABLED | rt64.SHADER_RAYTRACE_ENABLED)
    return d, dict(di_samples=1, max_lights=2), 1


def frame_of(view, frames):
    """What the rule needs to know of the view's last drawn frame."""
    return dict(width=W, height=H, frameCount=frames - 1, maxLights=view["max_lights"], diSamples=view["di_samples"])


def pixels():
    px, py = np.meshgrid(np.arange(0, W, 1), np.arange(0, H, 2), indexing="xy")
    return np.stack([px.reshape(-1), py.reshape(-1)], axis=1).astype(np.uint32)


def rays_and_keys(data, name):
    """-> (rays (N, 8) float32, keys (N, 4) uint32)."""
    seed = SEEDS[name]
    rng = np.random.default_rng(seed)
    pix = pixels()
    cam = ray_rule.camera_rays(data, W, H, pix)
    rnd = ray_rule.random_rays(data, seed, RANDOM_RAYS)
    frames = FRAMES[name]
    keys = np.zeros((len(cam) + len(rnd), 4), dtype=np.uint32)
    half = len(cam) // 2
    keys[:half, 0:2] = pix[:half]; keys[:half, 2] = frames[0]
    keys[half:len(cam), 0] = pix[half:, 0] + 64 * rng.integers(1, 40, len(cam) - half); keys[half:len(cam), 1] = pix[half:, 1] + 64 * rng.integers(1, 40, len(cam) - half)
    keys[half:len(cam), 2] = frames[1]
    keys[len(cam):, 0:2] = rng.integers(0, 4096, (len(rnd), 2)); keys[len(cam):, 2] = np.asarray(frames, dtype=np.uint32)[np.arange(len(rnd)) % len(frames)]
    keys[:, 3] = rng.integers(0, 2 ** 32, len(keys), dtype=np.uint64).astype(np.uint32)          # reserved is ignored
    return np.ascontiguousarray(np.concatenate([cam, rnd]).astype(np.float32)), keys


def oracle_hits(data, rays):
    """The closest hits of `rays` by the oracle's walk, in RT64_RAY_HIT's layout: what the CPU tests hand the rule where the GPU tests hand it the device's."""
    from oracle import oracle_py
    o = oracle_py.OracleScene(data)
    try:
        o.render(W, H, images=False)
        return ray_rule.trace(o, rays)
    finally:
        o.close()
