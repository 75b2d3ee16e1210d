"""The kernels' direct lighting held to tests/light_rule.py pixel by pixel, per light (rules L1-L9).

What the frame kernels read -- RT64_IMAGE_SHADING_POSITION, _SHADING_NORMAL, _SHADING_SPECULAR, _INSTANCE_ID as stored -- goes through the float64 rule, and
RT64_IMAGE_DIRECT_LIGHT_RAW (resDirect rounded to RGBA16F, w = 1: nothing is accumulated) must lie within the rule's bound at every pixel the rule decides.  A pixel is
undecided only where a selection or shadow threshold is closer than float32 can resolve; at most 0.5 % of a case's shaded pixels may be.  The cases are those of
tests/light_cases.py (88 x 72: the blue-noise address wraps, the 16-pixel tiles are partial); `four` and `offsets` also run on the other kernel paths."""
import numpy as np
import pytest

import light_cases as LC
import light_rule as R

pytestmark = pytest.mark.gpu

UNDECIDED_CAP = 0.005
IMAGES = ("SHADING_POSITION", "SHADING_NORMAL", "SHADING_SPECULAR", "INSTANCE_ID", "DIRECT_LIGHT_RAW", "VIEW_DIRECTION")
PATHS = {"default": {}, "three-kernels": {"fused_lean": 0, "lean_frames": 0}, "no-lds-cache": {"lds_cache": 0}, "general-kernels": {"simple_kernels": 0}}
# RT64_FRAME_STATS reports which frame form ran (fusedFrame), so `three-kernels` is asserted to have left the one-kernel frame.  It has no field for the LDS scene
# cache or for the simple / general build of the kernels: for those two paths the test can only require that the option was accepted, as the other tests that use
# them do (test_gpu_kbuffer.py, test_gpu_mipmaps.py, test_gpu_overlap.py); a stats field for them would be a change to the library's ABI and is not made here.
_images, _rules = {}, {}


def _render(rt64_lib, sample_data, name, path):
    """The images of a case on a kernel path, drawn once.  The five `frames-N` cases are one session of 65 frames read back at frames 0, 1, 62, 63 and 64."""
    if (name, path) not in _images:
        from sm64rt_legacy_renderer_amd import rt64, sample_scene
        group = [c for c in LC.CASES if c.startswith("frames-")] if name.startswith("frames-") else [name]
        made = {c: LC.make_case(sample_data, c) for c in group}
        d, view, _ = made[group[0]]
        want = {frames - 1: c for c, (_, _, frames) in made.items()}
        s = sample_scene.Rt64Scene(rt64_lib, d, LC.W, LC.H, hip_device=0)
        try:
            s.set_view_description(**view)
            for k, v in PATHS[path].items():
                assert s.option(k, v)
            for f in range(max(want) + 1):
                s.draw()
                if f in want:
                    # the path under test really ran: the one-kernel frame unless fused_lean = 0 sends the frame through primary_trace + primary_shade + direct
                    assert s.stats().fusedFrame == (0 if "fused_lean" in PATHS[path] else 1), (path, s.stats().fusedFrame, s.stats().leanFrame)
                    _images[(want[f], path)] = {k: s.readback(getattr(rt64, "IMAGE_" + k)) for k in IMAGES}
        finally:
            s.close()
    return _images[(name, path)]


def _rule(sample_data, name, img):
    """The rule on the default path's stored G-buffer, once per case (the float64 brute force over the scene's triangles runs here)."""
    if name not in _rules:
        d, view, frames = LC.make_case(sample_data, name)
        _rules[name] = (d, LC.run_rule(d, view, frames - 1, img["SHADING_POSITION"], img["SHADING_NORMAL"], img["SHADING_SPECULAR"], img["INSTANCE_ID"]))
    return _rules[name]


def _check(rt64_lib, sample_data, name, path):
    img = _render(rt64_lib, sample_data, name, path)
    base = _render(rt64_lib, sample_data, name, "default")
    for k in ("SHADING_POSITION", "SHADING_NORMAL", "SHADING_SPECULAR", "INSTANCE_ID"):       # the same inputs on every path, byte for byte
        assert img[k].tobytes() == base[k].tobytes(), k
    d, (value, bound, decided, info) = _rule(sample_data, name, base)
    lit = info["lit"]
    assert lit.sum() > 1500
    rd = R.ray_direction(LC.rule_inputs(d)["camera"])                                          # the camera restatement, against the f16 view direction
    assert (np.abs(img["VIEW_DIRECTION"][..., :3] - rd)[lit] <= 2.0 ** -11 * np.abs(rd[lit]) + 2.0 ** -24).all()
    stored = img["DIRECT_LIGHT_RAW"]
    worst, outside, undecided, mean = LC.compare(stored, value, bound, decided)
    shadow, multi, beyond = LC.shares(info)
    print("light_rule gpu    %-10s %-15s ratio=%.6f mean=%.6f undecided=%.3f%% %s shaded=%d in_shadow=%.3f multi=%.3f beyond_four_radii=%.3f"
          % (name, path, worst, mean, 100.0 * undecided, info["undecided"], int(lit.sum()), shadow, multi, beyond))
    if outside:
        dev = np.abs(stored[..., :3].astype(np.float64) - value[..., :3]); ratio = np.where(decided & lit, (dev / np.maximum(bound[..., :3], 1e-300)).max(axis=-1), 0.0)
        for y, x in list(zip(*np.nonzero(ratio >= 1.0)))[:8]:
            print("   outside: pixel (%d, %d) instance %d stored %s rule %s bound %s draws %d candidates %d"
                  % (x, y, img["INSTANCE_ID"][y, x], stored[y, x, :3], value[y, x, :3], bound[y, x, :3], info["draws"][y, x], info["candidates"][y, x]))
    assert outside == 0 and worst < 1.0, (outside, worst)
    assert undecided <= UNDECIDED_CAP, undecided
    miss = ~lit
    assert np.array_equal(stored[miss], np.tile(np.float32([1, 1, 1, 0]), (int(miss.sum()), 1))) and (stored[lit][:, 3] == 1.0).all()
    need = LC.SHARES[name]
    assert shadow >= need[0] and multi >= need[1] and beyond >= need[2], (shadow, multi, beyond, need)


@pytest.mark.parametrize("name", LC.CASES)
def test_direct_light_within_the_rule(rt64_lib, sample_data, name):
    _check(rt64_lib, sample_data, name, "default")


@pytest.mark.parametrize("path", [p for p in PATHS if p != "default"])
@pytest.mark.parametrize("name", ["four", "offsets"])
def test_direct_light_within_the_rule_on_every_kernel_path(rt64_lib, sample_data, name, path):
    _check(rt64_lib, sample_data, name, path)
