"""The kernels' raster (HUD / background) pass held to tests/raster_rule.py pixel by pixel (rules Z1-Z10), through every form the pass is launched in.

A case of tests/raster_cases.py is one 88 x 72 scene of raster instances.  The rule reads the scene as the host sent it and the bytes of the target before the
list -- the cleared buffer, or for a foreground list over a ray-traced frame the UNORM8 of OUTPUT_RGBA32F as read back (tests/test_gpu_denoise.py holds that
conversion bit for bit) -- so its result is computed once per (case, target, rows) and every launch form is held to the same one.

Asserted on every run, for FINAL_RGBA8 and BACKGROUND (raster_cases.hold): no decided pixel outside its byte interval; a decided pixel no layer covers keeps its
bytes (coverage); at most 1 % of the frame undecided; the exact case `ties` byte for byte with nothing undecided, and "covered exactly once" on the image itself.

Paths: `own-launch` raster_draw_kernel on a raster-only scene, gBackground cleared by the draw that fills it (frame_prologue 1, the default); `no-prologue`
frame_prologue 0: one setup launch per list, gBackground cleared by a memset; `rebuilt` always_rebuild 1: the lists re-staged every frame; `device-table` every
triangle an instance of its own, more than 16 in the list, so the setup reads the table from device memory and not from its arguments; `fold-1` / `fold-0` the
foreground list over the ray-traced sample scene, blended inside lean_frame_kernel or by its own launch; `band` a device that owns rows 19..53 (set_tile);
`strips-r/3` the three devices of a 3-way interleave of 16-row strips, each held to its own rows.

Regressions found by these cases: none so far (a case that exposes one is named here with the fix, as tests/test_gpu_denoise.py's check_svgf does)."""
import numpy as np
import pytest

import raster_cases as RC

pytestmark = pytest.mark.gpu

_rules = {}
BAND = (19, 53)


def _check(rt64_lib, sample_data, name, path, options=None, over=False, split=False, tile=None, interleave=None, fused=None, many=False):
    case = RC.make_case(sample_data, name, over_ray_traced=over, split=split)
    if many:
        n = sum(1 for i in case["data"].instances if not (case["data"].meshes[i.mesh].flags & 1) and not (i.flags & 1))
        assert n > 16, (name, n)
    images = RC.gpu_images(rt64_lib, case, options=options, tile=tile, interleave=interleave)
    st = images["stats"]
    print("raster_rule %-18s %-13s leanFrame=%d fusedFrame=%d primaryRays=%d" % ("gpu/" + path, name, st.leanFrame, st.fusedFrame, st.primaryRays))
    if fused is not None:                                    # (a second frame of an unchanged scene traces nothing: the ray-traced part is kept)
        assert st.fusedFrame == fused and (RC.base_bytes(images["output"])[..., :3] > 0).mean() > 0.5, (path, name, st.fusedFrame)
    elif not over:
        assert st.primaryRays == 0
    rows = images["rows"] if (tile or interleave) else None
    images["rows"] = rows
    key = (name, over, None if rows is None else rows.tobytes(), None if images["output"] is None else RC.base_bytes(images["output"]).tobytes())
    rule, _ = RC.hold(case, images, "gpu/" + path, rule=_rules.get(key))
    _rules[key] = rule


@pytest.mark.parametrize("name", RC.CASES)
def test_raster_pass_within_the_rule(rt64_lib, sample_data, name):
    _check(rt64_lib, sample_data, name, "own-launch")


@pytest.mark.parametrize("name", RC.CASES)
def test_raster_pass_within_the_rule_without_the_frame_prologue(rt64_lib, sample_data, name):
    _check(rt64_lib, sample_data, name, "no-prologue", options={"frame_prologue": 0})


@pytest.mark.parametrize("name", ["layers", "rects"])
def test_raster_pass_within_the_rule_with_lists_rebuilt_every_frame(rt64_lib, sample_data, name):
    _check(rt64_lib, sample_data, name, "rebuilt", options={"always_rebuild": 1})


@pytest.mark.parametrize("name", ["ties", "winding"])
def test_a_list_of_more_than_sixteen_instances_within_the_rule(rt64_lib, sample_data, name):
    _check(rt64_lib, sample_data, name, "device-table", split=True, many=True)


@pytest.mark.parametrize("fold", [1, 0])
@pytest.mark.parametrize("name", ["ties", "clip-corners", "layers", "textured"])
def test_foreground_list_over_a_ray_traced_frame_within_the_rule(rt64_lib, sample_data, name, fold):
    _check(rt64_lib, sample_data, name, "fold-%d" % fold, options={"fold_foreground": fold}, over=True, fused=1)


@pytest.mark.parametrize("name", ["ties", "layers", "rects"])
def test_a_band_is_held_to_its_own_rows(rt64_lib, sample_data, name):
    _check(rt64_lib, sample_data, name, "band", tile=BAND)


@pytest.mark.parametrize("rank", [0, 1, 2])
@pytest.mark.parametrize("name", ["ties", "layers"])
def test_every_device_of_a_three_way_interleave_is_held_to_its_own_strips(rt64_lib, sample_data, name, rank):
    _check(rt64_lib, sample_data, name, "strips-%d/3" % rank, interleave=(rank, 3))
