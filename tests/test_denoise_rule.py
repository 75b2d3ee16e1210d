"""tests/denoise_rule.py -- the GI filters restated from their specs -- checked on the CPU: first by properties that share no code with the rule
(a constant image stays constant, zero variance stays zero, sky passes through, edges in depth and normal stop the filter, the reference's border
weights sum to 1), then against the CPU oracle's frames (oracle/oracle_svgf.c, oracle_render.c gaussian_pass), fed with the oracle's own inputs.
The GPU holds the kernels to the same rule (tests/test_gpu_denoise.py)."""
import numpy as np
import pytest

import denoise_rule as R

ORACLE_LAST_ULPS = 1         # the last pass: one float16 rounding apart at most
ORACLE_CHAIN_ULPS = {1: 4, 0: 1}   # five passes: measured 3 (SVGF, 320x180 frames 0-2) and 1 (Gaussian)


def _guide(h, w, seed, sky=0.2):
    rng = np.random.default_rng(seed)
    depth = rng.uniform(1.0, 2.0, (h, w)).astype(np.float32)
    n = rng.normal(size=(h, w, 3)); n[..., 2] += 4.0
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float16).astype(np.float64)
    inst = np.where(rng.random((h, w)) < sky, -1, 0).astype(np.int32)
    return R.guide(depth, inst, n), depth, inst, n


def _ulps(a, b):
    return np.abs(a - b) / R.f16_ulp(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("step", R.STEPS)
def test_constant_colour_stays_constant_under_every_atrous_step(step):
    g = _guide(37, 53, step)[0]
    img = np.empty((37, 53, 4)); img[..., :3] = (0.25, 1.5, 3.0)
    img[..., 3] = R.f16(np.random.default_rng(step).uniform(0, 0.5, (37, 53)))
    out = R.atrous(img, g, step)
    assert np.array_equal(out[..., :3], img[..., :3])


def test_gaussian_border_weights_sum_to_one_and_keep_a_constant():
    for name, wt in R.GAUSS_CASES:
        assert abs(sum(wt) - 1.0) <= 3e-6, name
    img = np.empty((5, 6, 4)); img[..., :3] = (0.25, 1.5, 3.0); img[..., 3] = 7.0
    case = R.gauss_case(6, 5)
    assert set(np.unique(case)) == set(range(9))          # every border case occurs on a 6 x 5 frame
    out = R.gaussian_pass(img)
    assert np.array_equal(out[..., :3], img[..., :3]) and (out[..., 3] == 0.0).all()
    assert (R.gaussian_pass(img, img)[..., 3] == 7.0).all()    # the destination's alpha is left as it is


def test_gaussian_branch_order_on_one_pixel_wide_and_high_frames():
    names = [c[0] for c in R.GAUSS_CASES]
    case = lambda w, h: [names[k] for k in R.gauss_case(w, h).ravel()]
    assert case(1, 1) == ["top-left"]
    assert case(1, 4) == ["top-left", "left", "left", "bottom-left"]
    assert case(4, 1) == ["top-left", "top", "top", "top-right"]
    # one pixel wide: the top-left weights reach gInput[DTid + 1], which lies outside the texture and reads 0 -- a constant does not stay one
    img = np.ones((3, 1, 4))
    out = R.gaussian_pass(img)[..., 0]
    assert out[0, 0] < 1.0 and out[1, 0] < 1.0 and out[2, 0] == 1.0


def test_zero_variance_stays_zero():
    g = _guide(21, 40, 3)[0]
    img = np.random.default_rng(5).uniform(0, 2, (21, 40, 4)); img[..., 3] = 0.0
    x = R.f16(img)
    for step in R.STEPS:
        x = R.atrous(x, g, step)
        assert (x[..., 3] == 0.0).all()


def test_sky_pixels_pass_through_the_whole_chain_bit_for_bit():
    g, depth, inst, n = _guide(30, 45, 9, sky=0.4)
    rng = np.random.default_rng(1)
    raw = R.f16(rng.uniform(0, 2, (30, 45, 4))); raw[..., 3] = rng.integers(0, 8, (30, 45))
    mom = rng.uniform(0, 1, (30, 45, 2)); mom[..., 1] += mom[..., 0] ** 2
    out, _ = R.svgf(raw, mom, g)
    sky = inst < 0
    assert np.array_equal(out[sky][:, :3], raw[sky][:, :3]) and (out[sky][:, 3] == 0.0).all()
    assert not np.array_equal(out[~sky][:, :3], raw[~sky][:, :3])


def test_depth_and_normal_edges_stop_the_filter():
    """Left half red, right half blue, the variance large (a weak luminance stop).  A step in depth: the gradient of the last column before the step
    is the step itself, so that column may take some blue; no other pixel takes the other side's colour.  A 90-degree crease in the normal: none does."""
    h, w, edge = 24, 40, 20
    img = np.zeros((h, w, 4)); img[:, :edge, 0] = 1.0; img[:, edge:, 2] = 1.0; img[..., 3] = 4.0
    inst = np.zeros((h, w), np.int32)
    n = np.zeros((h, w, 3)); n[..., 2] = 1.0
    depth = np.ones((h, w), np.float32); depth[:, edge:] = 10.0
    g = R.guide(depth, inst, n)
    assert g["gz"][0, edge - 1] == 9.0 and (g["gz"][:, edge:] == 0.0).all()
    for step in R.STEPS:
        out = R.atrous(img, g, step)
        assert (out[:, :edge - 1, 2] == 0.0).all() and (out[:, edge:, 0] == 0.0).all(), step
        assert out[:, edge - 1, 2].max() > 0.0       # (the one column whose gradient spans the step)
    n2 = n.copy(); n2[:, edge:] = (1.0, 0.0, 0.0)
    g = R.guide(np.ones((h, w), np.float32), inst, n2)
    for step in R.STEPS:
        out = R.atrous(img, g, step)
        assert (out[:, :edge, 2] == 0.0).all() and (out[:, edge:, 0] == 0.0).all(), step


def test_guide_record_round_trip():
    g, depth, inst, n = _guide(9, 13, 4)
    back = R.unpack_guide(R.pack_guide(depth, inst, n))
    for k in ("valid", "depth", "gz", "normal"):
        assert np.array_equal(back[k], g[k]), k


# ---- against the oracle ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("w,h", [(320, 180), (33, 17)])
def test_rule_against_the_oracle(sample_data, mode, w, h):
    """Sample-scene frames 0-5 of the oracle with one GI sample and the denoiser (mode 1 SVGF, 0 Gaussian).  Frames 0-2 hold only young pixels (the
    7x7 estimate: the moments play no part), frames 3-5 take the variance of older pixels from the oracle's moments.  The rule applied to the
    oracle's last-pass input (filteredIndirectPing) = its result within 1 ulp, sky bit for bit; the whole chain from the raw image within
    ORACLE_CHAIN_ULPS."""
    from oracle import oracle_py
    o = oracle_py.OracleScene(sample_data)
    try:
        for f in range(6):
            r = o.render(w, h, giSamples=1, denoiserEnabled=1, denoiserMode=mode)
            filt = r["filteredIndirect"].astype(np.float64)
            valid = r["instanceId"] >= 0
            hist = r["indirectLight"][..., 3]
            assert (hist[valid] < 4.0).all() if f < 3 else (hist[valid] >= 4.0).any()
            if mode == 1:
                g = R.guide(r["depth"], r["instanceId"], r["normal"])
                last = R.atrous(r["filteredIndirectPing"], g, 16)
                chain, _ = R.svgf(r["indirectLight"], r["moments"], g)
                if f < 3:
                    assert np.array_equal(chain, R.svgf(r["indirectLight"], np.zeros_like(r["moments"]), g)[0])
                for got in (last, chain):
                    assert np.array_equal(got[~valid], filt[~valid])
                assert _ulps(last[valid], filt[valid]).max() <= ORACLE_LAST_ULPS, f
                assert _ulps(chain[valid], filt[valid]).max() <= ORACLE_CHAIN_ULPS[1], f
            else:
                last = R.gaussian_pass(r["filteredIndirectPing"])
                chain, ping = R.gaussian(r["indirectLight"])
                assert _ulps(last[..., :3], filt[..., :3]).max() <= ORACLE_LAST_ULPS, f
                assert _ulps(chain[..., :3], filt[..., :3]).max() <= ORACLE_CHAIN_ULPS[0], f
                assert np.array_equal(ping[..., 3], r["indirectLight"][..., 3])      # image 0 keeps the raw image's alpha
    finally:
        o.close()
