"""tests/sampler_rule.py pinned by checks that share no code with it: exact rational bilinear weights, texel centres, addressing periods,
mip selection at rho = 2^k, the closed-form footprint of a camera facing a plane head-on, and agreement with the oracle's sampler."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

import mipgen_rule
import sampler_rule as R


def _rand_levels(rng, w, h, mips=None):
    sizes = mipgen_rule.level_sizes(w, h)[:mips]
    return [rng.integers(0, 256, (lh, lw, 4), dtype=np.uint8) for lw, lh in sizes]


def _mod_addr(i, n, mode):
    """Addressing written out case by case with Python's own integers."""
    if mode == R.CLAMP:
        return 0 if i < 0 else (n - 1 if i >= n else i)
    if mode == R.MIRROR:
        k, r = divmod(i, n)                     # period 2n: even k keeps the direction, odd k runs backwards
        return r if k % 2 == 0 else n - 1 - r
    return i % n


def test_bilinear_weights_are_exact_fractions():
    rng = np.random.default_rng(1)
    for (w, h) in ((7, 5), (16, 8), (1, 3)):
        tex = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        u = (rng.random(300) * 6.0 - 3.0).astype(np.float32).astype(np.float64)
        v = (rng.random(300) * 6.0 - 3.0).astype(np.float32).astype(np.float64)
        for ha, va in ((R.WRAP, R.MIRROR), (R.CLAMP, R.WRAP), (R.MIRROR, R.CLAMP)):
            got, _, _ = R.sample_level([tex], u, v, 0, R.LINEAR, ha, va)
            for k in range(0, 300, 7):
                x = Fraction(u[k]) * w - Fraction(1, 2); y = Fraction(v[k]) * h - Fraction(1, 2)
                x0, y0 = math.floor(x), math.floor(y)
                fx, fy = x - x0, y - y0
                want = [Fraction(0)] * 4
                for (dx, wx) in ((0, 1 - fx), (1, fx)):
                    for (dy, wy) in ((0, 1 - fy), (1, fy)):
                        t = tex[_mod_addr(y0 + dy, h, va), _mod_addr(x0 + dx, w, ha)]
                        for c in range(4):
                            want[c] += wx * wy * Fraction(int(t[c]), 255)
                assert np.allclose(got[k], [float(q) for q in want], rtol=0, atol=1e-12)


def test_texel_centres_and_constant_textures():
    rng = np.random.default_rng(2)
    tex = rng.integers(0, 256, (6, 10, 4), dtype=np.uint8)
    yy, xx = np.mgrid[0:6, 0:10]
    u = (xx.ravel() + 0.5) / 10.0; v = (yy.ravel() + 0.5) / 6.0
    for filt in (R.POINT, R.LINEAR):
        got, _, _ = R.sample_level([tex], u, v, 0, filt, R.WRAP, R.WRAP)
        assert np.array_equal(R.to_byte(got), tex.reshape(-1, 4))
    levels = [np.full((max(37 >> l, 1), max(20 >> l, 1), 4), (12, 200, 77, 255), dtype=np.uint8) for l in range(6)]
    u = rng.random(500) * 8 - 4; v = rng.random(500) * 8 - 4
    for lod in (0.0, 0.3, 1.5, 2.99, 5.0):
        for filt in (R.POINT, R.LINEAR):
            for mode in (R.WRAP, R.MIRROR, R.CLAMP):
                val = R.sample_at_lod(levels, u, v, np.full(500, lod), filt, mode, mode)[0]
                assert np.allclose(val, np.array([12, 200, 77, 255]) / 255.0, rtol=0, atol=1e-12)


def test_addressing_periods_negatives_and_clamp():
    for n in (1, 2, 5, 8, 13):
        i = np.arange(-5 * n - 3, 5 * n + 4)
        for mode in (R.WRAP, R.MIRROR, R.CLAMP):
            got = R.address(i, n, mode)
            assert ((got >= 0) & (got < n)).all()
            assert list(got) == [_mod_addr(int(k), n, mode) for k in i]
        inside = np.arange(n)
        for mode in (R.WRAP, R.MIRROR, R.CLAMP):
            assert np.array_equal(R.address(inside, n, mode), inside)
        assert np.array_equal(R.address(i + n, n, R.WRAP), R.address(i, n, R.WRAP))
        assert np.array_equal(R.address(i + 2 * n, n, R.MIRROR), R.address(i, n, R.MIRROR))
        assert np.array_equal(R.address(-1 - i, n, R.MIRROR), R.address(i, n, R.MIRROR))          # mirror image about the edge at 0
        assert np.array_equal(R.address(2 * n - 1 - i, n, R.MIRROR), R.address(i, n, R.MIRROR))   # ... and about the edge at n
        assert (R.address(i[i < 0], n, R.CLAMP) == 0).all() and (R.address(i[i >= n], n, R.CLAMP) == n - 1).all()
    tex = np.zeros((1, 4, 4), dtype=np.uint8); tex[0, :, 0] = (10, 20, 30, 40)
    u = np.array([-0.1, -0.9, 1.1, 1.9, 2.1])
    got = lambda mode: R.to_byte(R.sample_level([tex], u, np.full(5, 0.5), 0, R.POINT, mode, R.WRAP)[0])[:, 0]
    assert list(got(R.WRAP)) == [40, 10, 10, 40, 10]
    assert list(got(R.MIRROR)) == [10, 40, 40, 10, 10]
    assert list(got(R.CLAMP)) == [10, 10, 40, 40, 40]


def test_lod_selection_blending_and_clamp():
    w0 = h0 = 64
    cols = [(l * 40, 255 - l * 30, (l * 97) % 256, 255) for l in range(7)]
    levels = [np.full((w0 >> l, h0 >> l, 4), cols[l], dtype=np.uint8) for l in range(7)]
    lv = lambda l: np.array(cols[l]) / 255.0
    u = np.array([0.3]); v = np.array([0.7])

    def at(rho_x, rho_y=0.0, filt=R.LINEAR, axis=0):
        g = np.array([[rho_x / w0, rho_y / h0]]); z = np.zeros((1, 2))
        return R.sample_grad(levels, u, v, g if axis == 0 else z, z if axis == 0 else g, filt, R.WRAP, R.WRAP)

    for k in range(7):
        for axis in (0, 1):
            r = at(2.0 ** k, axis=axis)
            assert r["lod"][0] == k and np.allclose(r["value"][0], lv(k), atol=1e-12)
            assert np.allclose(at(0.0, 2.0 ** k, axis=axis)["value"][0], lv(k), atol=1e-12)     # rho from the y extent
    for k in range(6):
        assert np.allclose(at(2.0 ** (k + 0.5))["value"][0], 0.5 * (lv(k) + lv(k + 1)), atol=1e-12)
        p_lo, p_hi = at(2.0 ** (k + 0.49), filt=R.POINT), at(2.0 ** (k + 0.51), filt=R.POINT)
        assert p_lo["level0"][0] == k and p_hi["level0"][0] == k + 1
        assert abs(p_lo["lod_margin"][0] - 0.01) < 1e-9
    assert np.allclose(at(3.0, 4.0)["lod"], np.log2(5.0))                   # |(3, 4)| = 5
    for tiny in (0.0, 1e-6, 0.5):
        assert at(tiny)["lod"][0] == 0.0 and np.allclose(at(tiny)["value"][0], lv(0))
    for huge in (2.0 ** 6, 2.0 ** 9, 1e30):
        assert at(huge)["lod"][0] == 6.0 and np.allclose(at(huge)["value"][0], lv(6))
        assert at(huge, filt=R.POINT)["level0"][0] == 6


def test_head_on_plane_has_the_closed_form_footprint():
    """Camera at the origin looking down -z at the plane z = -d, uv = k * (x, y): at the centre pixel the footprint is the pixel's
    world size times k along x and along y, and nothing across."""
    fov, near, far, SW, SH = math.radians(50.0), 0.1, 1000.0, 320, 180
    d, k = 7.0, 3.0
    view = np.eye(4)
    px, py = np.array([SW // 2 - 0.5]), np.array([SH // 2 - 0.5])      # pixel centre on the optical axis
    o, D, dDdx, dDdy = R.primary_rays(view, fov, near, far, SW, SH, px, py, SW, SH)
    assert np.allclose(o, 0.0) and np.allclose(D, [[0.0, 0.0, -1.0]])
    t = np.array([d])
    pos = np.array([[[-1.0, -1.0, -d], [1.0, -1.0, -d], [-1.0, 1.0, -d]]])
    uv = pos[:, :, :2] * k
    ddx, ddy = R.texture_grads(D, t, dDdx, dDdy, pos, uv, np.eye(3)[None], pos)
    pix = 2.0 * d * math.tan(fov / 2.0) / SH
    assert np.allclose(np.abs(ddx[0]), [pix * k, 0.0], atol=1e-12)
    assert np.allclose(np.abs(ddy[0]), [0.0, pix * k], atol=1e-12)
    # a render smaller than the screen (resolutionScale) keeps the screen's footprint: resolution.zw is the screen size
    _, _, dDdx2, dDdy2 = R.primary_rays(view, fov, near, far, SW, SH, np.array([119.5]), np.array([67.0]), 240, 135)
    assert np.allclose(dDdx2, dDdx) and np.allclose(dDdy2, dDdy)


def test_rule_agrees_with_the_oracle_sampler(oracle_lib):
    """A few thousand random (uv, gradient, filter, addressing) samples of a power-of-two and a non-power-of-two chain: the oracle's bytes
    lie within the rule's bounds, and equal the rule's byte wherever the margins leave one byte."""
    rng = np.random.default_rng(20261016)
    out = (C.c_float * 4)()
    strict_total = 0
    for (w, h) in ((64, 32), (100, 60), (1, 37)):
        levels = _rand_levels(rng, w, h)
        raw = mipgen_rule.dds_rgba8(levels)
        t = oracle_lib.oracle_texture_create_dds(raw.ctypes.data, raw.nbytes)
        assert t
        n = 1500
        u = (rng.random(n) * 7 - 3).astype(np.float32); v = (rng.random(n) * 7 - 3).astype(np.float32)
        scale = 2.0 ** rng.uniform(-3, len(levels) + 1, n) / max(w, h)
        ang = rng.random(n) * 2 * np.pi
        ddx = np.stack([np.cos(ang), np.sin(ang)], 1) * scale[:, None] * rng.uniform(0.2, 1.0, (n, 1))
        ddy = np.stack([-np.sin(ang), np.cos(ang)], 1) * scale[:, None] * rng.uniform(0.2, 1.0, (n, 1))
        ddx, ddy = ddx.astype(np.float32), ddy.astype(np.float32)
        for filt in (R.POINT, R.LINEAR):
            for ha, va in ((R.WRAP, R.MIRROR), (R.MIRROR, R.CLAMP), (R.CLAMP, R.WRAP)):
                got = np.zeros((n, 4))
                for k in range(n):
                    oracle_lib.oracle_texture_sample(t, float(u[k]), float(v[k]), float(ddx[k, 0]), float(ddx[k, 1]), float(ddy[k, 0]),
                                                     float(ddy[k, 1]), filt, ha, va, out)
                    got[k] = list(out)
                gb = R.to_byte(got)
                r = R.sample_grad_bounds(levels, u.astype(np.float64), v.astype(np.float64), ddx.astype(np.float64), ddy.astype(np.float64),
                                         filt, ha, va, du=2.0 ** -22 * np.maximum(np.abs(u), 1.0), dv=2.0 ** -22 * np.maximum(np.abs(v), 1.0),
                                         dlod=2.0 ** -18, eps=2.0 ** -19)
                s = r["strict"]
                assert np.array_equal(gb[s], r["byte"][s]), ((w, h), filt, ha, va, int((gb[s] != r["byte"][s]).any(1).sum()))
                assert ((gb >= r["lo"]) & (gb <= r["hi"])).all()
                if filt == R.POINT:
                    assert (r["corners"] == gb[None]).all(axis=2).any(axis=0).all()
                assert s.mean() > 0.9, s.mean()
                strict_total += int(s.sum())
        oracle_lib.oracle_texture_destroy(t)
    assert strict_total > 20000
