"""Scene cases of the raster-rule tests (tests/test_raster_rule.py on the CPU oracle, tests/test_gpu_raster_rule.py on the GPU) and `hold`, which compares a side's
FINAL_RGBA8 and BACKGROUND with tests/raster_rule.py.

Every case is one small scene of raster instances at 88 x 72 -- no multiple of the 32-pixel wave row or of the 8-row block, four and a half 16-row strips -- built
for one family of mistakes ("The raster pass against a float64 rule").  Clip-space positions are written as NDC x, y, a depth fraction z / w and w; the
mesh stores (x w, y w, z, w) in float32 and the rule reads what is stored.

Vertex alphas are 0.6, 0.8, 0.35 ..., never 0.5: 0.5 * 255 = 127.5 is a UNORM8 tie."""
import copy

import numpy as np

import light_cases as LC
import mipgen_rule
import raster_rule as R

W, H = LC.W, LC.H                       # 88 x 72
CLEAR = (0, 0, 0, 255)                  # the back buffer of a frame with nothing ray traced: opaque black (gBackground is cleared to 0)
UNDECIDED_CAP = 0.01                    # of the frame's pixels, per image
# vertex colour alone: colour and alpha cycles both (0 - 0) * 0 + INPUT1, alpha option: 44-byte vertices (position, normal, input1)
SHADER_VERTEX_COLOUR = (1 << 9) | (1 << 21) | (1 << 24)
# TEXEL0 * INPUT1 for the colour, INPUT1's alpha for the alpha (two different formulas), alpha option: 52-byte vertices (position, normal, uv, input1)
SHADER_TEXTURED = 5 | (1 << 6) | (1 << 21) | (1 << 24)
VC_DTYPE = np.dtype([("position", "<f4", 4), ("normal", "<f4", 3), ("input1", "<f4", 4)])
TX_DTYPE = np.dtype([("position", "<f4", 4), ("normal", "<f4", 3), ("uv", "<f4", 2), ("input1", "<f4", 4)])
RED, GREEN, BLUE = (1.0, 0.2, 0.2), (0.2, 1.0, 0.2), (0.2, 0.2, 1.0)
FLAT = (1.0, 0.4, 0.2)                 # x 0.6 x 255 = 153, 61.2, 30.6: no byte tie
POINT, LINEAR = 0, 1
WRAP, MIRROR, CLAMP = 0, 1, 2

CASES = ("ties", "winding", "clip-planes", "clip-corners", "clip-behind", "clip-guard", "layers", "rects", "textured")
EXACT = ("ties",)

# Minimum counts that make a case worth running, asserted on the rule's own info: about half of what the rule counts (profiles/raster_rule_deviation.txt).
SHARES = {
    "ties": dict(exact_triangles=60, ties=480, covered=880, back_facing=640),
    "winding": dict(back_facing=480, covered=980, empty_triangles=5, drawn_triangles=8),
    "clip-planes": dict(clipped=2200, cut_near=22, cut_far=100, behind_one=220),
    "clip-corners": dict(clipped=1150, cut_near=2300, cut_far=130),
    "clip-behind": dict(behind_one=170, behind_two=150, empty_triangles=1),
    "clip-guard": dict(cut_guard=340, clipped=3000),
    "layers": dict(two_layers=1400, roundtrip_differs=360, background_covered=2100),
    "rects": dict(scissored=22000, covered=920, background_covered=6336),
    "textured": dict(minified=1400, magnified=430, covered=2300),
}

# the case built to catch each wrong variant of the rule
MUTATION_CASE = {
    "bottom_right_rule": "ties", "pixel_corner": "ties", "affine_attributes": "winding", "rw_not_reoriented": "winding", "y_not_flipped": "winding",
    "rect_origin_top_left": "rects", "scissor_right_inclusive": "rects", "back_faces_culled": "winding", "near_plane_ignored": "clip-planes",
    "far_plane_ignored": "clip-planes", "guard_band_at_one": "clip-guard", "clipped_attributes_from_piece_corners": "clip-corners", "no_byte_round_trip": "layers",
    "premultiplied_blend": "layers", "draw_order_reversed": "layers", "background_after_foreground": "layers", "gradients_zero": "textured",
}


# ---- building a scene ----------------------------------------------------------------------------------------------------------------------------

def V(x, y, w=1.0, z=0.5):
    """NDC (x, y), depth fraction z / w and w -> the clip-space position the host sends."""
    return (x * w, y * w, z * w, w)


class _Builder:
    def __init__(self, sample_data, over_ray_traced):
        from sm64rt_legacy_renderer_amd import rt64
        self.rt64 = rt64
        d = copy.copy(sample_data)
        d.meshes = list(sample_data.meshes); d.textures = list(sample_data.textures)
        keep = [i for i in sample_data.instances if sample_data.meshes[i.mesh].flags & rt64.MESH_RAYTRACE_ENABLED]
        d.instances = list(keep) if over_ray_traced else []
        self.d, self.sample, self.levels = d, sample_data, {}

    def mesh(self, tris, colours=None, alpha=0.6, uvs=None):
        """tris: [(p0, p1, p2)] clip-space positions; colours: per triangle three (r, g, b) or (r, g, b, a), or None (FLAT); uvs: per triangle three (u, v)."""
        from sm64rt_legacy_renderer_amd import sample_scene
        v = np.zeros(3 * len(tris), dtype=TX_DTYPE if uvs is not None else VC_DTYPE)
        for t, tri in enumerate(tris):
            for k in range(3):
                c = (FLAT,) * 3 if colours is None else colours[t]
                col = tuple(c[k]) + ((alpha,) if len(c[k]) == 3 else ())
                v["position"][3 * t + k] = tri[k]; v["normal"][3 * t + k] = (0.0, 1.0, 0.0); v["input1"][3 * t + k] = col
                if uvs is not None:
                    v["uv"][3 * t + k] = uvs[t][k]
        self.d.meshes.append(sample_scene.MeshData("raster%d" % len(self.d.meshes), 0, v, np.arange(len(v), dtype=np.uint32)))
        return len(self.d.meshes) - 1

    def instance(self, mesh, background=False, scissor=None, viewport=None, shader=None, diffuse=4):
        from sm64rt_legacy_renderer_amd import sample_scene
        stock = self.sample.instances[0]
        textured = "uv" in self.d.meshes[mesh].vertices.dtype.names
        sh = shader or ((SHADER_TEXTURED if textured else SHADER_VERTEX_COLOUR), LINEAR, WRAP, WRAP, self.sample.shader_flags)
        i = sample_scene.InstanceData("raster%d" % len(self.d.instances), mesh, stock.transform, stock.transform, diffuse, None, None,
                                      sample_scene.copy_material(stock.material), self.rt64.INSTANCE_RASTER_BACKGROUND if background else 0,
                                      scissor=scissor, viewport=viewport, shader=tuple(sh))
        self.d.instances.append(i)
        return i

    def texture_with_chain(self, image):
        """An RGBA8 image with its generated mip chain (tests/mipgen_rule.py), handed to both sides as one DDS file -> texture index."""
        from sm64rt_legacy_renderer_amd import sample_scene
        levels = mipgen_rule.chain(np.ascontiguousarray(image))
        self.d.textures.append(sample_scene.TextureData("chain%d" % len(self.d.textures), self.rt64.TEXTURE_FORMAT_DDS, mipgen_rule.dds_rgba8(levels)))
        self.levels[len(self.d.textures) - 1] = levels
        return len(self.d.textures) - 1


def _ties(b):
    """Exact: a 64 x 64 viewport whose corner is pixel (8, 4), so NDC k / 64 is half a pixel.  Positions below are in HALF PIXELS of the viewport, y down."""
    vp = (8, H - 4 - 64, 64, 64)

    def P(hx, hy):
        return V((hx - 64) / 64.0, (64 - hy) / 64.0)
    tris, region = [], np.zeros((H, W), dtype=bool)
    flip = 0

    def add(p0, p1, p2):
        nonlocal flip
        tris.append((P(*p0), P(*p1), P(*p2)) if flip % 3 else (P(*p0), P(*p2), P(*p1)))     # both orientations, mixed
        flip += 1

    def quads(x0, y0, size, n):
        """n x n quads of `size` half pixels from (x0, y0), split along alternating diagonals: every edge is shared."""
        for j in range(n):
            for i in range(n):
                a, c = (x0 + i * size, y0 + j * size), (x0 + (i + 1) * size, y0 + (j + 1) * size)
                bb, dd = (c[0], a[1]), (a[0], c[1])
                if (i + j) % 2:
                    add(a, bb, c); add(a, c, dd)
                else:
                    add(a, bb, dd); add(bb, c, dd)
        cx = (np.arange(W) - 8) * 2 + 1; cy = (np.arange(H) - 4) * 2 + 1                 # pixel centres in half pixels of the viewport
        region[np.ix_((cy >= y0) & (cy < y0 + n * size), (cx >= x0) & (cx < x0 + n * size))] = True
    quads(4, 4, 14, 3)            # vertices on pixel corners (even): the 45-degree diagonals of 7-pixel quads run through pixel centres
    quads(61, 5, 12, 4)           # vertices on pixel centres (odd): horizontal and vertical edges through centres
    centre, rim = (27, 95), [(20, 0), (20, 20), (0, 20), (-20, 20), (-20, 0), (-20, -20), (0, -20), (20, -20)]       # a fan around a vertex on a pixel centre
    for k in range(8):
        add(centre, (centre[0] + rim[k][0], centre[1] + rim[k][1]), (centre[0] + rim[(k + 1) % 8][0], centre[1] + rim[(k + 1) % 8][1]))
    cx = (np.arange(W) - 8) * 2 + 1; cy = (np.arange(H) - 4) * 2 + 1
    region[np.ix_((cy >= 75) & (cy < 115), (cx >= 7) & (cx < 47))] = True
    # single triangles with a vertex on a pixel centre and edges of other slopes, apart from the tiled regions
    add((70, 70), (118, 82), (86, 118)); add((66, 100), (90, 124), (58, 122))
    b.instance(b.mesh(tris), viewport=vp)
    return dict(region=region)


def _winding(b):
    """The same triangles in both orientations with three vertex colours and per-vertex w up to 10 : 1, slivers, sub-pixel and zero-area triangles."""
    shapes = [((-0.93, 0.91), (-0.41, 0.83), (-0.71, 0.13)), ((-0.31, 0.87), (0.29, 0.93), (0.03, 0.17)), ((0.39, 0.89), (0.95, 0.77), (0.61, 0.11))]
    ws = [(1.0, 10.0, 3.0), (4.0, 0.5, 1.5), (0.7, 2.0, 7.0)]
    tris, cols = [], []
    for s, w in zip(shapes, ws):
        tris.append(tuple(V(p[0], p[1], wk) for p, wk in zip(s, w))); cols.append((RED, GREEN, BLUE))
        lower = tuple(V(p[0] + 0.013, p[1] - 0.97, wk) for p, wk in zip(s, w))          # the same triangle lower down, its corners 1 and 2 exchanged
        tris.append((lower[0], lower[2], lower[1])); cols.append((RED, BLUE, GREEN))
    slivers = [((-0.9, 0.05), (0.5, 0.012), (0.5, 0.003)), ((0.7, 0.06), (0.703, -0.05), (0.71, 0.06)), ((0.81, 0.02), (0.95, -0.04), (0.8, 0.012))]
    for k, s in enumerate(slivers):
        pts = tuple(V(p[0], p[1], 1.0 + k) for p in s)
        tris.append(pts if k % 2 else (pts[0], pts[2], pts[1])); cols.append((RED, GREEN, BLUE))
    for k in range(4):                                                                   # smaller than a pixel (a pixel is 0.023 x 0.028 NDC)
        x, y = -0.5 + 0.31 * k, -0.02 + 0.003 * k
        tris.append((V(x, y), V(x + 0.011, y + 0.002), V(x + 0.004, y + 0.013))); cols.append((RED, GREEN, BLUE))
    zero = [((0.25, 0.25), (0.25, 0.25), (0.5, 0.75)), ((-0.5, -0.5), (0.0, 0.0), (0.5, 0.5)), ((0.125, -0.75), (0.125, -0.25), (0.125, 0.5)),
            ((-0.75, 0.5), (0.25, 0.5), (-0.25, 0.5)), ((0.5, 0.5), (0.5, 0.5), (0.5, 0.5)), ((0.0, 0.0), (0.5, 0.25), (-0.5, -0.25))]
    for s in zero:                                                                       # no area: they draw nothing
        tris.append(tuple(V(p[0], p[1]) for p in s)); cols.append((RED, GREEN, BLUE))
    b.instance(b.mesh(tris, cols, alpha=0.8))
    return {}


def _cell(k, nx, ny, pts, margin=0.06):
    """Triangle corners given in a unit cell (x right, y up, may leave the cell) -> NDC of cell k of an nx x ny grid."""
    cx, cy = k % nx, k // nx
    sx, sy = 2.0 / nx, 2.0 / ny
    return [(-1.0 + sx * (cx + margin + (1 - 2 * margin) * p[0]), 1.0 - sy * (cy + 1 - margin - (1 - 2 * margin) * p[1])) for p in pts]


def _clip_planes(b):
    """Each of the seven planes crossed alone (a vertex with w <= 0 is also outside the far plane and one guard plane: it cannot be alone), one triangle a cell."""
    tris = []
    base = [(0.05, 0.07), (0.93, 0.21), (0.37, 0.95)]
    p = _cell(0, 4, 2, base); tris.append((V(*p[0]), V(*p[1]), (0.3, 0.2, 0.0, -0.5)))                       # W: the third corner behind the eye
    p = _cell(1, 4, 2, base); tris.append((V(*p[0], 1.0, 0.5), V(*p[1], 1.0, 0.5), V(*p[2], 1.0, -0.4)))       # NEAR
    p = _cell(2, 4, 2, base); tris.append((V(*p[0], 2.0, 0.5), V(*p[1], 1.0, 1.6), V(*p[2], 1.0, 0.5)))        # FAR
    p = _cell(3, 4, 2, base); tris.append((V(*p[0]), V(*p[1]), V(-6.3, p[2][1])))                              # X-
    p = _cell(4, 4, 2, base); tris.append((V(*p[0]), V(6.1, p[1][1], 2.0), V(*p[2])))                          # X+
    p = _cell(5, 4, 2, base); tris.append((V(p[0][0], -5.7), V(*p[1]), V(*p[2])))                              # Y-
    p = _cell(6, 4, 2, base); tris.append((V(*p[0]), V(*p[1]), V(p[2][0], 7.9, 3.0)))                          # Y+
    p = _cell(7, 4, 2, base); tris.append((V(*p[0]), V(*p[2]), V(*p[1])))                                      # none, the other orientation
    b.instance(b.mesh(tris, [(RED, GREEN, BLUE)] * len(tris)))
    return {}


def _clip_corners(b):
    """Two and three planes crossed by one triangle."""
    tris = []
    p = _cell(0, 3, 2, [(0.1, 0.1), (0.9, 0.2), (0.4, 0.9)]); tris.append((V(*p[0], 1.0, -0.3), V(*p[1], 1.0, 0.5), V(*p[2], 1.0, 1.5)))       # near and far
    p = _cell(1, 3, 2, [(0.1, 0.1), (0.9, 0.2), (0.4, 0.9)]); tris.append((V(*p[0], 1.0, 0.6), V(5.5, 6.5, 2.0, 0.4), V(*p[2], 1.0, 0.3)))     # X+ and Y+: a corner of the guard band
    p = _cell(2, 3, 2, [(0.1, 0.1), (0.9, 0.2), (0.4, 0.9)]); tris.append((V(*p[0], 1.0, -0.5), V(*p[1], 1.0, 0.5), V(-7.0, p[2][1], 1.5, 0.5)))   # near and X-
    p = _cell(3, 3, 2, [(0.1, 0.1), (0.9, 0.2), (0.4, 0.9)]); tris.append((V(*p[0], 1.0, -0.4), V(6.0, p[1][1], 1.0, 0.5), V(p[2][0], 9.0, 1.0, 1.3)))   # near, X+, Y+ / far
    p = _cell(4, 3, 2, [(0.1, 0.1), (0.9, 0.2), (0.4, 0.9)]); tris.append((V(-5.0, -6.0, 1.0, 0.2), V(*p[1], 2.0, 1.4), V(*p[2], 1.0, 0.5)))    # X-, Y-, far
    p = _cell(5, 3, 2, [(0.1, 0.1), (0.9, 0.2), (0.4, 0.9)]); tris.append((V(*p[0], 1.0, 0.5), V(*p[2], 3.0, 1.7), V(*p[1], 1.0, -0.6)))       # far and near, the other orientation
    b.instance(b.mesh(tris, [(RED, GREEN, BLUE)] * len(tris)))
    return {}


def _clip_behind(b):
    """One, two and all three corners behind the eye (w <= 0)."""
    tris = [((-0.8, -0.6, 0.2, 1.0), (0.9, -0.7, 0.2, 1.0), (0.1, 0.4, 0.5, -0.5)),             # one
            ((-0.5, -0.9, 0.1, 0.6), (0.4, 0.8, 0.3, -0.2), (0.9, -0.2, 0.3, -0.4)),            # two
            ((-0.5, 0.5, 0.1, -1.0), (0.5, 0.5, 0.1, -0.5), (0.0, -0.5, 0.1, 0.0)),             # all three (one of them at w = 0): nothing
            ((0.55, 0.35, 0.5, 1.0), (0.85, 0.4, 0.5, 1.0), (0.7, 0.8, 0.5, 1.0))]              # an ordinary one, drawn last
    b.instance(b.mesh(tris, [(RED, GREEN, BLUE)] * len(tris)))
    return {}


def _clip_guard(b):
    """A 22 x 18 viewport (a quarter of the frame along each axis) under a whole-frame scissor: NDC +-4 is 44 pixels left and right of x = 49 and 36 above and below
    y = 33, so the guard band's left edge (x = 5) and bottom edge (y = 69) lie on screen."""
    tris = [(V(-9.0, -8.0), V(9.5, -7.0), V(0.5, 11.0)), (V(-3.1, 0.4, 2.0), V(-5.9, -2.3, 1.0), (V(-2.9, -5.3, 3.0)))]
    b.instance(b.mesh(tris, [(RED, GREEN, BLUE), (BLUE, RED, GREEN)]), viewport=(38, 30, 22, 18), scissor=(0, 0, W, H))
    return {}


def _layers(b):
    """Overlapping translucent triangles in two foreground instances over a background instance.  The alphas are such that blending with the stored byte of the layer
    below differs from a blend kept in float (SHARES: roundtrip_differs)."""
    bg = [(V(-1.0, -1.0), V(1.0, -0.9), V(-0.2, 1.0)), (V(-0.9, 0.9), V(0.95, 0.6), V(0.9, -0.95))]
    b.instance(b.mesh(bg, [(RED, GREEN, BLUE), (BLUE, BLUE, RED)], alpha=0.37), background=True)
    one = [(V(-0.9, -0.8), V(0.6, -0.6), V(-0.2, 0.9)), (V(-0.5, -0.9), V(0.9, 0.1), V(-0.7, 0.5)), (V(0.1, -0.7), V(0.8, 0.8), V(-0.6, 0.2))]
    b.instance(b.mesh(one, [(RED, GREEN, BLUE), (GREEN, BLUE, RED), (BLUE, RED, GREEN)], alpha=0.6))
    two = [(V(-0.45, -0.4), V(0.5, -0.35), V(0.05, 0.6))]
    b.instance(b.mesh(two, [((0.9, 0.9, 0.1, 0.35), (0.1, 0.9, 0.9, 0.45), (0.9, 0.1, 0.9, 0.25))]))
    return {}


def _rects(b):
    """Scissors of one pixel, scissors on every frame edge, a scissor that misses, a viewport partly off screen; no rect is vertically symmetric."""
    full = [(V(-1.0, -1.0), V(3.0, -1.0), V(-1.0, 3.0))]                          # covers the whole viewport
    cols = [(RED, GREEN, BLUE)]
    small = [(V(-0.9, -0.8), V(0.7, -0.5), V(-0.3, 0.9))]
    m_full, m_small = b.mesh(full, cols, alpha=0.7), b.mesh(small, cols, alpha=0.7)
    b.instance(m_full, scissor=(20, 9, 1, 40))                                    # one pixel wide
    b.instance(m_full, scissor=(30, 50, 40, 1))                                   # one pixel high
    b.instance(m_full, scissor=(0, 3, 6, 30))                                     # on the left edge
    b.instance(m_full, scissor=(80, 20, 8, 25))                                   # on the right edge
    b.instance(m_full, scissor=(40, 0, 20, 5))                                    # on the bottom edge (RT64_RECT: y up from the bottom)
    b.instance(m_full, scissor=(50, 64, 25, 8))                                   # on the top edge
    b.instance(m_small, scissor=(70, 60, 10, 8))                                  # misses the triangle
    b.instance(m_small, viewport=(-20, 40, 60, 50), scissor=(0, 30, 45, 42))      # the viewport leaves the screen to the left and above
    b.instance(m_small, viewport=(44, 8, 40, 30))                                 # a viewport alone, low on the screen
    b.instance(m_full, scissor=(60, 10, 50, 12), background=True)                 # a scissor that leaves the screen, on the background list
    return {}


def _textured(b):
    """The sample's tiles texture with a generated chain on quads under a strong perspective, minified and magnified; filters, addressing modes, and a combiner with
    separate colour and alpha formulas (SHADER_TEXTURED)."""
    tiles = b.texture_with_chain(b.sample.textures[4].data)
    flags = b.sample.shader_flags
    combos = [(LINEAR, WRAP, WRAP, 6.0), (POINT, WRAP, MIRROR, 6.0), (LINEAR, MIRROR, CLAMP, 2.5), (POINT, CLAMP, WRAP, 0.04), (LINEAR, CLAMP, MIRROR, 0.05), (LINEAR, WRAP, WRAP, 0.03)]
    for k, (filt, ha, va, span) in enumerate(combos):
        p = _cell(k, 3, 2, [(0.0, 0.0), (1.0, 0.05), (0.95, 1.0), (0.05, 0.9)], margin=0.04)
        w = (1.0, 1.3, 6.0, 8.0)                                               # the top of the quad is far away
        q = [V(p[i][0], p[i][1], w[i]) for i in range(4)]
        t = [(-0.3 * span, -0.2 * span), (span, -0.1 * span), (1.1 * span, 1.2 * span), (-0.2 * span, span)]
        c = [(1.0, 0.9, 0.8, 0.9), (0.8, 1.0, 0.9, 0.7), (0.9, 0.8, 1.0, 0.8), (1.0, 1.0, 1.0, 0.6)]
        m = b.mesh([(q[0], q[1], q[2]), (q[0], q[2], q[3])], [(c[0], c[1], c[2]), (c[0], c[2], c[3])], uvs=[(t[0], t[1], t[2]), (t[0], t[2], t[3])])
        b.instance(m, shader=(SHADER_TEXTURED, filt, ha, va, flags), diffuse=tiles)
    return {}


_BUILD = {"ties": _ties, "winding": _winding, "clip-planes": _clip_planes, "clip-corners": _clip_corners, "clip-behind": _clip_behind, "clip-guard": _clip_guard,
          "layers": _layers, "rects": _rects, "textured": _textured}


def make_case(sample_data, name, over_ray_traced=False, split=False):
    """dict(name, data, levels, exact, region (ties: the tiled pixels) ...).  over_ray_traced: the sample's sphere and floor stay, so the foreground list lies over a
    ray-traced frame; split: every triangle becomes an instance of its own, in the same order (the same picture from a list of many instances)."""
    b = _Builder(sample_data, over_ray_traced)
    extra = _BUILD[name](b)
    if split:
        _split(b)
    return dict(dict(name=name, data=b.d, levels=b.levels, exact=name in EXACT, over_ray_traced=over_ray_traced), **extra)


def _split(b):
    from sm64rt_legacy_renderer_amd import sample_scene
    out = []
    for inst in b.d.instances:
        mesh = b.d.meshes[inst.mesh]
        if mesh.flags & b.rt64.MESH_RAYTRACE_ENABLED:
            out.append(inst); continue
        for t in range(len(mesh.indices) // 3):
            v = mesh.vertices[np.asarray(mesh.indices[3 * t:3 * t + 3], dtype=np.int64)].copy()
            b.d.meshes.append(sample_scene.MeshData("%s.%d" % (mesh.name, t), 0, v, np.arange(3, dtype=np.uint32)))
            c = copy.copy(inst); c.mesh = len(b.d.meshes) - 1; c.name = "%s.%d" % (inst.name, t)
            out.append(c)
    b.d.instances = out


# ---- what the rule reads -------------------------------------------------------------------------------------------------------------------------

def rule_scene(case, base=None, rows=None):
    """The scene as the host sent it, for raster_rule.frame: per raster instance the positions, indices, vertex inputs, UVs, shader, texture levels and rects."""
    data = case["data"]
    out = []
    for inst in data.instances:
        mesh = data.meshes[inst.mesh]
        if mesh.flags & 1:                                   # RT64_MESH_RAYTRACE_ENABLED
            continue
        v = mesh.vertices
        sid, filt, ha, va, _ = inst.shader
        out.append(dict(pos=v["position"].astype(np.float64), indices=np.asarray(mesh.indices, dtype=np.int64), inputs=[v["input1"].astype(np.float64)],
                        uv=v["uv"].astype(np.float64) if "uv" in v.dtype.names else None, shader_id=int(sid), filter=int(filt), haddr=int(ha), vaddr=int(va),
                        levels=case["levels"].get(inst.diffuse), viewport=inst.viewport, scissor=inst.scissor, background=bool(inst.flags & 1)))
    return dict(width=W, height=H, instances=out, base=base, rows=rows, clear=CLEAR)


def run_rule(case, base=None, rows=None, mutate=None):
    return R.frame(rule_scene(case, base, rows), mutate=mutate)


# ---- the sides -----------------------------------------------------------------------------------------------------------------------------------

def oracle_images(case):
    """dict(final, background, output) of the CPU oracle."""
    from oracle import oracle_py

    class Scene(oracle_py.OracleScene):
        def _desc(self, inst):
            d = super()._desc(inst)
            if getattr(inst, "shader", None) is not None:            # the binding fills in the scene's shader; these scenes give every raster instance its own
                d.shaderId, d.filter, d.hAddr, d.vAddr, d.shaderFlags = inst.shader
            return d
    o = Scene(case["data"])
    try:
        ref = o.render(W, H, maxReflections=0)
        return dict(final=ref["final"], background=ref["background"], output=ref["output"])
    finally:
        o.close()


def gpu_images(rt64_lib, case, options=None, tile=None, interleave=None, frames=2):
    """The same scene on the device.  -> dict(final (the rows this device owns), background, output, rows (H,) bool, stats)."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene, tiles
    s = sample_scene.Rt64Scene(rt64_lib, case["data"], W, H, hip_device=0)
    try:
        assert s.option("max_reflections", 0)
        for key, v in (options or {}).items():
            assert s.option(key, v), key
        rows = np.ones(H, dtype=bool)
        if tile is not None:
            s.set_tile(*tile)
            rows[:] = False; rows[tile[0]:tile[1]] = True
        if interleave is not None:
            s.set_interleave(*interleave)
            rows[:] = False
            for a, c in tiles.strip_ranges(H, *interleave):
                rows[a:c] = True
        for _ in range(frames):
            s.draw()
        st = s.stats()
        part = s.readback(rt64.IMAGE_FINAL_RGBA8)
        final = np.zeros((H, W, 4), dtype=np.uint8)
        assert part.shape[0] == int(rows.sum()), (part.shape, int(rows.sum()))
        final[rows] = part
        has_bg = any(i.flags & rt64.INSTANCE_RASTER_BACKGROUND for i in case["data"].instances)
        out = dict(final=final, rows=rows, stats=st, background=s.readback(rt64.IMAGE_BACKGROUND).copy() if has_bg else None, output=None)
        if case["over_ray_traced"] and tile is None and interleave is None:
            out["output"] = s.readback(rt64.IMAGE_OUTPUT_RGBA32F).copy()
        return out
    finally:
        s.close()


def base_bytes(output):
    """The back buffer before the foreground list: OUTPUT_RGBA32F stored as UNORM8 (tests/test_gpu_denoise.py holds that conversion)."""
    return np.clip(np.floor(np.asarray(output, dtype=np.float64) * 255.0 + 0.5), 0, 255).astype(np.uint8)


# ---- holding a side to the rule ------------------------------------------------------------------------------------------------------------------

def counts(case, rule):
    c = dict(rule["final"]["counts"])
    if rule["background"] is not None:
        c["background_covered"] = rule["background"]["counts"]["covered"]
    return c


def roundtrip_differs(case, rule, base=None):
    """Pixels at which the bytes of a blend kept in float32 across the layers cannot be the bytes of the blend through the stored byte."""
    wrong = run_rule(case, base=base, mutate="no_byte_round_trip")["final"]
    right = rule["final"]
    dec = ~right["undecided"] & ~wrong["undecided"]
    return int((dec & ((wrong["hi"] < right["lo"]) | (wrong["lo"] > right["hi"])).any(axis=-1)).sum())


def hold(case, images, side, rule=None, log=print, shares=True):
    """FINAL_RGBA8 and BACKGROUND of one side against the rule; asserts the conditions of the tests and returns (rule, report rows)."""
    name = case["name"]
    rows = images.get("rows")
    base = base_bytes(images["output"]) if case["over_ray_traced"] else None
    if rule is None:
        rule = run_rule(case, base=base, rows=rows)
    out = []
    for image, key in (("FINAL_RGBA8", "final"), ("BACKGROUND", "background")):
        if rule[key] is None:
            assert images.get(key) is None or not np.asarray(images[key]).any(), (name, image)
            continue
        r = rule[key]
        j = R.judge(r, images[key], rows if key == "final" else None)
        # coverage: a decided pixel no layer covers keeps the bytes it had (its interval is that byte), a covered one with alpha > 0 does not; counted on its own
        before = np.zeros((H, W, 4), dtype=np.uint8) if key == "background" else (np.broadcast_to(np.array(CLEAR, dtype=np.uint8), (H, W, 4)) if base is None else base)
        changed = (np.asarray(images[key]) != before).any(axis=-1)
        mine = np.ones((H, W), dtype=bool) if (rows is None or key == "background") else np.broadcast_to(np.asarray(rows)[:, None], (H, W))
        uncovered_changed = int((mine & ~r["undecided"] & (r["layers"] == 0) & changed).sum())
        out.append("raster_rule %-18s %-13s %-11s share largest=%.4f mean=%.4f wrong=%d undecided=%d uncovered_changed=%d" %
                   (side, name, image, j["share_max"], j["share_mean"], j["wrong"], j["undecided"], uncovered_changed))
        log(out[-1])
        assert j["wrong"] == 0 and uncovered_changed == 0, (name, image, j["wrong"], uncovered_changed, np.argwhere(j["bad"])[:8].tolist())
        assert j["undecided"] <= int(UNDECIDED_CAP * W * H), (name, image, j["undecided"])
        if case["exact"]:
            assert j["undecided"] == 0, (name, image)
            if base is None:                                 # flat colours over the cleared buffer: one byte per channel, and the image is those bytes
                assert (r["lo"] == r["hi"]).all() and np.array_equal(np.asarray(images[key])[mine], r["lo"][mine]), (name, image)
    if "region" in case:
        # Covered exactly once, on the rule's own count and on the image itself.  The back buffer is cleared to alpha 1, so alpha cannot show it; red can: the source's
        # red is 1 at alpha 0.6 over red 0, which blends as alpha would over 0 -- none 0, once 153, twice 0.6 + 0.6 * 0.4 = 0.84 -> 214.
        f = rule["final"]
        mine = np.ones((H, W), dtype=bool) if rows is None else np.broadcast_to(np.asarray(rows)[:, None], (H, W))
        assert (f["layers"][case["region"] & mine] == 1).all() and not f["layers"][~mine].any() and not f["undecided"].any()
        if base is None:
            red = np.asarray(images["final"])[..., 0]
            assert (red[case["region"] & mine] == 153).all(), (name, "a tiled pixel was blended twice or not at all", np.unique(red[case["region"] & mine]).tolist())
            assert np.isin(red[mine], (0, 153)).all(), (name, np.unique(red[mine]).tolist())
    if shares and not case["over_ray_traced"] and rows is None:
        c = counts(case, rule)
        if "roundtrip_differs" in SHARES.get(name, {}):
            c["roundtrip_differs"] = roundtrip_differs(case, rule, base)
        out.append("raster_rule %-18s %-13s counts %s" % (side, name, {k: v for k, v in c.items() if v}))
        log(out[-1])
        for k, need in SHARES.get(name, {}).items():
            assert c[k] >= need, (name, k, c[k], need)
    return rule, out
