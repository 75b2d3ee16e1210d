"""Rules D1-D7 of the BC1-BC5 / BGRA8 / BGRX8 DDS formats (tests/bcn_rule.py, csrc/bcn.hip) on the CPU: the palettes against exact fractions for
every endpoint pair, D1 against bit replication, the whole decode against Pillow's DDS decoder, and the DDS writers."""
import io
import struct
from fractions import Fraction

import numpy as np
import pytest

import bcn_rule as R


def _byte(fr):
    """The exact value as a byte, rounded half up."""
    return int(fr * 255 + Fraction(1, 2))


def test_d1_formula_is_exact_rounding():
    for d in (31, 62, 93, 63, 126, 189, 7 * 255, 5 * 255):
        n = np.arange(0, 3 * d + 1)
        assert np.array_equal(R.unorm8(n, d)[: d + 1], [_byte(Fraction(int(k), d)) for k in n[: d + 1]])


def test_d1_differs_from_bit_replication():
    """4 of the 32 five-bit values and 10 of the 64 six-bit values: a decoder that widens endpoints by replication cannot match D1."""
    v5, v6 = np.arange(32), np.arange(64)
    d5 = np.nonzero(R.unorm8(v5, 31) != R.replicate(v5, 5))[0]
    d6 = np.nonzero(R.unorm8(v6, 63) != R.replicate(v6, 6))[0]
    assert len(d5) == 4 and len(d6) == 10, (d5, d6)
    assert np.abs(R.unorm8(v5, 31) - R.replicate(v5, 5)).max() == 1


@pytest.mark.parametrize("bits", [5, 6])
def test_colour_palette_against_fractions_for_every_endpoint_pair(bits):
    """D2 on one channel: every pair (v0, v1), both palettes, every entry, against Fraction arithmetic."""
    m = (1 << bits) - 1
    v0, v1 = np.meshgrid(np.arange(m + 1), np.arange(m + 1), indexing="ij")
    v0, v1 = v0.ravel(), v1.ravel()
    shift = {5: 11, 6: 5}[bits]
    ch = {5: 0, 6: 1}[bits]
    c0, c1 = v0 << shift, v1 << shift
    four = R.colour_palette(c0, c1, True)[:, :, ch]
    bc1 = R.colour_palette(c0, c1, False)
    for i in range(len(v0)):
        e0, e1 = Fraction(int(v0[i]), m), Fraction(int(v1[i]), m)
        want4 = [_byte(e0), _byte(e1), _byte((2 * e0 + e1) / 3), _byte((e0 + 2 * e1) / 3)]
        assert list(four[i]) == want4
        if c0[i] > c1[i]:
            assert list(bc1[i, :, ch]) == want4 and list(bc1[i, :, 3]) == [255] * 4
        else:
            assert list(bc1[i, :, ch]) == [_byte(e0), _byte(e1), _byte((e0 + e1) / 2), 0]
            assert list(bc1[i, :, 3]) == [255, 255, 255, 0]


def test_channel_palette_against_fractions_for_every_endpoint_pair():
    """D4: all 65 536 (a0, a1), both modes, every entry."""
    a0, a1 = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    a0, a1 = a0.ravel(), a1.ravel()
    got = R.channel_palette(a0, a1).astype(np.int64)
    k = np.arange(8)
    num7 = (8 - k[None, 2:]) * a0[:, None] + (k[None, 2:] - 1) * a1[:, None]          # / 7
    num5 = (6 - k[None, 2:6]) * a0[:, None] + (k[None, 2:6] - 1) * a1[:, None]        # / 5
    # exact halves never occur (odd denominators): round(N / d) = floor((2N + d) / 2d) equals the nearest integer
    want = np.zeros_like(got)
    want[:, 0], want[:, 1] = a0, a1
    eight = a0 > a1
    want[eight, 2:] = (2 * num7[eight] + 7) // 14
    want[~eight, 2:6] = (2 * num5[~eight] + 5) // 10
    want[~eight, 6], want[~eight, 7] = 0, 255
    assert np.array_equal(got, want)
    for (x, y) in ((255, 0), (0, 255), (200, 13), (13, 200), (7, 7), (128, 127)):
        p = R.channel_palette(np.array([x]), np.array([y]))[0]
        if x > y:
            exact = [Fraction(x)] + [Fraction(y)] + [Fraction((8 - j) * x + (j - 1) * y, 7) for j in range(2, 8)]
        else:
            exact = [Fraction(x), Fraction(y)] + [Fraction((6 - j) * x + (j - 1) * y, 5) for j in range(2, 6)] + [Fraction(0), Fraction(255)]
        assert [int(v) for v in p] == [int(e + Fraction(1, 2)) for e in exact]


def test_bc2_alpha_and_channel_mapping():
    """D3 and D5 on hand-made blocks."""
    alpha = sum(i << (4 * i) for i in range(16))
    colour = struct.pack("<HHI", 0xFFFF, 0x0000, 0)                    # every texel entry 0: white
    t = R.decode_blocks("BC2", np.frombuffer(struct.pack("<Q", alpha) + colour, dtype=np.uint8)[None])[0]
    assert list(t[:, 3]) == [17 * i for i in range(16)] and (t[:, :3] == 255).all()
    bc4 = np.frombuffer(struct.pack("<BB6x", 200, 100), dtype=np.uint8)[None]
    t = R.decode_blocks("BC4", bc4)[0]
    assert (t == [200, 0, 0, 255]).all()
    bc5 = np.frombuffer(struct.pack("<BB6xBB6x", 10, 20, 30, 40), dtype=np.uint8)[None]
    t = R.decode_blocks("BC5", bc5)[0]
    assert (t == [10, 30, 0, 255]).all()
    raw = np.arange(2 * 3 * 4, dtype=np.uint8)
    bgra = R.decode_level("BGRA8", raw, 3, 2)
    assert np.array_equal(bgra.reshape(-1, 4), raw.reshape(-1, 4)[:, [2, 1, 0, 3]])
    bgrx = R.decode_level("BGRX8", raw, 3, 2)
    assert (bgrx[..., 3] == 255).all() and np.array_equal(bgrx[..., :3], bgra[..., :3])


def test_layout_and_level_sizes():
    """D6: block (bx, by) covers texels (4 bx + i % 4, 4 by + i / 4), edge texels dropped; levels of ceil(w / 4) * ceil(h / 4) blocks."""
    w, h = 6, 5
    # 2 x 2 blocks; block b's BC4 endpoints a0 = a1 = 10 * b + 1 (every texel that value)
    raw = np.concatenate([np.frombuffer(struct.pack("<BB6x", 10 * b + 1, 10 * b + 1), dtype=np.uint8) for b in range(4)])
    t = R.decode_level("BC4", raw, w, h)[..., 0]
    want = np.array([[1] * 4 + [11] * 2] * 4 + [[21] * 4 + [31] * 2])
    assert np.array_equal(t, want)
    assert [R.level_bytes("BC1", *s) for s in R.level_sizes(5, 7, 3)] == [2 * 2 * 8, 1 * 1 * 8, 1 * 1 * 8]
    assert [R.level_bytes("BC3", *s) for s in R.level_sizes(130, 66, 8)] == [33 * 17 * 16, 17 * 9 * 16, 8 * 4 * 16, 4 * 2 * 16, 2 * 1 * 16, 16, 16, 16]     # 130x66 .. 1x1


def test_texel_index_bits():
    """D2 / D4: texel i takes bits 2i (colour) and 16 + 3i (8-bit endpoint block)."""
    for i in range(16):
        colour = struct.pack("<HHI", 0xF800, 0x001F, 1 << (2 * i))         # texel i entry 1 (blue), others entry 0 (red)
        t = R.decode_blocks("BC1", np.frombuffer(colour, dtype=np.uint8)[None])[0]
        assert (t[i] == [0, 0, 255, 255]).all() and (np.delete(t, i, 0) == [255, 0, 0, 255]).all()
        word = 255 | (0 << 8) | (1 << (16 + 3 * i))
        t = R.decode_blocks("BC4", np.frombuffer(struct.pack("<Q", word), dtype=np.uint8)[None])[0]
        assert t[i, 0] == 0 and (np.delete(t, i, 0)[:, 0] == 255).all()


@pytest.mark.parametrize("fmt,code", [("BC1", b"DXT1"), ("BC2", b"DXT3"), ("BC3", b"DXT5"), ("BC4", b"ATI1"), ("BC5", b"ATI2")])
def test_rule_against_pillow(fmt, code):
    """Pillow's DDS decoder on seeded random blocks: within 1 per channel everywhere (an independent check of bit, index and block order)."""
    pytest.importorskip("PIL")
    from PIL import Image
    rng = np.random.default_rng(20261016)
    for (w, h) in ((64, 32), (20, 12)):
        body = R.random_body(rng, fmt, w, h, 1)
        im = Image.open(io.BytesIO(R.dds(fmt, body, w, h, 1, ("fourcc", code)).tobytes()))
        im.load()
        got = np.asarray(im).astype(np.int64)
        mine = R.decode_chain(fmt, body, w, h, 1)[0].astype(np.int64)
        mine = mine[..., 0] if im.mode == "L" else mine[..., : got.shape[-1]]
        d = np.abs(got - mine)
        print("%s %dx%d: max %d, %.1f %% of channels differ by 1" % (fmt, w, h, d.max(), 100.0 * (d == 1).mean()))
        assert d.max() <= 1


def test_random_blocks_use_both_modes():
    rng = np.random.default_rng(5)
    b = R.random_body(rng, "BC1", 256, 256, 1).reshape(-1, 8)
    c0 = b[:, 0].astype(int) | b[:, 1].astype(int) << 8
    c1 = b[:, 2].astype(int) | b[:, 3].astype(int) << 8
    assert 0.45 < (c0 > c1).mean() < 0.55
    assert 0.45 < (b[:, 0] > b[:, 1]).mean() < 0.55


def test_dds_writers_and_encoder_round_trip():
    """Each spelling's header fields; the encoder's output decodes close to its input and BC1 transparent texels decode to (0, 0, 0, 0)."""
    body = np.arange(R.level_bytes("BC3", 8, 8), dtype=np.uint8)
    for fmt in R.FORMATS:
        for sp in R.spellings(fmt):
            f = R.dds(fmt, R.random_body(np.random.default_rng(0), fmt, 8, 4, 2), 8, 4, 2, sp).tobytes()
            assert f[:4] == b"DDS " and struct.unpack_from("<3I", f, 12)[0:2] == (4, 8) and struct.unpack_from("<I", f, 28)[0] == 2
            pf_flags, cc = struct.unpack_from("<I4s", f, 80)
            if sp[0] == "dx10":
                assert cc == b"DX10" and struct.unpack_from("<I", f, 128)[0] == sp[1]
            elif sp[0] == "fourcc":
                assert pf_flags & 4 and cc == sp[1]
            else:
                assert pf_flags & 0x40 and struct.unpack_from("<5I", f, 88) == (32,) + R.MASKS[fmt]
    assert len(R.dds("BC3", body, 8, 8, 1)) == 148 + len(body)
    rng = np.random.default_rng(9)
    y, x = np.mgrid[0:32, 0:32]
    img = np.stack([x * 8, y * 8, (x + y) * 4, 255 - x * 4], -1).astype(np.uint8)
    for fmt in ("BC1", "BC2", "BC3", "BC4", "BC5", "BGRA8", "BGRX8"):
        got = R.decode_chain(fmt, R.encode_chain(fmt, [img]), 32, 32, 1)[0].astype(int)
        ch = {"BC4": 1, "BC5": 2}.get(fmt, 3 if fmt in ("BC1", "BGRX8") else 4)
        assert np.abs(got[..., :ch] - img[..., :ch]).max() <= (0 if fmt.startswith("BGR") else 24), fmt
    mask = rng.random((32, 32)) < 0.2
    got = R.decode_chain("BC1", R.encode_chain("BC1", [img], transparent=mask), 32, 32, 1)[0]
    assert (got[mask] == 0).all() and (got[~mask][:, 3] == 255).all()
