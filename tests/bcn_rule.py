"""Decode rules D1-D7 of the BC1-BC5 / BGRA8 / BGRX8 DDS formats (csrc/bcn.hip) restated in numpy, DDS writers in each spelling the
library accepts (DX10 header, legacy FourCC, legacy RGB masks), seeded random block data and a small block encoder that turns RGBA8 levels into
BCn files.  Test helper: imported by tests/test_bcn_rule.py and tests/test_gpu_bcn.py."""
import struct

import numpy as np

FORMATS = ("BC1", "BC2", "BC3", "BC4", "BC5", "BGRA8", "BGRX8")
BLOCK_BYTES = {"BC1": 8, "BC2": 16, "BC3": 16, "BC4": 8, "BC5": 16}
# DX10 dxgiFormat numbers (UNORM first, then _SRGB), legacy FourCCs and the legacy RGB masks (R, G, B, A) of every accepted spelling
DXGI = {"BC1": (71, 72), "BC2": (74, 75), "BC3": (77, 78), "BC4": (80,), "BC5": (83,), "BGRA8": (87, 91), "BGRX8": (88, 93)}
FOURCC = {"BC1": (b"DXT1",), "BC2": (b"DXT2", b"DXT3"), "BC3": (b"DXT4", b"DXT5"), "BC4": (b"ATI1", b"BC4U"), "BC5": (b"ATI2", b"BC5U")}
MASKS = {"BGRA8": (0x00FF0000, 0x0000FF00, 0x000000FF, 0xFF000000), "BGRX8": (0x00FF0000, 0x0000FF00, 0x000000FF, 0)}


def spellings(fmt):
    """Every accepted header spelling of a format: ("dx10", dxgi) / ("fourcc", code) / ("masks", None)."""
    out = [("dx10", d) for d in DXGI[fmt]] + [("fourcc", c) for c in FOURCC.get(fmt, ())]
    return out + ([("masks", None)] if fmt in MASKS else [])


# ---- D1 ----------------------------------------------------------------------------------------------------------------------------------

def unorm8(n, d):
    """D1: the byte of the exact fraction n / d, rounded half up: (2 * 255 * n + d) div (2 * d)."""
    n = np.asarray(n, dtype=np.int64)
    return (2 * 255 * n + d) // (2 * d)


def replicate(v, bits):
    """Bit replication to 8 bits -- what D1 is NOT."""
    v = np.asarray(v, dtype=np.int64)
    return (v << (8 - bits)) | (v >> (2 * bits - 8))


# ---- D2-D4 palettes ------------------------------------------------------------------------------------------------------------------------

def colour_palette(c0, c1, four):
    """D2: [..., 4, 4] uint8 palettes (r, g, b, a) of 16-bit endpoints c0, c1 (arrays); `four` forces the four-colour palette (BC2 / BC3)."""
    c0 = np.asarray(c0, dtype=np.int64); c1 = np.asarray(c1, dtype=np.int64)
    out = np.zeros(c0.shape + (4, 4), dtype=np.int64)
    three = (c0 <= c1) & (not four)
    for ch, (shift, bits) in enumerate(((11, 5), (5, 6), (0, 5))):
        m = (1 << bits) - 1
        v0, v1 = (c0 >> shift) & m, (c1 >> shift) & m
        out[..., 0, ch] = unorm8(v0, m)
        out[..., 1, ch] = unorm8(v1, m)
        out[..., 2, ch] = np.where(three, unorm8(v0 + v1, 2 * m), unorm8(2 * v0 + v1, 3 * m))
        out[..., 3, ch] = np.where(three, 0, unorm8(v0 + 2 * v1, 3 * m))
    out[..., :, 3] = 255
    out[..., 3, 3] = np.where(three, 0, 255)
    return out.astype(np.uint8)


def channel_palette(a0, a1):
    """D4: [..., 8] uint8 palettes of 8-bit endpoints a0, a1 (arrays)."""
    a0 = np.asarray(a0, dtype=np.int64); a1 = np.asarray(a1, dtype=np.int64)
    out = np.zeros(a0.shape + (8,), dtype=np.int64)
    out[..., 0], out[..., 1] = a0, a1
    eight = a0 > a1
    for k in range(2, 8):
        seven = unorm8((8 - k) * a0 + (k - 1) * a1, 7 * 255)
        if k <= 5:
            five = unorm8((6 - k) * a0 + (k - 1) * a1, 5 * 255)
        else:
            five = np.full_like(a0, 0 if k == 6 else 255)
        out[..., k] = np.where(eight, seven, five)
    return out.astype(np.uint8)


# ---- block decoding (D2-D5), levels (D6) ----------------------------------------------------------------------------------------------------

def _u64(b):
    """[n, 8] uint8 -> [n] uint64 little-endian."""
    return np.ascontiguousarray(b).view("<u8")[:, 0].astype(np.uint64)


def _colour_blocks(b, four):
    """[n, 8] colour blocks -> [n, 16, 4] texels."""
    c0 = b[:, 0].astype(np.int64) | (b[:, 1].astype(np.int64) << 8)
    c1 = b[:, 2].astype(np.int64) | (b[:, 3].astype(np.int64) << 8)
    idx = np.ascontiguousarray(b[:, 4:8]).view("<u4")[:, 0].astype(np.int64)
    sel = (idx[:, None] >> (2 * np.arange(16))) & 3
    pal = colour_palette(c0, c1, four)
    return np.take_along_axis(pal, sel[:, :, None], axis=1)


def _channel_blocks(b):
    """[n, 8] D4 blocks -> [n, 16] values."""
    bits = _u64(b) >> np.uint64(16)
    sel = ((bits[:, None] >> (3 * np.arange(16, dtype=np.uint64))) & np.uint64(7)).astype(np.int64)
    pal = channel_palette(b[:, 0], b[:, 1])
    return np.take_along_axis(pal, sel, axis=1)


def decode_blocks(fmt, raw):
    """D2-D5: [n, BLOCK_BYTES] uint8 blocks -> [n, 16, 4] uint8 texels (texel i of a block at x = i % 4, y = i // 4)."""
    raw = np.asarray(raw, dtype=np.uint8)
    n = raw.shape[0]
    if fmt == "BC1":
        return _colour_blocks(raw, False)
    if fmt in ("BC2", "BC3"):
        out = _colour_blocks(raw[:, 8:], True)
        if fmt == "BC2":
            a = ((_u64(raw[:, :8])[:, None] >> (4 * np.arange(16, dtype=np.uint64))) & np.uint64(15)).astype(np.int64) * 17
        else:
            a = _channel_blocks(raw[:, :8])
        out[:, :, 3] = a
        return out
    out = np.zeros((n, 16, 4), dtype=np.uint8)
    out[:, :, 3] = 255
    out[:, :, 0] = _channel_blocks(raw[:, :8])
    if fmt == "BC5":
        out[:, :, 1] = _channel_blocks(raw[:, 8:])
    return out


def level_sizes(w, h, mips):
    return [(max(1, w >> m), max(1, h >> m)) for m in range(mips)]


def level_bytes(fmt, w, h):
    """D6: bytes of one level in the file."""
    if fmt in BLOCK_BYTES:
        return ((w + 3) // 4) * ((h + 3) // 4) * BLOCK_BYTES[fmt]
    return w * h * 4


def decode_level(fmt, raw, w, h):
    """One level's bytes -> [h, w, 4] uint8 (D5, D6)."""
    raw = np.asarray(raw, dtype=np.uint8)
    if fmt in ("BGRA8", "BGRX8"):
        t = raw.reshape(h, w, 4)[..., [2, 1, 0, 3]].copy()
        if fmt == "BGRX8":
            t[..., 3] = 255
        return t
    bw, bh = (w + 3) // 4, (h + 3) // 4
    tex = decode_blocks(fmt, raw.reshape(bw * bh, BLOCK_BYTES[fmt])).reshape(bh, bw, 4, 4, 4)
    return np.ascontiguousarray(tex.transpose(0, 2, 1, 3, 4).reshape(bh * 4, bw * 4, 4)[:h, :w])


def decode_chain(fmt, body, w, h, mips):
    """Every level of a file body (the bytes after the header), level 0 first."""
    out, o = [], 0
    for (mw, mh) in level_sizes(w, h, mips):
        n = level_bytes(fmt, mw, mh)
        out.append(decode_level(fmt, body[o:o + n], mw, mh))
        o += n
    return out


def random_body(rng, fmt, w, h, mips):
    """Seeded random bytes for every level: random blocks use both BC1 modes and both D4 modes about equally."""
    n = sum(level_bytes(fmt, mw, mh) for (mw, mh) in level_sizes(w, h, mips))
    return rng.integers(0, 256, n, dtype=np.uint8)


# ---- DDS files ----------------------------------------------------------------------------------------------------------------------------

def dds(fmt, body, w, h, mips, spelling=("dx10", None)):
    """A DDS file (uint8 array) around `body`.  spelling: ("dx10", dxgiFormat or None for the first), ("fourcc", code or None), ("masks", None)."""
    kind, code = spelling
    flags = 0x1007 | (0x20000 if mips > 1 else 0)                   # CAPS | HEIGHT | WIDTH | PIXELFORMAT (| MIPMAPCOUNT)
    caps = 0x1000 | (0x400008 if mips > 1 else 0)
    pitch = level_bytes(fmt, w, h) if fmt in BLOCK_BYTES else w * 4
    flags |= 0x80000 if fmt in BLOCK_BYTES else 0x8                 # LINEARSIZE or PITCH
    masks = (0, 0, 0, 0)
    if kind == "dx10":
        pf_flags, cc, bits = 0x4, b"DX10", 0
    elif kind == "fourcc":
        pf_flags, cc, bits = 0x4, code or FOURCC[fmt][0], 0
    else:
        masks = MASKS[fmt]
        pf_flags, cc, bits = 0x40 | (0x1 if masks[3] else 0), b"\0\0\0\0", 32
    hdr = struct.pack("<4s7I44xII4s5I4I4x", b"DDS ", 124, flags, h, w, pitch, 0, mips, 32, pf_flags, cc, bits, *masks, caps, 0, 0, 0)
    if kind == "dx10":
        hdr += struct.pack("<5I", code or DXGI[fmt][0], 3, 0, 1, 0)
    return np.frombuffer(hdr + np.asarray(body, dtype=np.uint8).tobytes(), dtype=np.uint8).copy()


def dds_dx10_raw(dxgi, body, w, h, mips):
    """A DX10 DDS file of any dxgiFormat number (refusal tests)."""
    flags = 0x1007 | (0x20000 if mips > 1 else 0)
    hdr = struct.pack("<4s7I44xII4s5I4I4x", b"DDS ", 124, flags, h, w, 0, 0, mips, 32, 0x4, b"DX10", 0, 0, 0, 0, 0, 0x1000, 0, 0, 0)
    hdr += struct.pack("<5I", dxgi, 3, 0, 1, 0)
    return np.frombuffer(hdr + np.asarray(body, dtype=np.uint8).tobytes(), dtype=np.uint8).copy()


# ---- a small encoder (test data that looks like the sample's textures) -----------------------------------------------------------------------

def _blocks_of(img):
    """[h, w, 4] -> [bh * bw, 16, 4] int64, the level padded to whole blocks by repeating its last row / column."""
    h, w = img.shape[:2]
    bh, bw = (h + 3) // 4, (w + 3) // 4
    p = np.pad(img, ((0, bh * 4 - h), (0, bw * 4 - w), (0, 0)), mode="edge").astype(np.int64)
    return p.reshape(bh, 4, bw, 4, 4).transpose(0, 2, 1, 3, 4).reshape(bh * bw, 16, 4)


def _to565(rgb):
    return ((rgb[..., 0] * 31 + 127) // 255) << 11 | ((rgb[..., 1] * 63 + 127) // 255) << 5 | ((rgb[..., 2] * 31 + 127) // 255)


def _encode_colour(t, four, transparent=None):
    """[n, 16, 4] -> [n, 8] colour blocks: brightest and darkest texel as endpoints, each texel's nearest palette entry.  `transparent` ([n, 16]
    bool, BC1 only): those blocks use the three-colour palette and the masked texels index 3 (transparent black)."""
    lum = t[..., 0] * 2 + t[..., 1] * 4 + t[..., 2]
    hi = _to565(np.take_along_axis(t, lum.argmax(1)[:, None, None], 1)[:, 0])
    lo = _to565(np.take_along_axis(t, lum.argmin(1)[:, None, None], 1)[:, 0])
    c0, c1 = np.maximum(hi, lo), np.minimum(hi, lo)
    cut = transparent.any(1) if transparent is not None else np.zeros(len(t), dtype=bool)
    c0, c1 = np.where(cut, c1, c0), np.where(cut, c0, c1)             # three-colour blocks: c0 <= c1
    pal = colour_palette(c0, c1, four).astype(np.int64)                # [n, 4, 4]
    d = ((t[:, :, None, :3] - pal[:, None, :, :3]) ** 2).sum(-1)       # [n, 16, 4]
    if not four:
        d[:, :, 3] = np.where((c0 <= c1)[:, None], 1 << 40, d[:, :, 3])
    idx = d.argmin(-1)
    if transparent is not None:
        idx = np.where(transparent, 3, idx)
    word = (idx << (2 * np.arange(16))).sum(1)
    out = np.zeros((len(t), 8), dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = c0 & 255, c0 >> 8, c1 & 255, c1 >> 8
    out[:, 4:8] = word.astype("<u4").view(np.uint8).reshape(-1, 4)
    return out


def _encode_channel(v):
    """[n, 16] -> [n, 8] D4 blocks: a0 = max, a1 = min (the eight-value palette when they differ), each value's nearest entry."""
    a0, a1 = v.max(1), v.min(1)
    pal = channel_palette(a0, a1).astype(np.int64)
    idx = np.abs(v[:, :, None] - pal[:, None, :]).argmin(-1).astype(np.uint64)
    bits = (idx << (3 * np.arange(16, dtype=np.uint64))).sum(1, dtype=np.uint64)
    word = a0.astype(np.uint64) | (a1.astype(np.uint64) << np.uint64(8)) | (bits << np.uint64(16))
    return word.astype("<u8").view(np.uint8).reshape(-1, 8)


def encode_level(fmt, img, transparent=None):
    """An RGBA8 level ([h, w, 4]) as the bytes of one level of `fmt` (lossy: what matters to the tests is the decode)."""
    if fmt in ("BGRA8", "BGRX8"):
        return np.ascontiguousarray(img[..., [2, 1, 0, 3]]).reshape(-1)
    t = _blocks_of(img)
    tr = _blocks_of(transparent[..., None].repeat(4, -1))[..., 0].astype(bool) if transparent is not None else None
    if fmt == "BC1":
        b = _encode_colour(t, False, tr)
    elif fmt == "BC2":
        a = ((t[..., 3] * 15 + 127) // 255).astype(np.uint64)
        word = (a << (np.uint64(4) * np.arange(16, dtype=np.uint64))).sum(1, dtype=np.uint64)
        b = np.concatenate([word.astype("<u8").view(np.uint8).reshape(-1, 8), _encode_colour(t, True)], 1)
    elif fmt == "BC3":
        b = np.concatenate([_encode_channel(t[..., 3]), _encode_colour(t, True)], 1)
    elif fmt == "BC4":
        b = _encode_channel(t[..., 0])
    else:
        b = np.concatenate([_encode_channel(t[..., 0]), _encode_channel(t[..., 1])], 1)
    return np.ascontiguousarray(b).reshape(-1)


def encode_chain(fmt, levels, transparent=None):
    """A file body for RGBA8 levels; `transparent` ([h, w] bool, BC1) marks level-0 texels to make transparent."""
    return np.concatenate([encode_level(fmt, l, transparent if m == 0 else None) for m, l in enumerate(levels)])
