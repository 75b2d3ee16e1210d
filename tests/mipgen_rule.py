"""Mip rule M2-M4 of the device option generate_mipmaps (csrc/mipgen.hip) restated in numpy, and a packer that writes a chain as an
uncompressed RGBA8 DDS file (DX10 header, DXGI_FORMAT_R8G8B8A8_UNORM) -- the form in which the oracle, which generates no mips itself, is handed
the same levels the GPU made.  Test helper: imported by tests/test_mipgen_rule.py and tests/test_gpu_mipmaps.py."""
import copy
import struct

import numpy as np

MAX_MIPS = 16                  # RT64_MAX_MIPS (csrc/rt64_gpu.h)
DXGI_R8G8B8A8_UNORM = 28


def level_count(w, h):
    """M2: min(floor(log2(max(w, h))) + 1, RT64_MAX_MIPS)."""
    return min(int(max(w, h)).bit_length(), MAX_MIPS)


def level_sizes(w, h):
    """M2: (width, height) of every level."""
    return [(max(1, w >> m), max(1, h >> m)) for m in range(level_count(w, h))]


def axis_taps(s):
    """M3 along one axis of source size s: (taps [d, 3] int64, weights [d, 3] int64, D).  Unused taps carry weight 0 and index 0."""
    d = max(1, s >> 1)
    x = np.arange(d, dtype=np.int64)
    taps = np.zeros((d, 3), dtype=np.int64)
    wts = np.zeros((d, 3), dtype=np.int64)
    if s == 1:
        wts[:, 0] = 1
        return taps, wts, 1
    taps[:, 0], taps[:, 1] = 2 * x, 2 * x + 1
    if s % 2 == 0:
        wts[:, 0] = wts[:, 1] = 1
        return taps, wts, 2
    n = (s - 1) // 2
    taps[:, 2] = 2 * x + 2
    wts[:, 0], wts[:, 1], wts[:, 2] = n - x, n, x + 1
    return taps, wts, s


def next_level(src):
    """M3 + M4: level m from the stored level m - 1 ([h, w, 4] uint8) -> [max(1, h >> 1), max(1, w >> 1), 4] uint8."""
    src = np.ascontiguousarray(src)
    sh, sw = src.shape[:2]
    if sw % 2 == 0 and sh % 2 == 0:             # (a + b + c + d + 2) >> 2
        s = src.astype(np.uint16)
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    tx, wx, dx = axis_taps(sw)
    ty, wy, dy = axis_taps(sh)
    s = src.astype(np.int64)
    rows = sum(wx[None, :, i, None] * s[:, tx[:, i], :] for i in range(3))           # [sh, dw, 4]
    total = sum(wy[:, i, None, None] * rows[ty[:, i], :, :] for i in range(3))       # [dh, dw, 4]
    D = dx * dy
    return ((total + D // 2) // D).astype(np.uint8)


def chain(img):
    """Every level of an RGBA8 image ([h, w, 4] uint8) under M2-M4, level 0 first."""
    h, w = img.shape[:2]
    out = [np.ascontiguousarray(img, dtype=np.uint8)]
    for _ in range(level_count(w, h) - 1):
        out.append(next_level(out[-1]))
    return out


def dds_rgba8(levels):
    """A chain as the bytes of an uncompressed RGBA8 DDS file with mipCount = len(levels)."""
    h, w = levels[0].shape[:2]
    n = len(levels)
    flags = 0x1007 | 0x8 | (0x20000 if n > 1 else 0)              # CAPS | HEIGHT | WIDTH | PIXELFORMAT | PITCH (| MIPMAPCOUNT)
    caps = 0x1000 | ((0x400008) if n > 1 else 0)                  # TEXTURE (| COMPLEX | MIPMAP)
    hdr = struct.pack("<4s7I44xII4s5I4I4x", b"DDS ", 124, flags, h, w, w * 4, 0, n, 32, 4, b"DX10", 0, 0, 0, 0, 0, caps, 0, 0, 0)
    dx10 = struct.pack("<5I", DXGI_R8G8B8A8_UNORM, 3, 0, 1, 0)
    body = b"".join(np.ascontiguousarray(l, dtype=np.uint8).tobytes() for l in levels)
    return np.frombuffer(hdr + dx10 + body, dtype=np.uint8).copy()


def with_mip_chains(data):
    """A copy of a sample_scene.SceneData whose RGBA8 textures are replaced by DDS files holding their M2-M4 chains: what the library stores for
    them when generate_mipmaps is set.  DDS textures are kept as they are (M1)."""
    from sm64rt_legacy_renderer_amd import rt64, sample_scene
    d = copy.copy(data)
    d.textures = []
    for t in data.textures:
        if t.format == rt64.TEXTURE_FORMAT_RGBA8:
            d.textures.append(sample_scene.TextureData(t.name, rt64.TEXTURE_FORMAT_DDS, dds_rgba8(chain(t.data))))
        else:
            d.textures.append(t)
    return d
