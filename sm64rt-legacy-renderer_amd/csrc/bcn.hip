// bcn.hip -- BC1-BC5 block decoder and the BGRA8 / BGRX8 reorder: DDS textures of these formats are expanded to RGBA8 once at
// RT64_CreateTexture time, like BC7 (bc7.hip).
//
// The reference hands DDS files to the D3D12 runtime (rt64_texture.cpp:146-187, DDSTextureLoader12.cpp:555-849) and lets the texture units
// decode them while sampling.  D3D allows the hardware a tolerance, so nothing defines the result bit for bit; the library pins its rule
// (restated in numpy by tests/bcn_rule.py):
//   D1 Rounding   every decoded channel byte is the exact real value D3D defines, rounded half up: byte = (2 * 255 * N + D) div (2 * D) for
//                 the exact fraction N / D.  Endpoints are never widened to 8 bits by bit replication first.
//   D2 Colour     two 5:6:5 endpoints c0, c1, then 2-bit indices (texel i at bits 2i of the little-endian 32-bit word).  BC1 with c0 > c1 and
//                 every BC2 / BC3 colour block: e0, e1, (2 e0 + e1) / 3, (e0 + 2 e1) / 3.  BC1 with c0 <= c1: e0, e1, (e0 + e1) / 2 and
//                 transparent black.  e = v / 31, v / 63, v / 31.
//   D3 BC2 alpha  4 bits per texel at bits 4i of the little-endian 64-bit word: 17 a.
//   D4 BC3 alpha, BC4, BC5 channels: 8-bit endpoints a0, a1, then 3-bit indices in the following 48 bits.  a0 > a1: entries 2..7 are
//                 ((8 - k) a0 + (k - 1) a1) / 7; otherwise entries 2..5 are ((6 - k) a0 + (k - 1) a1) / 5, entry 6 is 0, entry 7 is 255.
//   D5 Channels   BC1 / BC2 / BC3 (r, g, b, a); BC4 (r, 0, 0, 255); BC5 (r, g, 0, 255), red block first; BGRA8 reordered; BGRX8 alpha 255.
//   D6 Layout     level m has ceil(w / 4) ceil(h / 4) blocks; block (bx, by) covers texels (4 bx + i % 4, 4 by + i / 4); texels past the
//                 level's edge are dropped.
//   D7 sRGB       the _SRGB variants store their bytes as they are (no linearisation), like R8G8B8A8_UNORM_SRGB and BC7_UNORM_SRGB.
//
// One launch decodes a texture's whole chain: one thread per 4 x 4 block (8- or 16-byte load, 16 x 4-byte stores), or one thread per texel
// for the 32-bit formats (in place: the raw texels are copied to the texel store first).
#include "kernels.h"

namespace {

struct BcnLevel { uint32_t firstBlock, texelOffset, w, h; };
struct BcnChain {
    BcnLevel level[RT64_MAX_MIPS];
    uint32_t levels, format;
    uint32_t count;                   // blocks of the whole chain (BC1-BC5) or texels (BGRA8 / BGRX8)
};

// D1: the byte of the exact fraction n / D, rounded half up.
template <uint32_t D> __device__ __forceinline__ uint32_t unorm8(uint32_t n) { return (510u * n + D) / (2u * D); }

__device__ __forceinline__ uint32_t rgba(uint32_t r, uint32_t g, uint32_t b, uint32_t a) { return r | (g << 8) | (b << 16) | (a << 24); }

// D2: the four palette entries of a colour block (c0 in the low half of `ends`); `four` forces the four-colour palette (BC2 / BC3).
struct Palette4 { uint32_t p0, p1, p2, p3; };
__device__ __forceinline__ Palette4 colour_palette(uint32_t ends, bool four) {
    const uint32_t c0 = ends & 0xFFFFu, c1 = ends >> 16;
    const uint32_t r0 = c0 >> 11, g0 = (c0 >> 5) & 63u, b0 = c0 & 31u, r1 = c1 >> 11, g1 = (c1 >> 5) & 63u, b1 = c1 & 31u;
    Palette4 p;
    p.p0 = rgba(unorm8<31>(r0), unorm8<63>(g0), unorm8<31>(b0), 255u);
    p.p1 = rgba(unorm8<31>(r1), unorm8<63>(g1), unorm8<31>(b1), 255u);
    if (four || c0 > c1) {
        p.p2 = rgba(unorm8<93>(2u * r0 + r1), unorm8<189>(2u * g0 + g1), unorm8<93>(2u * b0 + b1), 255u);
        p.p3 = rgba(unorm8<93>(r0 + 2u * r1), unorm8<189>(g0 + 2u * g1), unorm8<93>(b0 + 2u * b1), 255u);
    }
    else {
        p.p2 = rgba(unorm8<62>(r0 + r1), unorm8<126>(g0 + g1), unorm8<62>(b0 + b1), 255u);
        p.p3 = 0u;
    }
    return p;
}

// (value operands: a conditional of two struct members would select between their addresses and keep the palette in memory)
__device__ __forceinline__ uint32_t pick4(Palette4 p, uint32_t i) {
    const uint32_t lo = (i & 1u) ? uint32_t(p.p1) : uint32_t(p.p0), hi = (i & 1u) ? uint32_t(p.p3) : uint32_t(p.p2);
    return (i & 2u) ? hi : lo;
}

// D4: entry k of the palette of the 8-bit endpoints a0, a1.
__device__ __forceinline__ uint32_t channel(uint32_t a0, uint32_t a1, uint32_t k) {
    if (k < 2u) return k ? a1 : a0;
    if (a0 > a1) return (2u * ((8u - k) * a0 + (k - 1u) * a1) + 7u) / 14u;        // (510 N + 1785) / 3570
    if (k >= 6u) return k == 6u ? 0u : 255u;
    return (2u * ((6u - k) * a0 + (k - 1u) * a1) + 5u) / 10u;                       // (510 N + 1275) / 2550
}

// The 16 values of an 8-byte D4 block, texel i in out[i] (the caller shifts them into their channel).
__device__ __forceinline__ void channel_block(uint2 blk, uint32_t out[16]) {
    const uint32_t a0 = blk.x & 0xFFu, a1 = (blk.x >> 8) & 0xFFu;
    const unsigned long long bits = ((unsigned long long)blk.x | ((unsigned long long)blk.y << 32)) >> 16;
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = channel(a0, a1, (uint32_t)(bits >> (3 * i)) & 7u);
}

__global__ __launch_bounds__(256) void bcn_decode_kernel(const uint8_t *src, uint32_t *dst, BcnChain c) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= c.count) return;
    if (c.format == BCN_BGRA8 || c.format == BCN_BGRX8) {          // in place: this thread reads and writes texel t only
        const uint32_t v = reinterpret_cast<const uint32_t *>(src)[t];
        const uint32_t a = c.format == BCN_BGRX8 ? 0xFF000000u : (v & 0xFF000000u);
        dst[t] = (v & 0x0000FF00u) | ((v >> 16) & 0xFFu) | ((v & 0xFFu) << 16) | a;
        return;
    }
    // D6: the level of block t (levels are uniform across the wave: the loop reads the kernel arguments with scalar loads)
    BcnLevel L = c.level[0];
    for (uint32_t m = 1; m < c.levels; m++) if (t >= c.level[m].firstBlock) L = c.level[m];
    const uint32_t bw = (L.w + 3u) >> 2, local = t - L.firstBlock, by = local / bw, bx = local - by * bw;
    uint32_t texel[16];
    if (c.format == BCN_BC1) {
        const uint2 blk = reinterpret_cast<const uint2 *>(src)[t];
        const Palette4 p = colour_palette(blk.x, false);
#pragma unroll
        for (int i = 0; i < 16; i++) texel[i] = pick4(p, (blk.y >> (2 * i)) & 3u);
    }
    else if (c.format == BCN_BC2 || c.format == BCN_BC3) {
        const uint4 blk = reinterpret_cast<const uint4 *>(src)[t];
        const Palette4 p = colour_palette(blk.z, true);
        uint32_t alpha[16];
        if (c.format == BCN_BC2) {
#pragma unroll
            for (int i = 0; i < 16; i++) alpha[i] = 17u * (((i < 8 ? blk.x : blk.y) >> (4 * (i & 7))) & 15u);
        }
        else channel_block(make_uint2(blk.x, blk.y), alpha);
#pragma unroll
        for (int i = 0; i < 16; i++) texel[i] = (pick4(p, (blk.w >> (2 * i)) & 3u) & 0x00FFFFFFu) | (alpha[i] << 24);
    }
    else if (c.format == BCN_BC4) {
        channel_block(reinterpret_cast<const uint2 *>(src)[t], texel);
#pragma unroll
        for (int i = 0; i < 16; i++) texel[i] |= 0xFF000000u;
    }
    else {                                                          // BC5: red block, then green block
        const uint4 blk = reinterpret_cast<const uint4 *>(src)[t];
        uint32_t g[16];
        channel_block(make_uint2(blk.x, blk.y), texel);
        channel_block(make_uint2(blk.z, blk.w), g);
#pragma unroll
        for (int i = 0; i < 16; i++) texel[i] |= (g[i] << 8) | 0xFF000000u;
    }
    uint32_t *out = dst + L.texelOffset;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t x = 4u * bx + (uint32_t)(i & 3), y = 4u * by + (uint32_t)(i >> 2);
        if (x < L.w && y < L.h) out[(size_t)y * L.w + x] = texel[i];
    }
}

}  // namespace

uint32_t bcn_block_bytes(uint32_t format) {
    return format == BCN_BC1 || format == BCN_BC4 ? 8u : 16u;
}

hipError_t bcn_decode_launch(const uint8_t *src, uint8_t *rgba, uint32_t format, const uint32_t *mipOffset, uint32_t width, uint32_t height, int levels, hipStream_t stream) {
    if (format < BCN_BC1 || format > BCN_BGRX8 || levels < 1 || levels > RT64_MAX_MIPS || width == 0 || height == 0) return hipErrorInvalidValue;
    BcnChain c = {};
    c.levels = (uint32_t)levels; c.format = format;
    uint32_t blocks = 0;
    for (int m = 0; m < levels; m++) {
        const uint32_t w = std::max(width >> m, 1u), h = std::max(height >> m, 1u);
        c.level[m] = { blocks, mipOffset[m], w, h };
        blocks += ((w + 3u) / 4u) * ((h + 3u) / 4u);
    }
    const uint32_t lw = c.level[levels - 1].w, lh = c.level[levels - 1].h;
    c.count = format >= BCN_BGRA8 ? mipOffset[levels - 1] + lw * lh : blocks;
    hipLaunchKernelGGL(bcn_decode_kernel, dim3((c.count + 255u) / 256u), dim3(256), 0, stream, src, reinterpret_cast<uint32_t *>(rgba), c);
    return hipGetLastError();
}
